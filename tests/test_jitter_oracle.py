"""CPU: the jittered render's contract (include/rt_api.h) on the oracle.  The hash's known answers; rt_jitter_sample
(host only, compiled from the functions the kernel calls) against the numpy levels of tests/jitter_common.py; the J = 1
pin on the numpy restatement; the fixtures made from the reference build (tests/golden/jitter.npz); the uniformity and
adjacency of the levels; the conditions that make each case of tests/test_gpu_jitter.py discriminating; and the CLI's
usage errors.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ray_tracer_fragment_shader_amd import abi, scenes

from . import dof_common as dc
from . import jitter_common as jc
from . import motion_common as mc
from . import ssaa_common as sc

SEEDS = (0, 1, 12345, 0xFFFFFFFF)
W, H = 19, 11                                # the GPU tests' frame at S = 2: a 38 x 22 sample frame
A, R, F = 8.0, 40.0, 1.0
# (S, J, w, h) of test_gpu_jitter.py's instance cases
SHAPES = [(2, 4, 19, 11), (4, 2, 11, 5), (8, 16, 3, 2), (1, 16, 19, 11)]
# the one-dimension cases on c2: (what, A, R, F, the dimensions it jitters beside the sub-pixel ones)
ONE_DIM = [("A only", A, 0.0, 0.0, (2, 3)), ("R only", 0.0, R, 0.0, (4, 5)), ("F only", 0.0, 0.0, F, (6,))]


def test_symbols_and_signatures():
    for name, n in (("rt_jitter_sample", 7), ("rt_render_jitter_dev", 16), ("rt_render_jitter", 17)):
        assert name in abi.SIGNATURES and len(abi.SIGNATURES[name][1]) == n and hasattr(abi.lib(), name)
    assert abi.lib().rt_abi_version() == 10


def test_known_answers():
    assert int(jc.fmix32(0)) == 0
    assert int(jc.fmix32(1)) == 0x514E28B7
    assert int(jc.fmix32(int(jc.fmix32(5)) ^ 7)) == 0xE80274BD
    # the same through the library: sample 5 of a one-row frame, seed 7, J = 16: the nibbles of the word
    lv = (ctypes.c_int32 * 7)()
    assert abi.lib().rt_jitter_sample(8, 1, 16, 7, 5, 0, lv) == abi.RT_OK
    assert list(lv) == [(0xE80274BD >> (4 * d)) & 15 for d in range(7)]


@pytest.mark.parametrize("J", [1, 2, 16])
def test_jitter_sample_is_the_numpy_levels(J):
    """Every sample of a 74 x 42 sample frame (a 37 x 21 frame at S = 2)."""
    L = abi.lib()
    lv = (ctypes.c_int32 * 7)()
    for seed in SEEDS:
        k = jc.levels(74, 42, J, seed)
        assert k.min() >= 0 and k.max() <= J - 1
        for Jr in range(42):
            for I in range(74):
                assert L.rt_jitter_sample(37, 2, J, seed, I, Jr, lv) == abi.RT_OK
                assert list(lv) == list(k[:, Jr, I]), (seed, I, Jr)


def test_jitter_sample_errors():
    L = abi.lib()
    lv = (ctypes.c_int32 * 7)()
    for args, word in (((37, 3, 4, 0, 0, 0), "samples"), ((37, 2, 3, 0, 0, 0), "jitter"), ((37, 2, 0, 0, 0, 0), "jitter"),
                       ((37, 2, 32, 0, 0, 0), "jitter"), ((0, 2, 4, 0, 0, 0), "size"), ((2 ** 30, 8, 4, 0, 0, 0), "size"),
                       ((37, 2, 4, 0, 74, 0), "sample"), ((37, 2, 4, 0, -1, 0), "sample"), ((37, 2, 4, 0, 0, -1), "sample"),
                       ((2 ** 15, 2, 4, 0, 0, 2 ** 15), "sample")):
        assert L.rt_jitter_sample(*args, lv) == abi.RT_EINVAL and word in abi.last_error(), args
    assert L.rt_jitter_sample(37, 2, 4, 0, 0, 0, None) == abi.RT_EINVAL and "null" in abi.last_error()


@pytest.mark.parametrize("SW,SH", [(64, 64), (74, 42)])
@pytest.mark.parametrize("seed", SEEDS)
def test_levels_are_uniform_and_uncorrelated(SW, SH, seed):
    """J = 16.  Uniformity: every level of every dimension occurs between 0.6 x and 1.5 x its expected count.
    Adjacency: the share of adjacent samples with equal level lies in [1 / 32, 1 / 8] (independent levels: 1 / 16)."""
    k = jc.levels(SW, SH, 16, seed)
    want = SW * SH / 16.0
    for d in range(7):
        counts = np.bincount(k[d].reshape(-1), minlength=16)
        assert len(counts) == 16
        assert 0.6 * want <= counts.min() and counts.max() <= 1.5 * want, (jc.DIMS[d], counts)
        for what, share in (("horizontally", (k[d][:, 1:] == k[d][:, :-1]).mean()),
                            ("vertically", (k[d][1:] == k[d][:-1]).mean())):
            assert 1 / 32 <= share <= 1 / 8, (jc.DIMS[d], what, share)


@pytest.mark.parametrize("seed", [0, 99])
@pytest.mark.parametrize("name,S", [("c2", 2), ("c2", 4), ("demo", 2)])
def test_one_sub_position_is_the_motion_render(name, S, seed):
    e = jc.expected(name, W, H, S, 1, seed, A, R, 0.75, mc.MOVES[name])
    m = mc.expected(name, W, H, S, A, R, 0.75, mc.MOVES[name])
    assert not e["k"].any()
    assert e["hi"].tobytes() == m["hi"].tobytes() and e["rgb"].tobytes() == m["rgb"].tobytes()
    assert np.array_equal(e["hi_rc"], m["hi_rc"]) and np.array_equal(e["rc2"], m["rc2"])


@pytest.mark.parametrize("key,name,S,J,seed,Ff,Af,Rf,lights,moves", jc.FIXTURES)
def test_fixtures_are_the_oracle_route(key, name, S, J, seed, Ff, Af, Rf, lights, moves):
    e = jc.expected(name, jc.FIX_W, jc.FIX_H, S, J, seed, Af, Rf, Ff, moves, lights)
    sc.assert_same_bits(jc.fixtures()[key], e["rgb"], key)


def test_pinhole_samples_are_pixels_of_the_fine_frame():
    """A = R = F = 0: sample (I, Jr) is pixel (J I + k_0, J Jr + k_1) of the fine camera's frame (po.render)."""
    from oracle import pyoracle as po
    S, J, seed = 2, 4, 1
    e = jc.expected("c2", W, H, S, J, seed, 0.0, 0.0, 0.0)
    scene, depth = sc.scene_of("c2")
    fine, fine_rc = po.render(scene.to_abi(), jc.fine_camera(e["cam"], S, J), S * J * W, S * J * H, depth)
    sm = jc.samples(e["cam"], W, H, S, J, seed, 0.0, 0.0, 0.0)
    assert jc.fine_gather(fine, sm["fine"]).tobytes() == e["hi"].tobytes()
    assert np.array_equal(jc.fine_gather(fine_rc, sm["fine"]), e["hi_rc"])


# ---- the conditions that make the GPU cases discriminating ----------------------------------------------------------
@pytest.mark.parametrize("S,J,w,h", SHAPES)
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_instance_frames_differ_from_the_regular_grid(name, S, J, w, h):
    e = jc.expected(name, w, h, S, J, 1, A, R, F, mc.MOVES[name])
    m = jc.expected(name, w, h, S, 1, 1, A, R, F, mc.MOVES[name])
    assert not np.isnan(e["rgb"]).any()
    assert dc.differ(e["rgb"], m["rgb"]).sum() >= 0.1 * w * h


@pytest.mark.parametrize("what,Af,Rf,Ff,dims", ONE_DIM)
def test_one_dimension_frames_need_their_dimension(what, Af, Rf, Ff, dims):
    moves = mc.MOVES["c2"]
    e = jc.expected("c2", W, H, 2, 4, 1, Af, Rf, Ff, moves)
    forced = jc.expected("c2", W, H, 2, 4, 1, Af, Rf, Ff, moves, force=dims)
    regular = jc.expected("c2", W, H, 2, 1, 1, Af, Rf, Ff, moves)
    assert dc.differ(e["rgb"], forced["rgb"]).sum() >= 10, what
    assert dc.differ(e["rgb"], regular["rgb"]).sum() >= 0.1 * W * H, what


def test_screen_point_frame_needs_the_sub_pixel_levels():
    e = jc.expected("c2", W, H, 2, 4, 1, 0.0, 0.0, 0.0)
    for dims in ((0,), (1,)):
        assert dc.differ(e["rgb"], jc.expected("c2", W, H, 2, 4, 1, 0.0, 0.0, 0.0, force=dims)["rgb"]).sum() >= 10


@pytest.mark.parametrize("case", [mc.shadow_only_case, mc.reflection_only_case, mc.fast_small_case])
def test_motion_discriminators_at_jittered_times(case):
    """S = 2, J = 8 on the 37 x 21 frames of the motion tests: the motion shows, and so does the time's jitter."""
    scene, depth, _, shutter, moves = case()
    cam = scenes.make_camera(37, 21, 500.0 / 37)
    d = mc.displacement(scene, moves)
    e = jc.render(scene, cam, 37, 21, depth, 2, 8, 1, 0.0, 0.0, shutter, d)
    e0 = jc.render(scene, cam, 37, 21, depth, 2, 8, 1, 0.0, 0.0, 0.0, d)
    ef = jc.render(scene, cam, 37, 21, depth, 2, 8, 1, 0.0, 0.0, shutter, d, force=(6,))
    assert dc.differ(sc.to_rgba8(e["rgb"]), sc.to_rgba8(e0["rgb"])).sum() >= 10
    assert dc.differ(e["rgb"], ef["rgb"]).sum() >= 10


def test_seeds_differ():
    e0 = jc.expected("c2", W, H, 2, 4, 0, A, R, F, mc.MOVES["c2"])
    e1 = jc.expected("c2", W, H, 2, 4, 1, A, R, F, mc.MOVES["c2"])
    assert dc.differ(e0["rgb"], e1["rgb"]).sum() >= 0.1 * W * H


def test_cli_usage_errors(tmp_path):
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    for args, word in ((["--jitter", "4"], "--samples"),
                       (["--samples", "2", "--jitter", "3"], "1, 2, 4, 8 or 16"),
                       (["--samples", "2", "--jitter", "0"], "1, 2, 4, 8 or 16"),
                       (["--samples", "2", "--jitter", "32"], "1, 2, 4, 8 or 16"),
                       (["--samples", "4", "--jitter", "4", "--adaptive", "8"], "--adaptive"),
                       (["--samples", "4", "--jitter", "4", "--coarse", "2", "--refine", "8"], "--refine"),
                       (["--samples", "4", "--jitter", "4", "--faithful", "glibc"], "--faithful"),
                       (["--samples", "4", "--jitter", "4", "--gpus", "2"], "--gpus")):
        r = subprocess.run([exe, "--config", "c2", "--out", str(tmp_path / "x.ppm")] + args, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert "--jitter" in r.stderr and word in r.stderr, (args, r.stderr)
        assert not (tmp_path / "x.ppm").exists()


def test_nan_frame_has_some_nans():
    e = jc.expected("tree_c2", W, H, 2, 4, 1, 0.0, 0.0, F, mc.MOVES["tree_c2"])
    nan_px = np.isnan(e["rgb"]).any(axis=2)
    assert 0 < nan_px.sum() <= 0.25 * W * H
