"""Adaptive sampling of the lens family's renders on the CPU: the three new symbols (the ABI version stays 10),
rt_lens_adaptive_workspace_bytes, the pins of the contract on its numpy restatement (tests/lens_adaptive_common.py),
the fixtures made from the reference build (tests/golden/lens_adaptive.npz), the conditions that make each case of
tests/test_gpu_lens_adaptive.py discriminating, and the CLI's usage errors.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes

from . import adaptive_common as ac
from . import dof_common as dc
from . import lens_adaptive_common as la
from . import motion_common as mc
from . import soft_common as so
from . import ssaa_common as sc

W, H = 37, 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVES = mc.MOVES
A, R, F, T = 8.0, 40.0, 0.75, 32


def test_symbols_and_abi_version():
    L = abi.lib()
    assert L.rt_abi_version() == 10 and abi.ABI_VERSION == 10
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_api.h")).read(), flags=re.S)
    for name in ("rt_lens_adaptive_workspace_bytes", "rt_render_lens_adaptive_dev", "rt_render_lens_adaptive"):
        assert hasattr(L, name), name
        assert name in abi.SIGNATURES
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    assert len(abi.SIGNATURES["rt_lens_adaptive_workspace_bytes"][1]) == 3
    assert len(abi.SIGNATURES["rt_render_lens_adaptive_dev"][1]) == 19
    assert len(abi.SIGNATURES["rt_render_lens_adaptive"][1]) == 19


# the workspace -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (37, 21), (131, 100), (1920, 1080), (65536, 32768)])
def test_workspace_bytes_cover_the_layout(w, h):
    """The counter, the work list (one uint32 per pixel), one spread byte per pixel and the coarse RGBA8 image."""
    n = ctypes.c_size_t(7)
    assert abi.lib().rt_lens_adaptive_workspace_bytes(w, h, ctypes.byref(n)) == abi.RT_OK
    npx = w * h
    assert n.value >= 4 + 4 * npx + npx + 4 * npx
    assert n.value <= 9 * npx + 5 * 256, "more than the layout and its alignment"
    plain = ctypes.c_size_t()
    assert abi.lib().rt_adaptive_workspace_bytes(w, h, 2, ctypes.byref(plain)) == abi.RT_OK
    assert n.value >= plain.value + npx


def test_workspace_bytes_argument_errors():
    L = abi.lib()
    n = ctypes.c_size_t(7)
    for w, h in ((0, 5), (5, 0), (-1, 5), (5, -3), (65536, 32769), (2 ** 30, 3)):
        n.value = 7
        assert L.rt_lens_adaptive_workspace_bytes(w, h, ctypes.byref(n)) == abi.RT_EINVAL, (w, h)
        assert "size" in abi.last_error() and n.value == 0
    assert L.rt_lens_adaptive_workspace_bytes(5, 5, None) == abi.RT_EINVAL and "null" in abi.last_error()


# rule 2 by hand ------------------------------------------------------------------------------------------------
def test_spread_by_hand():
    """A 2 x 1 frame at S = 2: pixel 0's samples have the red bytes 0, 26, 51, 255 and a NaN blue; pixel 1's agree."""
    hi = np.zeros((2, 4, 3))
    hi[0, 0, 0], hi[0, 1, 0], hi[1, 0, 0], hi[1, 1, 0] = -3.0, 0.1, 0.2, 7.0
    hi[1, 1, 2] = np.nan
    hi[:, 2:] = (0.5, 0.25, 0.125)
    assert la.spread_of(hi, 2).tolist() == [[255, 0]]
    hi[1, 1, 0] = 0.31
    assert la.spread_of(hi, 2).tolist() == [[79, 0]]
    hi[1, 1, 2] = 0.4                                          # the blue bytes 0, 0, 0, 102
    assert la.spread_of(hi, 2).tolist() == [[102, 0]]
    assert la.spread_of(hi[::2, ::2], 1).tolist() == [[0, 0]]


# rule 4 on the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_threshold_pins(name):
    lo = mc.expected(name, W, H, 2, A, R, F, MOVES[name])
    hi = mc.expected(name, W, H, 4, A, R, F, MOVES[name])
    e = la.expected(name, W, H, 2, 4, 255, A, R, F, MOVES[name])
    assert not e["mask"].any()
    sc.assert_same_bits(e["rgb"], lo["rgb"], "T = 255")
    assert np.array_equal(e["rc2"], lo["rc2"])
    e = la.expected(name, W, H, 2, 4, -1, A, R, F, MOVES[name])
    assert e["mask"].all() and e["a"].all()
    sc.assert_same_bits(e["rgb"], hi["rgb"], "T = -1")
    assert np.array_equal(e["rc2"], hi["rc2"])
    for t in (-1, 0, 32, 255):
        e = la.expected(name, W, H, 4, 4, t, A, R, F, MOVES[name])
        sc.assert_same_bits(e["rgb"], hi["rgb"], f"S_lo = S_hi, T = {t}")
        assert np.array_equal(e["rc2"], hi["rc2"])


def test_one_pixel_frame():
    scene, depth = sc.scene_of("c2")
    cam = scenes.make_camera(1, 1, 500.0 / 37)
    d = mc.displacement(scene, MOVES["c2"])
    assert la.render(scene, cam, 1, 1, depth, 2, 4, -1, A, R, F, d)["mask"].all()
    assert not la.render(scene, cam, 1, 1, depth, 1, 4, 0, A, R, F, d)["mask"].any()
    assert not ac.refine_mask(np.zeros((1, 1, 4), np.uint8), -1).any()


@pytest.mark.parametrize("name", ["c2", "demo"])
def test_one_coarse_sample_has_no_spread(name):
    e = la.expected(name, W, H, 1, 4, 0, A, R, F, MOVES[name])
    assert not e["a"].any() and e["b"].any()


@pytest.mark.parametrize("name,S", ac.FIXTURES)
def test_pinhole_frozen_one_coarse_sample_is_the_adaptive_render(name, S):
    """A = R = F = 0, S_lo = 1, T >= 0: rt_render_adaptive_dev's frame, its fixture and its mask."""
    fx = ac.fixtures()
    e = la.expected(name, ac.FIX_W, ac.FIX_H, 1, S, ac.FIX_T, 0.0, 0.0, 0.0)
    want = ac.expected(name, ac.FIX_W, ac.FIX_H, S, ac.FIX_T)
    sc.assert_same_bits(e["rgb"], want["rgb"], name)
    assert np.array_equal(e["rc2"], want["rc2"]) and np.array_equal(e["mask"], want["mask"])
    key = sc.fixture_key(name, S)
    sc.assert_same_bits(e["rgb"], fx[key], key)


def test_reductions_to_the_other_renders():
    """F = 0 is the soft frame, R = 0 as well the lens frame, A = 0 as well the supersampled one, at both levels."""
    for S in (2, 4):
        sc.assert_same_bits(mc.expected("c2", W, H, S, A, R, 0.0, MOVES["c2"])["rgb"],
                            so.expected("c2", W, H, S, A, R)["rgb"], "soft")
        sc.assert_same_bits(mc.expected("c2", W, H, S, A, 0.0, 0.0)["rgb"], dc.expected("c2", W, H, S, A)["rgb"], "dof")
        sc.assert_same_bits(mc.expected("c2", W, H, S, 0.0, 0.0, 0.0)["rgb"], sc.expected("c2", W, H, S)["rgb"], "ss")


# fixtures --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,S_lo,S_hi,Ff,Af,Rf,lights,moves", la.FIXTURES)
def test_oracle_route_reproduces_fixture(key, name, S_lo, S_hi, Ff, Af, Rf, lights, moves):
    fx = la.fixtures()
    assert sorted(fx) == sorted([f[0] for f in la.FIXTURES] + [f[0] + "_mask" for f in la.FIXTURES])
    want, mask = fx[key], fx[key + "_mask"]
    assert want.shape == (la.FIX_H, la.FIX_W, 3) and want.dtype == np.float64
    assert mask.shape == (la.FIX_H, la.FIX_W) and mask.dtype == np.uint8
    e = la.expected(name, la.FIX_W, la.FIX_H, S_lo, S_hi, la.FIX_T, Af, Rf, Ff, moves, lights)
    sc.assert_same_bits(e["rgb"], want, key)
    assert np.array_equal(e["mask"], mask.astype(bool))
    share = mask.mean()
    print(f"{key}: refined share {share:.3f}")
    assert 0.05 < share < 0.95
    if name == "tree_c2":
        assert np.isnan(want).any(), "the NaN fixture has no NaN"


@pytest.mark.ref
@pytest.mark.parametrize("key,name,S_lo,S_hi,Ff,Af,Rf,lights,moves", la.FIXTURES)
def test_reference_build_reproduces_fixture(key, name, S_lo, S_hi, Ff, Af, Rf, lights, moves):
    if not po.ref_available():
        pytest.skip("no reference build here")
    scene, depth = sc.scene_of(name)
    cam = scenes.make_camera(la.FIX_W, la.FIX_H, 500.0 / la.FIX_W)
    d = mc.displacement(scene, moves)
    hi = mc.render_ref(scene, cam, la.FIX_W, la.FIX_H, depth, S_hi, Af, Rf, Ff, d, lights)
    lo = mc.render_ref(scene, cam, la.FIX_W, la.FIX_H, depth, S_lo, Af, Rf, Ff, d, lights)
    mask = la.fixtures()[key + "_mask"].astype(bool)
    sc.assert_same_bits(np.where(mask[..., None], hi, lo), la.fixtures()[key], key)


# the conditions of the GPU cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_variant_cases_are_discriminating(name):
    """(2, 4): both criteria flag pixels the other does not, and taking the wrong level on either side of the mask
    changes pixels."""
    e = la.expected(name, W, H, 2, 4, T, A, R, F, MOVES[name])
    share, a_only, b_only, unref_diff, ref_diff = la.census(e)
    print(f"{name} (2, 4): share {share:.3f}, (a) only {a_only}, (b) only {b_only}, unrefined and different "
          f"{unref_diff}, refined and different {ref_diff}")
    assert 0.3 <= share <= 0.8 and a_only >= 5 and b_only >= 50 and unref_diff >= 5 and ref_diff >= 200
    e = la.expected(name, W, H, 1, 4, T, A, R, F, MOVES[name])
    share, _, _, unref_diff, _ = la.census(e)
    print(f"{name} (1, 4): share {share:.3f}, unrefined and different {unref_diff}")
    # (the range is stated to two decimals: c5's share is 23 / 37 = 0.6216)
    assert 0.35 <= round(share, 2) <= 0.62 and unref_diff >= 47


@pytest.mark.parametrize("pair", [(2, 8), (4, 8)])
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_eight_sample_cases(name, pair):
    e = la.expected(name, W, H, pair[0], pair[1], T, A, R, F, MOVES[name])
    assert 0.05 < e["mask"].mean() < 0.95


def test_compaction_case():
    """131 x 100 at T = 8: both criteria at work, and refined pixels in both 8192-pixel compaction workgroups."""
    e = la.expected("c2", 131, 100, 2, 4, 8, A, R, F, MOVES["c2"])
    share, a_only, b_only, _, _ = la.census(e)
    print(f"c2 131 x 100 T = 8: share {share:.3f}, (a) only {a_only}, (b) only {b_only}")
    assert a_only >= 100 and b_only >= 300 and 0.15 < share < 0.5
    flat = e["mask"].reshape(-1)
    assert flat[:8192].any() and flat[8192:].any()


def test_nan_frame_condition():
    e = la.expected("tree_c2", W, H, 2, 4, T, 0.0, 0.0, 1.0, MOVES["tree_c2"])
    nan_px = np.isnan(e["rgb"]).any(axis=2)
    assert e["depth"] == 3 and 0 < nan_px.sum() <= 0.25 * W * H
    assert 0 < e["mask"].sum() < W * H


# the CLI -------------------------------------------------------------------------------------------------------
def test_cli_usage_errors(tmp_path):
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    for args, word in ((["--samples", "4", "--coarse", "2"], "--refine"),
                       (["--samples", "4", "--refine", "8"], "--coarse"),
                       (["--coarse", "2", "--refine", "8"], "--samples"),
                       (["--samples", "2", "--coarse", "4", "--refine", "8"], "--coarse"),
                       (["--samples", "4", "--coarse", "2", "--refine", "8", "--adaptive", "8"], "--adaptive"),
                       (["--samples", "4", "--coarse", "2", "--refine", "8", "--faithful", "glibc"], "--faithful"),
                       (["--samples", "4", "--coarse", "2", "--refine", "8", "--gpus", "2"], "--gpus"),
                       (["--samples", "4", "--adaptive", "8", "--aperture", "8"], "--adaptive"),
                       (["--samples", "4", "--adaptive", "8", "--light-size", "40"], "--adaptive"),
                       (["--samples", "4", "--adaptive", "8", "--shutter", "1"], "--adaptive")):
        r = subprocess.run([exe, "--config", "c2", "--out", str(tmp_path / "x.ppm")] + args, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert word in r.stderr, (args, r.stderr)
        assert not (tmp_path / "x.ppm").exists()
