"""CPU: the converging render's contract (include/rt_api.h: converging accumulation) on the oracle.  The symbols; the
pins of rule 5 on the numpy restatement (tests/converge_common.py); the fixture made from the reference build
(tests/golden/converge.npz); the conditions that make each case of tests/test_gpu_converge.py discriminating — pixels
stop at M, later and not at all, whole tiles stop and others stay mixed, loosely stopped pixels resume, and a fused sum
of squares or a local partial sum gives other bits; and the CLI's usage errors.  No GPU."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes
from ray_tracer_fragment_shader_amd.tracer import Tracer

from . import accum_common as ac
from . import converge_common as cc
from . import dof_common as dc
from . import motion_common as mc
from . import shutter_common as hc
from . import ssaa_common as sc
from .test_jitter_oracle import SHAPES

W, H = 19, 11                                # the GPU tests' frame at S = 2: a 38 x 22 sample frame, 15 tiles
A, R, F = 8.0, 40.0, 1.0
MOVES = mc.MOVES
M = 3
# (S, J, E, K): the main case, the strict case and the S = 1 case of tests/test_gpu_converge.py
MAIN, STRICT, ONE = (2, 4, 1.0 / 32.0, 16), (2, 4, 1.0 / 255.0, 10), (1, 16, 1.0 / 8.0, 16)
# the budget and tolerance of the every-instance cases over test_jitter_oracle.SHAPES
INST_K, INST_E = 6, 1.0 / 64.0


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    for name in ("rt_render_converge_dev", "rt_render_converge"):
        assert name in abi.SIGNATURES and hasattr(abi.lib(), name), name


def _c2(S, J, E, K, seed=1):
    return cc.expected("c2", "crane", W, H, S, J, seed, K, M, E, A, R, F, MOVES["c2"])


def _c2_frames(S, J, seed=1):
    return cc.frames("c2", "crane", W, H, S, J, seed, A, R, F, MOVES["c2"])


def test_symbols_and_signatures():
    for name, n in (("rt_render_converge_dev", 24), ("rt_render_converge", 25)):
        assert len(abi.SIGNATURES[name][1]) == n
    assert abi.lib().rt_abi_version() == 10
    for method in ("alloc_converge", "render_converge_into", "render_converge"):
        assert callable(getattr(Tracer, method))


def test_render_entry_points_reject_before_any_device_work():
    L = abi.lib()
    cam = scenes.make_camera(W, H, 1.0)
    buf = (ctypes.c_double * (3 * W * H))()
    cnt = (ctypes.c_uint32 * (W * H))()
    rc = L.rt_render_converge_dev(None, ctypes.byref(cam), None, W, H, 1, 2, 4, 1, 3, 3, 0.01, A, R, F, buf, buf, cnt,
                                  None, None, None, None, None, None)
    assert rc == abi.RT_EINVAL and "context" in abi.last_error()
    rc = L.rt_render_converge(None, None, None, ctypes.byref(cam), None, W, H, 1, 2, 4, 1, 3, 3, 0.01, A, R, F, buf, buf,
                              cnt, None, None, None, None, None)
    assert rc == abi.RT_EINVAL and "context" in abi.last_error()


# ---- the numpy restatement itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
def test_nothing_stops_is_the_accumulating_render(K):
    """M > K from a zeroed count: acc, mean and counters are accum_common.accumulate's, count = K, all active."""
    fo = _c2_frames(2, 4)
    r = cc.converge(fo, cc.zero_state(H, W), K, K + 1, 1.0 / 32.0)
    a = ac.expected("c2", "crane", W, H, 2, 4, 1, 0, K, A, R, F, MOVES["c2"])
    assert r["acc"].tobytes() == a["acc"].tobytes() and r["mean"].tobytes() == a["mean"].tobytes()
    assert np.array_equal(r["rc2"], a["rc2"]) and (r["n"] == K).all() and r["active"] == W * H
    if K == 1:
        assert r["mean"].tobytes() == hc.expected("c2", "crane", W, H, 2, 4, 1, A, R, F, MOVES["c2"])["rgb"].tobytes()


def test_a_pixel_with_count_n_holds_the_sum_of_n_passes():
    e = _c2(*MAIN)
    for n in np.unique(e["n"]):
        a = ac.expected("c2", "crane", W, H, 2, 4, 1, 0, int(n), A, R, F, MOVES["c2"])
        m = e["n"] == n
        assert e["acc"][m].tobytes() == a["acc"][m].tobytes(), n


def test_split_calls_continue_the_same_state():
    S, J, E, K = MAIN
    fo, whole = _c2_frames(S, J), _c2(*MAIN)
    for plan in ((6, 10), (1,) * 16):
        st, rc = cc.zero_state(H, W), np.zeros((H, W, 2), np.uint32)
        for k in plan:
            r = cc.converge(fo, st, k, M, E)
            st, rc = cc.state_of(r), rc + r["rc2"]
        for key in ("acc", "sq", "n", "mean"):
            assert r[key].tobytes() == whole[key].tobytes(), (plan, key)
        assert np.array_equal(rc, whole["rc2"]) and r["active"] == whole["active"]


# ---- the conditions that make the GPU cases discriminating ----------------------------------------------------------
def test_main_case_has_every_class_of_pixel_and_of_tile():
    S, J, E, K = MAIN
    n = _c2(*MAIN)["n"]
    at_m, later, never = (n == M).sum(), ((n > M) & (n < K)).sum(), (n == K).sum()
    assert at_m + later + never == W * H
    assert min(at_m, later, never) >= 0.1 * W * H, (at_m, later, never)
    tiles = cc.tile_counts(n, S)
    assert len(tiles) == 15
    assert sum((t < K).all() for t in tiles) >= 1            # wholly stopped before the budget: the wave leaves early
    assert sum((t < K).any() and (t == K).any() for t in tiles) >= 1      # mixed: stopped lanes in a live wave


def test_strict_case_has_a_tile_in_which_no_pixel_stops():
    S, J, E, K = STRICT
    e = _c2(*STRICT)
    assert sum((t == K).all() for t in cc.tile_counts(e["n"], S)) >= 1
    assert (e["n"] == M).sum() >= 0.1 * W * H and e["active"] >= 0.1 * W * H


def test_one_sample_case_stops_most_pixels():
    S, J, E, K = ONE
    n = _c2(*ONE)["n"]
    assert (n == M).sum() >= 0.1 * W * H and ((n > M) & (n < K)).sum() >= 0.1 * W * H and (n == K).sum() >= 1


def test_loosely_stopped_pixels_resume_under_a_smaller_tolerance():
    fo = _c2_frames(2, 4)
    a = cc.converge(fo, cc.zero_state(H, W), 6, M, 1.0 / 8.0)
    loose = cc.stopped(a["acc"], a["sq"], a["n"], M, 1.0 / 8.0)
    b = cc.converge(fo, cc.state_of(a), 10, M, 1.0 / 32.0)
    resumed = loose & (b["received"] > 0)
    assert loose.sum() >= 0.5 * W * H and resumed.sum() >= 0.1 * loose.sum(), (loose.sum(), resumed.sum())
    assert (loose & (b["received"] == 0)).sum() >= 0.1 * W * H            # and others stay stopped
    # a pixel's passes have no gap: what it holds is still the sum of its first n passes
    for n in np.unique(b["n"]):
        ref = ac.expected("c2", "crane", W, H, 2, 4, 1, 0, int(n), A, R, F, MOVES["c2"])
        assert b["acc"][b["n"] == n].tobytes() == ref["acc"][b["n"] == n].tobytes(), n


@pytest.mark.parametrize("S,J,w,h", SHAPES)
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_instance_cases_have_stopped_and_running_pixels(name, S, J, w, h):
    """S = 8 needs J >= 2: with J = 1 every pass is the same frame and everything stops at M."""
    e = cc.expected(name, "crane", w, h, S, J, 1, INST_K, M, INST_E, A, R, F, MOVES[name])
    assert (e["n"] == M).sum() >= 1 and (e["n"] == INST_K).sum() >= 1, np.bincount(e["n"].ravel())


def test_one_sub_position_stops_everything_at_m():
    e = cc.expected("c2", "crane", 3, 2, 8, 1, 1, INST_K, M, INST_E, A, R, 0.0, MOVES["c2"])
    assert (e["n"] == M).all() and e["active"] == 0


def test_a_fused_sum_of_squares_shows_in_the_bits():
    """Six passes with nothing stopping: sq = fma(v, v, sq), the exact product added and rounded once, is another
    value than rule 2's rounded product."""
    fo = _c2_frames(2, 4)
    r = cc.converge(fo, cc.zero_state(H, W), 6, 7, 0.0)
    fused = None
    for p in range(6):
        v = fo(p)[0].ravel()
        if fused is None:
            fused = v * v
        else:
            fused = np.array([float(Fraction(x) * Fraction(x) + Fraction(s)) for x, s in zip(v, fused)])
    assert not np.isnan(r["sq"]).any()
    assert (fused != r["sq"].ravel()).sum() >= 20


def test_a_local_partial_sum_shows_in_the_bits():
    """Summing a call's passes apart and adding that sum to accum is another value than rule 2's."""
    fo = _c2_frames(2, 4)
    a = cc.converge(fo, cc.zero_state(H, W), 2, 7, 0.0)
    b = cc.converge(fo, cc.state_of(a), 3, 7, 0.0)
    local = a["acc"] + ((fo(2)[0] + fo(3)[0]) + fo(4)[0])
    assert dc.differ(b["acc"], local).sum() >= 10


def test_last_pass_number():
    """n = 2^31 - 1, M = 2, E = 0, K = 3: one pass, with the seed + 2^31 - 1, then n = 2^31 stops the pixel for good."""
    fo = cc.frames("c2", "crane", 3, 2, 2, 4, 5, A, R, F, MOVES["c2"], pitch_w=37)
    first = fo(0)[0]
    st = (first.copy(), first * first, np.full((2, 3), 2 ** 31 - 1, np.int64))
    r = cc.converge(fo, st, 3, 2, 0.0)
    assert (r["n"] == 2 ** 31).all() and (r["received"] == 1).all() and r["active"] == 0
    v = hc.expected("c2", "crane", 3, 2, 2, 4, ac.seed_of(5, 2 ** 31 - 1), A, R, F, MOVES["c2"], pitch_w=37)["rgb"]
    assert r["acc"].tobytes() == (first + v).tobytes()


def test_nan_passes_do_not_hold_a_pixel_back():
    e = cc.expected("tree_c2", "crane", W, H, 2, 4, 1, 6, M, 1.0 / 32.0, 0.0, 0.0, F, MOVES["tree_c2"])
    nan_px = np.isnan(e["acc"]).any(axis=2)
    assert 0 < nan_px.sum() <= W * H / 3
    assert (e["n"][np.isnan(e["acc"]).all(axis=2)] == M).all() and np.isnan(e["acc"]).all(axis=2).sum() >= 1


# ---- the fixture --------------------------------------------------------------------------------------------------------
def _fixture_case():
    key, base, seed, K, Mf, E = cc.FIXTURE
    name, S, J, Ff, Af, Rf, lights, moves, motion = ac.shutter_fixture(base)
    return key, name, motion, S, J, seed, K, Mf, E, Af, Rf, Ff, moves, lights


def test_fixture_is_the_oracle_route():
    key, name, motion, S, J, seed, K, Mf, E, Af, Rf, Ff, moves, lights = _fixture_case()
    e = cc.expected(name, motion, cc.FIX_W, cc.FIX_H, S, J, seed, K, Mf, E, Af, Rf, Ff, moves, lights)
    fx = cc.fixtures()
    for k in ("acc", "sq", "mean"):
        sc.assert_same_bits(fx[f"{key}_{k}"], e[k], f"{key} {k}")
    assert fx[key + "_count"].dtype == np.uint32 and np.array_equal(fx[key + "_count"], e["n"])
    hist = np.bincount(e["n"].ravel(), minlength=K + 1)
    assert hist[Mf] >= 10 and hist[K] >= 10 and (hist[Mf + 1:K] > 0).sum() >= 3, hist    # the counts are mixed


@pytest.mark.ref
def test_reference_build_agrees_with_the_oracle_route():
    """The fixture case again through the reference build, where there is one."""
    if not po.ref_available():
        pytest.skip("no reference build here")
    key, name, motion, S, J, seed, K, Mf, E, Af, Rf, Ff, moves, lights = _fixture_case()
    scene, depth = sc.scene_of(name)
    cam = scenes.make_camera(cc.FIX_W, cc.FIX_H, 500.0 / cc.FIX_W)
    none = np.zeros((cc.FIX_H, cc.FIX_W, 2), np.uint32)
    cache = {}

    def frame_of(p):
        if p not in cache:
            cache[p] = hc.render_ref(scene, cam, hc.MOTIONS[motion], cc.FIX_W, cc.FIX_H, depth, S, J, ac.seed_of(seed, p),
                                     Af, Rf, Ff, mc.displacement(scene, moves), lights)
        return cache[p], none

    r = cc.converge(frame_of, cc.zero_state(cc.FIX_H, cc.FIX_W), K, Mf, E)
    fx = cc.fixtures()
    sc.assert_same_bits(r["acc"], fx[key + "_acc"], key)
    sc.assert_same_bits(r["sq"], fx[key + "_sq"], key)
    assert np.array_equal(r["n"], fx[key + "_count"])


# ---- the CLI ------------------------------------------------------------------------------------------------------------
def test_cli_usage_errors(tmp_path):
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    base = ["--samples", "2", "--jitter", "4"]
    for args, flag, word in ((base + ["--tolerance", "0.01"], "--tolerance", "--passes"),
                             (base + ["--passes", "8", "--tolerance", "-1"], "--tolerance", ">= 0"),
                             (base + ["--passes", "8", "--min-passes", "3"], "--min-passes", "--tolerance"),
                             (base + ["--passes", "8", "--tolerance", "0.01", "--min-passes", "1"], "--min-passes", "2 .."),
                             (base + ["--passes", "8", "--tolerance", "0.01", "--min-passes", "2147483649"],
                              "--min-passes", "2 ..")):
        r = subprocess.run([exe, "--config", "c2", "--out", str(tmp_path / "x.ppm")] + args, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert flag in r.stderr and word in r.stderr, (args, r.stderr)
        assert not (tmp_path / "x.ppm").exists()
