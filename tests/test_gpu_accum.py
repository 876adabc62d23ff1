"""GPU: progressive accumulation (rt_render_accum_dev / rt_render_accum, Tracer.render_accum, the CLI) against the
contract of include/rt_api.h restated with numpy on frames of the CPU oracle (tests/accum_common.py over
tests/shutter_common.py) and against the fixtures made from the reference build (tests/golden/accum.npz, shutter.npz,
jitter.npz, motion.npz, soft.npz, dof.npz, ssaa.npz).  Expected values never come from the code under test.

Float images and the accumulator are compared bit for bit (NaNs by position: their sign and payload are unspecified);
byte images and ray counters exactly.  Frames are 19 x 11 at pitch 500 / 19 unless said: at S = 2 a 38 x 22 sample frame
with partial 8 x 8 tiles in both axes.  tests/test_accum_oracle.py shows on the oracle that the cases are
discriminating: consecutive seeds give other frames, and another sum order, a local partial sum or a reciprocal give
other bits.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402

from . import accum_common as ac  # noqa: E402
from . import dof_common as dc  # noqa: E402
from . import jitter_common as jc  # noqa: E402
from . import lens_gpu_common as lg  # noqa: E402
from . import motion_common as mc  # noqa: E402
from . import shutter_common as hc  # noqa: E402
from . import soft_common as so  # noqa: E402
from . import ssaa_common as sc  # noqa: E402
from .lens_gpu_common import BAD, OUTS, _check_all, _host, fresh, tr  # noqa: E402,F401
from .test_jitter_oracle import SHAPES  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 19, 11
A, R, F = 8.0, 40.0, 1.0
MOVES = mc.MOVES
ALL = dict(rgba32f=True, rgba8=True, rgb64f=True, raycount=True)


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    for name in ("rt_render_accum_dev", "rt_render_accum"):
        assert name in abi.SIGNATURES and hasattr(abi.lib(), name), name


def _dev(t, a):
    return torch.from_numpy(np.array(a, copy=True)).to(torch.device("cuda", t.device))     # (a may be read-only)


def _accum(t, w, h, fill=None, start=None):
    """An accumulator of the context's device: uninitialised, filled with a value, or a copy of a host array."""
    acc = t.alloc_accum(w, h)
    if start is not None:
        acc.copy_(_dev(t, start))
    elif fill is not None:
        acc.fill_(fill)
    return acc


def _render(t, cam, motion, w, h, depth, S, J, seed, n0, K, aperture, light_size, shutter, acc):
    """-> (every output on the host, the accumulator on the host)."""
    m = None if motion is None else hc.motion_abi(motion)
    bufs, acc = t.render_accum(cam, m, w, h, depth, S, J, seed, n0, K, aperture, light_size, shutter, accum=acc, **ALL)
    got = _host(bufs)
    return got, acc.cpu().numpy()


def _check(got, acc, e, what):
    sc.assert_same_bits(acc, e["acc"], what + " accum")
    _check_all(got, e["mean"], e["rc2"], what)


def _set(t, name, e):
    scene, depth = sc.scene_of(name)
    t.set_scene(scene)
    t.set_motion(e["d"])
    return depth


def _expected_run(t, name, motion, w, h, S, J, seed, n0, K, aperture, light_size, shutter, what, moves=None,
                  pitch_w=None):
    """accum_common.expected of a canonical scene (with its MOVES unless given) and the GPU call, compared; a call with
    n0 > 0 starts from the oracle's accumulator after n0 passes, one with n0 = 0 from a NaN-filled buffer."""
    e = ac.expected(name, motion, w, h, S, J, seed, n0, K, aperture, light_size, shutter,
                    MOVES[name] if moves is None else moves, pitch_w=pitch_w)
    depth = _set(t, name, e)
    acc = _accum(t, w, h, fill=float("nan")) if n0 == 0 else _accum(t, w, h, start=e["acc0"])
    got, acc = _render(t, e["cam"], e["motion"], w, h, depth, S, J, seed, n0, K, aperture, light_size, shutter, acc)
    _check(got, acc, e, what)
    return e, got, acc


# 1. every instance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,J,w,h", SHAPES)
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_variants(tr, name, S, J, w, h):
    """c2 depth 1 and c5 depth 3: the opaque instance; demo depth 5: the FULL one; tree_demo depth 5: the ray-tree
    one.  Three passes of a crane with lens, panel and moving spheres together."""
    _expected_run(tr, name, "crane", w, h, S, J, 1, 0, 3, A, R, F, f"{name} S={S} J={J}")


# 2. one pass from pass 0 is the shutter render ---------------------------------------------------------------------
def _pin(t, cam, m, w, h, depth, S, J, seed, Af, Rf, Ff, want, what):
    """n0 = 0, K = 1 from a NaN-filled accumulator against Tracer.render_shutter, output by output, and against the
    fixture `want` (when given)."""
    sh = _host(t.render_shutter(cam, m, w, h, depth, S, J, seed, Af, Rf, Ff, **ALL))
    bufs, acc = t.render_accum(cam, m, w, h, depth, S, J, seed, 0, 1, Af, Rf, Ff, accum=_accum(t, w, h, float("nan")),
                               **ALL)
    got, acc = _host(bufs), acc.cpu().numpy()
    for k in ("rgba32f", "rgb64f"):
        sc.assert_same_bits(got[k], sh[k], f"{what} {k}")
    assert got["rgba8"].tobytes() == sh["rgba8"].tobytes() and np.array_equal(got["raycount"], sh["raycount"]), what
    sc.assert_same_bits(acc, sh["rgb64f"], what + " accum")
    if want is not None:
        sc.assert_same_bits(got["rgb64f"], want, what + " fixture")


@pytest.mark.parametrize("key,name,S,J,seed,Ff,Af,Rf,lights,moves,motion", hc.FIXTURES)
def test_one_pass_is_the_shutter_fixture(tr, key, name, S, J, seed, Ff, Af, Rf, lights, moves, motion):
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene if lights is None else so.scene_abi(scene, lights))
    tr.set_motion(mc.displacement(scene, moves))
    cam = scenes.make_camera(hc.FIX_W, hc.FIX_H, 500.0 / hc.FIX_W)
    _pin(tr, cam, hc.motion_abi(hc.MOTIONS[motion]), hc.FIX_W, hc.FIX_H, depth, S, J, seed, Af, Rf, Ff,
         hc.fixtures()[key], key)


def test_one_pass_down_the_chain_of_fixtures(tr):
    """One fixture each of the jittered, motion, soft, lens and supersampled renders, with a frozen camera."""
    cam = scenes.make_camera(sc.FIX_W, sc.FIX_H, 500.0 / sc.FIX_W)

    def run(scene_abi_or_scene, scene, moves, depth, S, J, seed, Af, Rf, Ff, want, what):
        tr.set_scene(scene_abi_or_scene)
        tr.set_motion(None if moves is None else mc.displacement(scene, moves))
        _pin(tr, cam, None, sc.FIX_W, sc.FIX_H, depth, S, J, seed, Af, Rf, Ff, want, what)

    key, name, S, J, seed, Ff, Af, Rf, lights, moves = jc.FIXTURES[1]
    scene, depth = sc.scene_of(name)
    run(so.scene_abi(scene, lights), scene, moves, depth, S, J, seed, Af, Rf, Ff, jc.fixtures()[key], "jitter " + key)
    key, name, S, Ff, Af, Rf, lights, moves = mc.FIXTURES[2]
    scene, depth = sc.scene_of(name)
    run(so.scene_abi(scene, lights), scene, moves, depth, S, 1, 77, Af, Rf, Ff, mc.fixtures()[key], "motion " + key)
    name, S, Rf, Af, centres = so.FIXTURES[0]
    scene, depth = sc.scene_of(name)
    run(so.scene_abi(scene, centres), scene, MOVES[name], depth, S, 1, 77, Af, Rf, 0.0,
        so.fixtures()[so.fixture_key(name, S)], f"soft {name} S={S}")
    name, S = dc.FIXTURES[0]
    scene, depth = sc.scene_of(name)
    run(scene, scene, MOVES[name], depth, S, 1, 77, dc.FIX_A, 0.0, 0.0, dc.fixtures()[sc.fixture_key(name, S)],
        f"dof {name} S={S}")
    name, S = sc.FIXTURES[0]
    scene, depth = sc.scene_of(name)
    run(scene, scene, None, depth, S, 1, 77, 0.0, 0.0, 1.0, sc.fixtures()[sc.fixture_key(name, S)], f"ssaa {name} S={S}")


@pytest.mark.parametrize("name", ["c2", "demo"])
def test_one_pass_one_sample_one_sub_position_is_the_plain_render(tr, name):
    """S = J = 1, n0 = 0, K = 1: sigma = 0 and the mean is the value itself: the plain frame."""
    def render(cam, depth):
        got, _ = _render(tr, cam, hc.MOTIONS["crane"], lg.W, lg.H, depth, 1, 1, 77, 0, 1, A, R, F,
                         _accum(tr, lg.W, lg.H, float("nan")))
        return got
    lg.check_one_sample_is_the_plain_render(tr, name, render, lambda scene: tr.set_motion(mc.displacement(scene, MOVES[name])))


@pytest.mark.parametrize("key,base,seed,K", ac.FIXTURES)
def test_accum_fixtures(tr, key, base, seed, K):
    name, S, J, Ff, Af, Rf, lights, moves, motion = ac.shutter_fixture(base)
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene if lights is None else so.scene_abi(scene, lights))
    tr.set_motion(mc.displacement(scene, moves))
    cam = scenes.make_camera(ac.FIX_W, ac.FIX_H, 500.0 / ac.FIX_W)
    got, acc = _render(tr, cam, hc.MOTIONS[motion], ac.FIX_W, ac.FIX_H, depth, S, J, seed, 0, K, Af, Rf, Ff,
                       _accum(tr, ac.FIX_W, ac.FIX_H, float("nan")))
    sc.assert_same_bits(acc, ac.fixtures()[key + "_acc"], key + " acc")
    sc.assert_same_bits(got["rgb64f"], ac.fixtures()[key + "_mean"], key + " mean")


# 3. a sum continued call after call ----------------------------------------------------------------------------------
def test_split_calls_leave_the_bytes_of_one_call(tr):
    """(0, 5) against (0, 2) + (2, 3) and against five calls of one pass, the accumulator handed on by the code under
    test; every variant against the oracle, and the calls' counters summed against the one call's."""
    S, J, seed = 2, 4, 1
    e = ac.expected("c2", "crane", W, H, S, J, seed, 0, 5, A, R, F, MOVES["c2"])
    depth = _set(tr, "c2", e)
    args = (e["cam"], e["motion"], W, H, depth, S, J, seed)
    one, one_acc = _render(tr, *args, 0, 5, A, R, F, _accum(tr, W, H, float("nan")))
    _check(one, one_acc, e, "(0, 5)")
    for plan in ((2, 3), (1, 1, 1, 1, 1)):
        acc_t = _accum(tr, W, H, float("nan"))
        n0, counts = 0, np.zeros_like(e["rc2"])
        for K in plan:
            m = hc.motion_abi(e["motion"])
            bufs, acc_t = tr.render_accum(e["cam"], m, W, H, depth, S, J, seed, n0, K, A, R, F, accum=acc_t, **ALL)
            got = _host(bufs)
            part = ac.expected("c2", "crane", W, H, S, J, seed, n0, K, A, R, F, MOVES["c2"])
            _check(got, acc_t.cpu().numpy(), part, f"{plan} at {n0}")
            counts = counts + got["raycount"]
            n0 += K
        assert acc_t.cpu().numpy().tobytes() == one_acc.tobytes(), plan
        for k in ("rgba32f", "rgba8", "rgb64f"):
            assert got[k].tobytes() == one[k].tobytes(), (plan, k)
        assert np.array_equal(counts, one["raycount"]), plan


# 4. the launch split ---------------------------------------------------------------------------------------------------
def test_launch_split_is_invisible(tr, monkeypatch):
    """A context created under RT_ACCUM_MAX_PASSES=2 runs K = 5 as launches of 2, 2 and 1 passes, the accumulator and
    the counters reloaded in between: the bytes of the default context's one call, and the oracle's."""
    S, J, seed = 2, 4, 1
    e = ac.expected("c2", "crane", W, H, S, J, seed, 0, 5, A, R, F, MOVES["c2"])
    depth = _set(tr, "c2", e)
    args = (e["cam"], e["motion"], W, H, depth, S, J, seed, 0, 5, A, R, F)
    want, want_acc = _render(tr, *args, _accum(tr, W, H, float("nan")))
    _check(want, want_acc, e, "default context")
    monkeypatch.setenv("RT_ACCUM_MAX_PASSES", "2")
    t2 = Tracer(0)
    try:
        _set(t2, "c2", e)
        got, acc = _render(t2, *args, _accum(t2, W, H, float("nan")))
        _check(got, acc, e, "RT_ACCUM_MAX_PASSES=2")
        assert acc.tobytes() == want_acc.tobytes()
        for k in OUTS:
            assert got[k].tobytes() == want[k].tobytes(), k
        e2 = ac.expected("c2", "crane", W, H, S, J, seed, 2, 3, A, R, F, MOVES["c2"])     # a continued call, split 2 + 1
        got, acc = _render(t2, e["cam"], e["motion"], W, H, depth, S, J, seed, 2, 3, A, R, F,
                           _accum(t2, W, H, start=e2["acc0"]))
        _check(got, acc, e2, "RT_ACCUM_MAX_PASSES=2 from pass 2")
    finally:
        t2.close()


# 5. the seed wraps ---------------------------------------------------------------------------------------------------
def test_seed_wrap(tr):
    """Seed 0xFFFFFFFF, K = 3, S = 1, J = 16: the seeds 0xFFFFFFFF, 0, 1; the case whose mean a reciprocal misses."""
    _expected_run(tr, "c2", "crane", W, H, 1, 16, 0xFFFFFFFF, 0, 3, A, R, F, "seed wrap")


@pytest.mark.parametrize("n0,K", [(0, 7), (3, 4)])
def test_seven_passes(tr, n0, K):
    """K = 7 at once (two launches at the default split) and as passes 3 .. 6 of a continued sum."""
    _expected_run(tr, "c2", "crane", W, H, 1, 16, 0xFFFFFFFF, n0, K, A, R, F, f"({n0}, {K})")


# 6. the smallest shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (9, 1), (1, 9), (8, 8), (9, 9)])
def test_small_frames(tr, w, h, S):
    """c2 on a w x h frame at pitch 500 / 37 (the camera of that size, not a crop), two passes."""
    _expected_run(tr, "c2", "crane", w, h, S, 4, 1, 0, 2, A, R, F, f"{w}x{h} S={S}", pitch_w=37)


@pytest.mark.parametrize("S,w", [(2, 13), (4, 7), (1, 21)])
def test_odd_widths(tr, S, w):
    """A width that is no multiple of 8 / S at J = 16: the key comes from the true sample-frame width, in every pass."""
    assert (S * w) % 8 != 0
    _expected_run(tr, "c2", "crane", w, 5, S, 16, 9, 0, 2, A, R, F, f"odd width {w} S={S}", pitch_w=37)


# 7. a frozen camera, a frozen scene ----------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [None, hc.ZERO])
def test_frozen_camera_accumulates_jittered_frames(tr, motion):
    S, J, seed, K = 2, 4, 3, 3
    es = [jc.expected("c2", W, H, S, J, ac.seed_of(seed, p), A, R, F, MOVES["c2"]) for p in range(K)]
    e = ac.accumulate([x["rgb"] for x in es], [x["rc2"] for x in es], 0, K)
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    tr.set_motion(es[0]["d"])
    got, acc = _render(tr, es[0]["cam"], motion, W, H, depth, S, J, seed, 0, K, A, R, F, _accum(tr, W, H, float("nan")))
    _check(got, acc, e, "frozen camera")


def test_equal_passes_sum_to_the_repeated_addition(tr):
    """F = 0 and J = 1: every pass is the same frame v, so accum is ((v + v) + v) + v and the mean that over 4."""
    S, K = 2, 4
    v = hc.expected("c2", "crane", W, H, S, 1, 0, A, R, 0.0, MOVES["c2"])
    want = ((v["rgb"] + v["rgb"]) + v["rgb"]) + v["rgb"]
    depth = _set(tr, "c2", v)
    got, acc = _render(tr, v["cam"], v["motion"], W, H, depth, S, 1, 11, 0, K, A, R, 0.0, _accum(tr, W, H, float("nan")))
    sc.assert_same_bits(acc, want, "accum")
    _check_all(got, want / np.float64(K), v["rc2"] * np.uint32(K), "equal passes")


# 8. NaN frames -----------------------------------------------------------------------------------------------
def test_nan_passes(tr):
    S, J = 2, 4
    e = ac.expected("tree_c2", "crane", W, H, S, J, 1, 0, 3, 0.0, 0.0, F, MOVES["tree_c2"])
    nan_px = np.isnan(e["acc"]).any(axis=2)
    assert 0 < nan_px.sum() <= W * H / 3
    depth = _set(tr, "tree_c2", e)
    got, acc = _render(tr, e["cam"], e["motion"], W, H, depth, S, J, 1, 0, 3, 0.0, 0.0, F, _accum(tr, W, H, 0.0))
    assert np.array_equal(np.isnan(acc), np.isnan(e["acc"]))
    _check(got, acc, e, "tree_c2")
    assert (got["rgba8"][..., :3][np.isnan(e["mean"])] == 0).all()


# 9. each output alone, no output -----------------------------------------------------------------------------------
@pytest.mark.parametrize("only", OUTS + (None,))
def test_nullable_outputs(tr, only):
    """Each output alone, and none at all: the accumulator is written every time."""
    S, J, seed = 2, 4, 1
    e = ac.expected("c2", "crane", W, H, S, J, seed, 2, 3, A, R, F, MOVES["c2"])
    depth = _set(tr, "c2", e)
    flags = {k: k == only for k in OUTS}
    bufs, acc = tr.render_accum(e["cam"], hc.motion_abi(e["motion"]), W, H, depth, S, J, seed, 2, 3, A, R, F,
                                accum=_accum(tr, W, H, start=e["acc0"]), **flags)
    got = _host(bufs)
    sc.assert_same_bits(acc.cpu().numpy(), e["acc"], f"accum with {only}")
    assert list(got) == ([only] if only else [])
    if only:
        want = {"rgba32f": sc.to_rgba32f(e["mean"]), "rgba8": sc.to_rgba8(e["mean"]), "rgb64f": e["mean"],
                "raycount": e["rc2"]}[only]
        assert got[only].shape == want.shape and got[only].tobytes() == want.tobytes()


# 10. graph capture ---------------------------------------------------------------------------------------------------
def test_graph_capture(fresh):
    """A capture of a K = 3 call with n0 = 2, and three replays, each from a restored accumulator and zeroed images."""
    S, J, seed = 2, 4, 5
    e = ac.expected("c2", "crane", W, H, S, J, seed, 2, 3, 0.0, 0.0, F, MOVES["c2"])
    depth = _set(fresh, "c2", e)
    m = hc.motion_abi(e["motion"])
    start = _dev(fresh, e["acc0"])
    acc = fresh.alloc_accum(W, H)
    bufs = fresh.alloc_ss(W, H, None, **ALL)
    render_into = lambda s: fresh.render_accum_into(e["cam"], m, W, H, depth, S, J, seed, 2, 3, 0.0, 0.0, F, acc, bufs,  # noqa: E731
                                                    stream=s)
    s = torch.cuda.Stream()
    acc.copy_(start)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        render_into(s)                                                           # warm-up outside the capture
    s.synchronize()
    _check(_host(bufs), acc.cpu().numpy(), e, "direct")
    g = torch.cuda.CUDAGraph()
    acc.copy_(start)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        render_into(s)
    for k in range(3):
        for b in bufs.values():
            b.zero_()
        acc.copy_(start)
        torch.cuda.synchronize()
        g.replay()
        _check(_host(bufs), acc.cpu().numpy(), e, f"replay {k} of 3")


# 11. the context's other state ---------------------------------------------------------------------------------
def test_no_side_effect(fresh):
    """A view's first, calibration and cached renders, a soft-shadow frame, a motion frame and a jittered frame; then
    accumulating calls with other cameras, motions and splits; then the four again: the scene and motion records and the
    per-view state must still be what they were."""
    w, h = lg.W, lg.H
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    d = mc.displacement(scene, MOVES["c2"])
    fresh.set_motion(d)
    cam = scenes.make_camera(w, h, 500.0 / w)
    frames = lg.view_frames(fresh, scene, cam, depth)

    def others():
        return [_host(fresh.render_soft(cam, w, h, depth, 2, A, R, **ALL)),
                _host(fresh.render_motion(cam, w, h, depth, 2, 0.0, 0.0, F, **ALL)),
                _host(fresh.render_jitter(cam, w, h, depth, 2, 4, 1, 0.0, 0.0, F, **ALL))]

    before = others()
    sc.assert_same_bits(before[0]["rgb64f"], so.expected("c2", w, h, 2, A, R)["rgb"], "soft frame")
    m = mc.expected("c2", w, h, 2, 0.0, 0.0, F, MOVES["c2"])
    _check_all(before[1], m["rgb"], m["rc2"], "motion frame")
    j = jc.expected("c2", w, h, 2, 4, 1, 0.0, 0.0, F, MOVES["c2"])
    _check_all(before[2], j["rgb"], j["rc2"], "jittered frame")
    other = scenes.make_camera(W, H, 500.0 / W)
    other.eye[0] += 40.0
    other.eye[1] += 25.0
    acc = fresh.alloc_accum(W, H)
    for c, S, J, seed, motion, plan in ((other, 2, 4, 1, "crane", (3,)), (other, 4, 2, 2, "pan", (1, 5)),
                                        (scenes.make_camera(W, H, 500.0 / W), 2, 16, 3, "dolly", (2, 2))):
        n0 = 0
        for K in plan:
            fresh.render_accum(c, hc.motion_abi(hc.MOTIONS[motion]), W, H, depth, S, J, seed, n0, K, A, 0.0, F, accum=acc,
                               **ALL)
            n0 += K
    e = ac.expected("c2", "dolly", W, H, 2, 16, 3, 0, 4, A, 0.0, F, MOVES["c2"])      # the last sum is a checked one
    sc.assert_same_bits(acc.cpu().numpy(), e["acc"], "the last accumulator")
    lg.check_view_unchanged(frames, _host(fresh.render(cam, w, h, depth, **ALL)))
    for was, now in zip(before, others()):
        for key in OUTS:
            assert now[key].tobytes() == was[key].tobytes(), key


# 12. rt_render_accum: host buffers -----------------------------------------------------------------------------------
def test_render_accum_host_buffers(tr):
    """(0, 2) then (2, 3) through the host entry point, the accumulator a host array in and out."""
    S, J, seed = 2, 4, 6
    first = ac.expected("c2", "crane", lg.W, lg.H, S, J, seed, 0, 2, A, 0.0, F, MOVES["c2"])
    e = ac.expected("c2", "crane", lg.W, lg.H, S, J, seed, 2, 3, A, 0.0, F, MOVES["c2"])
    scene, depth = sc.scene_of("c2")
    s_abi = scene.to_abi()
    d = np.ascontiguousarray(e["d"])
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    m = hc.motion_abi(e["motion"])
    acc = np.full((lg.H, lg.W, 3), np.nan)
    pa = ctypes.c_void_p(acc.ctypes.data)
    f64 = np.zeros((lg.H, lg.W, 3), np.float64)
    abi.check(abi.lib().rt_render_accum(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(e["cam"]), ctypes.byref(m), lg.W,
                                        lg.H, depth, S, J, seed, 0, 2, A, 0.0, F, pa, None, None,
                                        ctypes.c_void_p(f64.ctypes.data), None), "rt_render_accum")
    sc.assert_same_bits(acc, first["acc"], "accum after (0, 2)")
    sc.assert_same_bits(f64, first["mean"], "mean after (0, 2)")
    f32, u8, st = np.zeros((lg.H, lg.W, 4), np.float32), np.zeros((lg.H, lg.W, 4), np.uint8), abi.rt_stats()
    abi.check(abi.lib().rt_render_accum(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(e["cam"]), ctypes.byref(m), lg.W,
                                        lg.H, depth, S, J, seed, 2, 3, A, 0.0, F, pa, ctypes.c_void_p(f32.ctypes.data),
                                        ctypes.c_void_p(u8.ctypes.data), ctypes.c_void_p(f64.ctypes.data),
                                        ctypes.byref(st)), "rt_render_accum")
    sc.assert_same_bits(acc, e["acc"], "accum after (2, 3)")
    sc.assert_same_bits(f64, e["mean"], "rgb64f")
    sc.assert_same_bits(f32, sc.to_rgba32f(e["mean"]), "rgba32f")
    assert np.array_equal(u8, sc.to_rgba8(e["mean"]))
    seg, sh = int(e["rc2"][..., 0].sum(dtype=np.uint64)), int(e["rc2"][..., 1].sum(dtype=np.uint64))
    prim = lg.W * lg.H * S * S * 3
    assert st.primary_rays == prim and st.reflect_rays == seg - prim and st.shadow_rays == sh
    # a null accumulator is rejected before anything is rendered
    rc = abi.lib().rt_render_accum(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(e["cam"]), ctypes.byref(m), lg.W, lg.H,
                                   depth, S, J, seed, 0, 2, A, 0.0, F, None, None, None, None, None)
    assert rc == abi.RT_EINVAL and "accum" in abi.last_error()


# 13. the CLI ---------------------------------------------------------------------------------------------------------
def test_cli(tmp_path):
    """_read_ppm reads lg.W x lg.H images."""
    motion = ((12.0, 30.0, -16.0), (50.0, 20.0, 0.0))
    e = ac.expected("c2", motion, lg.W, lg.H, 2, 4, 7, 0, 3, 8.0, 0.0, 0.5, MOVES["c2"])
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c2_accum.ppm"
    base = [exe, "--config", "c2", "--width", str(lg.W), "--height", str(lg.H), "--samples", "2", "--shutter", "0.5",
            "--move", "4:50,0,0", "--move", "0:0,12,-30", "--aperture", "8", "--eye-move", "12,30,-16", "--look-move",
            "50,20,0", "--jitter", "4", "--seed", "7", "--out", str(out)]
    r = subprocess.run(base + ["--passes", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if "accumulated" in ln]
    assert len(line) == 1 and "3 passes" in line[0] and f"{3 * lg.W * lg.H * 4} primary rays" in line[0], r.stdout
    assert np.array_equal(lg._read_ppm(out), sc.to_rgba8(e["mean"])[::-1, :, :3])  # PPM rows run top to bottom
    # without --passes: the one jittered frame, as before
    r = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "accumulated" not in r.stdout
    assert np.array_equal(lg._read_ppm(out), sc.to_rgba8(e["frames"][0])[::-1, :, :3])


# 14. argument errors -----------------------------------------------------------------------------------------
def test_argument_errors(tr):
    e = ac.expected("c2", "crane", W, H, 2, 4, 1, 0, 3, A, R, F, MOVES["c2"])
    depth = _set(tr, "c2", e)
    cam = scenes.make_camera(W, H, 500.0 / W)
    m = hc.motion_abi(e["motion"])
    bufs = tr.alloc_ss(W, H, None, **ALL)
    acc = tr.alloc_accum(W, H)
    acc.fill_(-7.0)
    bufs["rgba32f"].fill_(-7.0)
    bufs["rgb64f"].fill_(-7.0)
    bufs["rgba8"].fill_(249)                                 # -7 as a byte
    bufs["raycount"].fill_(-7)
    L = abi.lib()

    def call(cam=cam, motion=m, w=W, h=H, S=2, J=4, n0=0, K=3, ap=A, ls=R, sh=F, accum=acc):
        return L.rt_render_accum_dev(tr._ctx, ctypes.byref(cam), None if motion is None else ctypes.byref(motion), w, h,
                                     depth, S, J, 1, n0, K, ap, ls, sh,
                                     None if accum is None else ctypes.c_void_p(accum.data_ptr()),
                                     ctypes.c_void_p(bufs["rgba32f"].data_ptr()), ctypes.c_void_p(bufs["rgba8"].data_ptr()),
                                     ctypes.c_void_p(bufs["rgb64f"].data_ptr()),
                                     ctypes.c_void_p(bufs["raycount"].data_ptr()), lg.stream_ptr())

    # the call's own checks
    assert call(accum=None) == abi.RT_EINVAL and "accum" in abi.last_error()
    for K in (0, -1, 65537):
        assert call(K=K) == abi.RT_EINVAL and "passes" in abi.last_error(), K
    for n0, K in ((2 ** 31, 1), (2 ** 31 - 2, 3), (2 ** 32 - 1, 1), (2 ** 31 - 65535, 65536)):
        assert call(n0=n0, K=K) == abi.RT_EINVAL and "first_pass" in abi.last_error(), (n0, K)
    # one check from each family of the shutter render
    bad = hc.motion_abi(e["motion"])
    bad.eye[0] = float("nan")
    assert call(motion=bad) == abi.RT_EINVAL and "displacement" in abi.last_error()
    down = scenes.make_camera(W, H, 500.0 / W)             # looking straight down: parallel to up at sigma = 0
    down.look_at[0], down.look_at[1], down.look_at[2] = down.eye[0], down.eye[1] - 100.0, down.eye[2]
    assert call(cam=down) == abi.RT_EINVAL and "parallel to up" in abi.last_error()
    assert call(J=3) == abi.RT_EINVAL and "jitter" in abi.last_error()
    assert call(w=2 ** 24, h=1, S=8, J=16) == abi.RT_EINVAL and "overflow" in abi.last_error()
    assert call(S=3) == abi.RT_EINVAL and "samples" in abi.last_error()
    assert call(ap=BAD[0]) == abi.RT_EINVAL and "aperture" in abi.last_error()
    assert call(ls=BAD[2]) == abi.RT_EINVAL and "light_size" in abi.last_error()
    assert call(sh=2.0) == abi.RT_EINVAL and "shutter" in abi.last_error()
    assert call(w=0) == abi.RT_EINVAL and "size" in abi.last_error()
    with pytest.raises(abi.RtError) as ei:
        tr.render_accum_into(cam, m, W, H, depth, 2, 4, 1, 0, 0, A, R, F, acc, bufs)
    assert ei.value.code == abi.RT_EINVAL and "passes" in str(ei.value)
    torch.cuda.synchronize()
    assert (acc == -7.0).all(), "a rejected call wrote the accumulator"
    assert (bufs["rgba32f"] == -7.0).all() and (bufs["rgb64f"] == -7.0).all() and (bufs["rgba8"] == 249).all()
    assert (bufs["raycount"] == -7).all(), "a rejected call wrote pixels"
    assert call() == abi.RT_OK                               # the same buffers, good arguments
    _check(_host(bufs), acc.cpu().numpy(), e, "after the errors")
    assert call(n0=2 ** 31 - 1, K=1) == abi.RT_OK            # the last pass there is: first_pass + passes = 2^31
    torch.cuda.synchronize()
