"""GPU: adaptive sampling of the lens, soft-shadow and motion-blur renders (rt_render_lens_adaptive_dev /
rt_render_lens_adaptive, Tracer.render_lens_adaptive, the CLI) against the contract of include/rt_api.h evaluated on
rays traced by the CPU oracle (tests/lens_adaptive_common.py) and against the fixtures made from the reference build
(tests/golden/lens_adaptive.npz, motion.npz, soft.npz, dof.npz, ssaa.npz, adaptive.npz).  Expected values never come
from the code under test.

Float images are compared bit for bit (NaNs by position: their sign and payload are unspecified); byte images, ray
counters and the refined mask exactly.  Frames are 37 x 21 at pitch 500 / 37 unless said: partial 8 x 8 sample tiles in
both axes.  tests/test_lens_adaptive_oracle.py shows on the oracle that each case is discriminating: both criteria
flag pixels the other does not, and the wrong level on either side of the mask changes pixels.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402

from . import adaptive_common as ac  # noqa: E402
from . import dof_common as dc  # noqa: E402
from . import lens_adaptive_common as la  # noqa: E402
from . import lens_gpu_common as lg  # noqa: E402
from . import motion_common as mc  # noqa: E402
from . import soft_common as so  # noqa: E402
from . import ssaa_common as sc  # noqa: E402
from .lens_gpu_common import BAD, H, OUTS, W, _check_all, _host, _read_ppm, fresh, tr  # noqa: E402,F401

pytestmark = pytest.mark.gpu

A, R, F, T = 8.0, 40.0, 0.75, 32
MOVES = mc.MOVES


def _render(t, cam, w, h, depth, S_lo, S_hi, thr, aperture=A, light_size=R, shutter=F):
    return _host(t.render_lens_adaptive(cam, w, h, depth, S_lo, S_hi, thr, aperture, light_size, shutter, rgba32f=True,
                                        rgba8=True, rgb64f=True, raycount=True))


def _check_expected(got, e, what):
    """Every output and the mask against lens_adaptive_common's dict."""
    assert got["refined"].dtype == np.uint8 and np.array_equal(got["refined"], e["mask"].astype(np.uint8)), what + " mask"
    _check_all(got, e["rgb"], e["rc2"], what)


def _set(t, name, e):
    scene, depth = sc.scene_of(name)
    t.set_scene(scene)
    t.set_motion(e["d"])
    return depth


# 1. every instance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(2, 4), (1, 4)])
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_variants(tr, name, pair):
    """c2 depth 1 and c5 depth 3: the opaque instances; demo depth 5: the FULL ones; tree_demo depth 5: the ray-tree
    ones.  Lens, panel and motion together."""
    e = la.expected(name, W, H, pair[0], pair[1], T, A, R, F, MOVES[name])
    share, a_only, b_only, unref_diff, ref_diff = la.census(e)
    if pair == (2, 4):
        assert 0.3 <= share <= 0.8 and a_only >= 5 and b_only >= 50 and unref_diff >= 5 and ref_diff >= 200
    else:
        assert 0.35 <= round(share, 2) <= 0.62 and unref_diff >= 47
    depth = _set(tr, name, e)
    _check_expected(_render(tr, e["cam"], W, H, depth, pair[0], pair[1], T), e, f"{name} {pair}")


@pytest.mark.parametrize("pair", [(2, 8), (4, 8)])
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_eight_samples(tr, name, pair):
    e = la.expected(name, W, H, pair[0], pair[1], T, A, R, F, MOVES[name])
    assert 0.05 < e["mask"].mean() < 0.95
    depth = _set(tr, name, e)
    _check_expected(_render(tr, e["cam"], W, H, depth, pair[0], pair[1], T), e, f"{name} {pair}")


# 2. several compaction workgroups and a real spread criterion --------------------------------------------------
def test_several_classification_workgroups(tr):
    """131 x 100 = 13100 pixels: two 8192-pixel workgroups fill the list, the second partly empty."""
    w, h = 131, 100
    e = la.expected("c2", w, h, 2, 4, 8, A, R, F, MOVES["c2"])
    share, a_only, b_only, _, _ = la.census(e)
    assert a_only >= 100 and b_only >= 300 and 0.15 < share < 0.5
    flat = e["mask"].reshape(-1)
    assert flat[:8192].any() and flat[8192:].any()
    depth = _set(tr, "c2", e)
    _check_expected(_render(tr, e["cam"], w, h, depth, 2, 4, 8), e, f"{w}x{h}")


# 3. a list longer than the refine grid ---------------------------------------------------------------------------
def test_grid_stride_refine(tr):
    """13100 listed pixels at S_hi = 8, one per wave: more than the refine launch's 8192 workgroups."""
    w, h = 131, 100
    e = la.expected("c2", w, h, 2, 8, -1, A, R, F, MOVES["c2"])
    assert e["mask"].all() and w * h > 8192
    sc.assert_same_bits(e["rgb"], mc.expected("c2", w, h, 8, A, R, F, MOVES["c2"])["rgb"], "T = -1 is the S = 8 frame")
    depth = _set(tr, "c2", e)
    _check_expected(_render(tr, e["cam"], w, h, depth, 2, 8, -1), e, f"{w}x{h} (2, 8) T=-1")


# 4. the fixtures from the reference build through the new kernels ------------------------------------------------
def _fixture_run(t, want, w, h, depth, S, aperture, light_size, shutter, what, rc2=None):
    """T = -1 with S_hi = S from both smaller coarse counts: the refine kernel; T = 255 with S_lo = S: the coarse one."""
    cam = scenes.make_camera(w, h, 500.0 / w)
    for S_lo, S_hi, thr in [(1, S, -1), (2, S, -1), (S, S, 255)] + ([(S, 8, 255)] if S < 8 else []):
        got = _host(t.render_lens_adaptive(cam, w, h, depth, S_lo, S_hi, thr, aperture, light_size, shutter,
                                           rgba32f=False, rgb64f=True, raycount=True))
        assert (got["refined"] == (1 if thr == -1 else 0)).all()
        sc.assert_same_bits(got["rgb64f"], want, f"{what} ({S_lo}, {S_hi}) T={thr}")
        if rc2 is not None:
            assert np.array_equal(got["raycount"], rc2), f"{what} ({S_lo}, {S_hi}) T={thr} raycount"


@pytest.mark.parametrize("key,name,S,Ff,Af,Rf,lights,moves", mc.FIXTURES)
def test_motion_fixtures(tr, key, name, S, Ff, Af, Rf, lights, moves):
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene if lights is None else so.scene_abi(scene, lights))
    tr.set_motion(mc.displacement(scene, moves))
    _fixture_run(tr, mc.fixtures()[key], mc.FIX_W, mc.FIX_H, depth, S, Af, Rf, Ff, key)


@pytest.mark.parametrize("name,S,Rf,Af,centres", so.FIXTURES)
def test_soft_fixtures(tr, name, S, Rf, Af, centres):
    scene, depth = sc.scene_of(name)
    tr.set_scene(so.scene_abi(scene, centres))
    tr.set_motion(mc.displacement(scene, MOVES[name]))                       # F = 0: the motion in force is not seen
    _fixture_run(tr, so.fixtures()[so.fixture_key(name, S)], so.FIX_W, so.FIX_H, depth, S, Af, Rf, 0.0,
                 f"soft {name} S={S}", so.expected(name, so.FIX_W, so.FIX_H, S, Af, Rf, centres)["rc2"])


@pytest.mark.parametrize("name,S", dc.FIXTURES)
def test_dof_fixtures(tr, name, S):
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    tr.set_motion(None)
    _fixture_run(tr, dc.fixtures()[sc.fixture_key(name, S)], dc.FIX_W, dc.FIX_H, depth, S, dc.FIX_A, 0.0, 1.0,
                 f"dof {name} S={S}", dc.expected(name, dc.FIX_W, dc.FIX_H, S, dc.FIX_A)["rc2"])


@pytest.mark.parametrize("name,S", sc.FIXTURES)
def test_ssaa_fixtures(tr, name, S):
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    tr.set_motion(None)
    _fixture_run(tr, sc.fixtures()[sc.fixture_key(name, S)], sc.FIX_W, sc.FIX_H, depth, S, 0.0, 0.0, 0.0,
                 f"ssaa {name} S={S}", sc.expected(name, sc.FIX_W, sc.FIX_H, S)["rc2"])


@pytest.mark.parametrize("name,S", ac.FIXTURES)
def test_adaptive_fixtures(tr, name, S):
    """A = R = F = 0, S_lo = 1: rt_render_adaptive_dev's frame and mask."""
    fx = ac.fixtures()
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    tr.set_motion(None)
    cam = scenes.make_camera(ac.FIX_W, ac.FIX_H, 500.0 / ac.FIX_W)
    got = _render(tr, cam, ac.FIX_W, ac.FIX_H, depth, 1, S, ac.FIX_T, 0.0, 0.0, 0.0)
    assert np.array_equal(got["refined"], fx[sc.fixture_key(name, S) + "_mask"])
    sc.assert_same_bits(got["rgb64f"], fx[sc.fixture_key(name, S)], f"{name} S={S}")
    want = ac.expected(name, ac.FIX_W, ac.FIX_H, S, ac.FIX_T)
    assert np.array_equal(got["raycount"], want["rc2"])
    plain = _host(tr.render_adaptive(cam, ac.FIX_W, ac.FIX_H, depth, S, ac.FIX_T, rgba32f=True, rgba8=True, rgb64f=True,
                                     raycount=True))
    for k in OUTS + ("refined",):
        assert got[k].tobytes() == plain[k].tobytes(), k


@pytest.mark.parametrize("case", [mc.shadow_only_case, mc.reflection_only_case, mc.fast_small_case])
def test_discriminating_frames(tr, case):
    """The frames a kernel that moves only some uses of the sphere centre cannot pass, through the refine kernel."""
    scene, depth, S, shutter, moves = case()
    cam = scenes.make_camera(W, H, 500.0 / W)
    d = mc.displacement(scene, moves)
    e = la.render(scene, cam, W, H, depth, 1, S, -1, 0.0, 0.0, shutter, d)
    tr.set_scene(scene)
    tr.set_motion(d)
    _check_expected(_render(tr, cam, W, H, depth, 1, S, -1, 0.0, 0.0, shutter), e, case.__name__)


# 5. the new fixtures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,S_lo,S_hi,Ff,Af,Rf,lights,moves", la.FIXTURES)
def test_lens_adaptive_fixtures(tr, key, name, S_lo, S_hi, Ff, Af, Rf, lights, moves):
    fx = la.fixtures()
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene if lights is None else so.scene_abi(scene, lights))
    tr.set_motion(mc.displacement(scene, moves))
    cam = scenes.make_camera(la.FIX_W, la.FIX_H, 500.0 / la.FIX_W)
    got = _host(tr.render_lens_adaptive(cam, la.FIX_W, la.FIX_H, depth, S_lo, S_hi, la.FIX_T, Af, Rf, Ff, rgba32f=False,
                                        rgb64f=True))
    assert np.array_equal(got["refined"], fx[key + "_mask"])
    sc.assert_same_bits(got["rgb64f"], fx[key], key)


# 6. NaN frames -----------------------------------------------------------------------------------------------
def test_nan_frames(tr):
    e = la.expected("tree_c2", W, H, 2, 4, T, 0.0, 0.0, 1.0, MOVES["tree_c2"])
    nan_px = np.isnan(e["rgb"]).any(axis=2)
    assert 0 < nan_px.sum() <= 0.25 * W * H and 0 < e["mask"].sum() < W * H
    depth = _set(tr, "tree_c2", e)
    assert depth == 3
    got = _render(tr, e["cam"], W, H, depth, 2, 4, T, 0.0, 0.0, 1.0)
    assert np.array_equal(np.isnan(got["rgb64f"]), np.isnan(e["rgb"]))
    _check_expected(got, e, "tree_c2 (2, 4)")
    assert (got["rgba8"][..., :3][np.isnan(e["rgb"])] == 0).all()


# 7. the smallest shapes: neighbour indexing at the frame's edges, lists shorter than a wave --------------------
@pytest.mark.parametrize("thr", [0, -1])
@pytest.mark.parametrize("pair", [(2, 4), (1, 8)])
@pytest.mark.parametrize("w,h", [(1, 1), (9, 1), (1, 9), (8, 8), (9, 9)])
def test_small_frames(tr, w, h, pair, thr):
    """c2 on a w x h frame at pitch 500 / 37 (the camera of that size, not a crop)."""
    scene, depth = sc.scene_of("c2")
    cam = scenes.make_camera(w, h, 500.0 / 37)
    d = mc.displacement(scene, MOVES["c2"])
    e = la.render(scene, cam, w, h, depth, pair[0], pair[1], thr, A, R, F, d)
    if thr == -1:
        assert e["mask"].all(), "T = -1 refines every pixel, a 1 x 1 frame included"
    tr.set_scene(scene)
    tr.set_motion(d)
    _check_expected(_render(tr, cam, w, h, depth, pair[0], pair[1], thr), e, f"{w}x{h} {pair} T={thr}")


# 8. one context, one workspace, thresholds in turn -------------------------------------------------------------
def test_one_workspace_many_thresholds(fresh):
    """A stale counter or list, and coarse bytes overwritten by the previous refine pass (the byte image is the
    criterion's input and the refine pass's output)."""
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    fresh.set_motion(mc.displacement(scene, MOVES["c2"]))
    bufs = fresh.alloc_lens_adaptive(W, H, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    for k, thr in enumerate([-1, 32, 255, 32, -1, 32, 32]):
        e = la.expected("c2", W, H, 2, 4, thr, A, R, F, MOVES["c2"])
        fresh.render_lens_adaptive_into(e["cam"], W, H, depth, 2, 4, thr, A, R, F, bufs)
        got = _host(bufs)
        _check_expected(got, e, f"render {k} T={thr}")
        assert int(got["workspace"][:4].view(np.uint32)[0]) == int(e["mask"].sum())


def test_workspace_coarse_bytes(fresh):
    """Without an rgba8 output the coarse bytes live in the workspace; its first word counts the refined pixels."""
    e = la.expected("c2", W, H, 2, 4, T, A, R, F, MOVES["c2"])
    depth = _set(fresh, "c2", e)
    bufs = fresh.alloc_lens_adaptive(W, H, rgba32f=False, rgba8=False, rgb64f=True, raycount=False)
    for k in range(3):
        fresh.render_lens_adaptive_into(e["cam"], W, H, depth, 2, 4, T, A, R, F, bufs)
        got = _host(bufs)
        assert np.array_equal(got["refined"], e["mask"].astype(np.uint8))
        sc.assert_same_bits(got["rgb64f"], e["rgb"], f"render {k}")
        assert int(got["workspace"][:4].view(np.uint32)[0]) == int(e["mask"].sum())


# 9. hipGraph capture -----------------------------------------------------------------------------------------
def test_graph_capture(fresh):
    e = la.expected("c2", W, H, 2, 4, T, A, R, F, MOVES["c2"])
    depth = _set(fresh, "c2", e)
    bufs = fresh.alloc_lens_adaptive(W, H, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fresh.render_lens_adaptive_into(e["cam"], W, H, depth, 2, 4, T, A, R, F, bufs, stream=s)   # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fresh.render_lens_adaptive_into(e["cam"], W, H, depth, 2, 4, T, A, R, F, bufs, stream=s)
    for k in range(3):
        for b in bufs.values():
            if b is not None:
                b.zero_()
        g.replay()
        _check_expected(_host(bufs), e, f"replay {k}")


# 10. the context's other state -----------------------------------------------------------------------------------
def test_no_side_effect(fresh):
    """A view's first, calibration and cached renders and a motion frame; adaptive lens frames of another eye and of
    this one; then the view and the motion frame again."""
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    d = mc.displacement(scene, MOVES["c2"])
    fresh.set_motion(d)
    cam = scenes.make_camera(W, H, 500.0 / W)
    frames = lg.view_frames(fresh, scene, cam, depth)
    motion = _host(fresh.render_motion(cam, W, H, depth, 2, A, R, F, rgba32f=True, rgba8=True, rgb64f=True,
                                       raycount=True))
    sc.assert_same_bits(motion["rgb64f"], mc.expected("c2", W, H, 2, A, R, F, MOVES["c2"])["rgb"], "motion frame")
    other = scenes.make_camera(W, H, 500.0 / W)
    other.eye[0] += 40.0
    other.eye[1] += 25.0
    for c, pair in ((other, (2, 4)), (cam, (1, 4)), (cam, (2, 4))):
        e = la.render(scene, c, W, H, depth, pair[0], pair[1], T, A, R, F, d)
        _check_expected(_render(fresh, c, W, H, depth, pair[0], pair[1], T), e, f"{pair}")
    lg.check_view_unchanged(frames, _host(fresh.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True,
                                                       raycount=True)))
    again = _host(fresh.render_motion(cam, W, H, depth, 2, A, R, F, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
    for key in OUTS:
        assert again[key].tobytes() == motion[key].tobytes(), key


# 11. rt_render_lens_adaptive: host buffers, stats and the CLI ----------------------------------------------------
def test_render_lens_adaptive_host_buffers(tr):
    S_lo, S_hi = 2, 4
    e = la.expected("c2", W, H, S_lo, S_hi, T, A, R, F, MOVES["c2"])
    scene, depth = sc.scene_of("c2")
    s_abi = scene.to_abi()
    d = np.ascontiguousarray(e["d"])
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f32 = np.zeros((H, W, 4), np.float32)
    u8 = np.zeros((H, W, 4), np.uint8)
    f64 = np.zeros((H, W, 3), np.float64)
    ref = np.full((H, W), 7, np.uint8)
    st = abi.rt_stats()
    n = ctypes.c_uint64(0)
    L = abi.lib()
    abi.check(L.rt_render_lens_adaptive(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(e["cam"]), W, H, depth, S_lo, S_hi,
                                        T, A, R, F, ctypes.c_void_p(f32.ctypes.data), ctypes.c_void_p(u8.ctypes.data),
                                        ctypes.c_void_p(f64.ctypes.data), ctypes.c_void_p(ref.ctypes.data),
                                        ctypes.byref(st), ctypes.byref(n)), "rt_render_lens_adaptive")
    sc.assert_same_bits(f64, e["rgb"], "rgb64f")
    sc.assert_same_bits(f32, sc.to_rgba32f(e["rgb"]), "rgba32f")
    assert np.array_equal(u8, sc.to_rgba8(e["rgb"])) and np.array_equal(ref, e["mask"].astype(np.uint8))
    nref = int(e["mask"].sum())
    assert n.value == nref and 0 < nref < W * H
    seg, sh = int(e["rc2"][..., 0].sum(dtype=np.uint64)), int(e["rc2"][..., 1].sum(dtype=np.uint64))
    prim = (W * H - nref) * S_lo * S_lo + nref * S_hi * S_hi
    assert st.primary_rays == prim
    assert st.reflect_rays == seg - prim and st.shadow_rays == sh
    # every pointer optional
    n.value = 0
    abi.check(L.rt_render_lens_adaptive(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(e["cam"]), W, H, depth, S_lo, S_hi,
                                        T, A, R, F, None, None, None, None, None, ctypes.byref(n)),
              "rt_render_lens_adaptive")
    assert n.value == nref
    # no displacement: the frozen frame
    e0 = la.expected("c2", W, H, S_lo, S_hi, T, A, R, F)
    abi.check(L.rt_render_lens_adaptive(tr._ctx, ctypes.byref(s_abi), None, ctypes.byref(e["cam"]), W, H, depth, S_lo,
                                        S_hi, T, A, R, F, None, None, ctypes.c_void_p(f64.ctypes.data),
                                        ctypes.c_void_p(ref.ctypes.data), None, None), "rt_render_lens_adaptive")
    sc.assert_same_bits(f64, e0["rgb"], "without displacement")
    assert np.array_equal(ref, e0["mask"].astype(np.uint8))


def test_cli(tmp_path):
    e = la.expected("c2", W, H, 2, 4, 8, A, R, 0.5, MOVES["c2"])
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c2_lens_adaptive.ppm"
    args = [exe, "--config", "c2", "--width", str(W), "--height", str(H), "--samples", "4", "--coarse", "2", "--refine",
            "8", "--aperture", "8", "--light-size", "40", "--shutter", "0.5", "--move", "4:50,0,0", "--move",
            "0:0,12,-30", "--out", str(out)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    nref = int(e["mask"].sum())
    line = [ln for ln in r.stdout.splitlines() if "pixels refined" in ln]
    assert len(line) == 1 and f"{nref} of {W * H} pixels refined from 2 x 2 to 4 x 4 samples" in line[0], r.stdout
    assert np.array_equal(_read_ppm(out), sc.to_rgba8(e["rgb"])[::-1, :, :3])     # PPM rows run top to bottom


# 12. argument errors -----------------------------------------------------------------------------------------
def test_argument_errors(tr):
    e = la.expected("c2", W, H, 2, 4, T, A, R, F, MOVES["c2"])
    depth = _set(tr, "c2", e)
    cam = scenes.make_camera(W, H, 500.0 / W)
    bufs = tr.alloc_lens_adaptive(W, H, rgba32f=False, rgb64f=True)
    out, ws = bufs["rgb64f"], bufs["workspace"]
    out.fill_(-7.0)
    bufs["refined"].fill_(9)
    L = abi.lib()

    def call(S_lo=2, S_hi=4, thr=T, ap=A, ls=R, sh=F, c=cam, w=W, h=H, wsp=ws.data_ptr(), wsn=ws.numel()):
        return L.rt_render_lens_adaptive_dev(tr._ctx, ctypes.byref(c), w, h, depth, S_lo, S_hi, thr, ap, ls, sh, None,
                                             None, ctypes.c_void_p(out.data_ptr()), None,
                                             ctypes.c_void_p(bufs["refined"].data_ptr()), ctypes.c_void_p(wsp), wsn,
                                             lg.stream_ptr())

    for S in (0, 3, 16, -2):
        assert call(S_lo=S) == abi.RT_EINVAL and "samples_lo" in abi.last_error(), S
        assert call(S_hi=S) == abi.RT_EINVAL and "samples_hi" in abi.last_error(), S
    for lo, hi in ((4, 2), (8, 1), (2, 1)):
        assert call(S_lo=lo, S_hi=hi) == abi.RT_EINVAL and "samples_lo" in abi.last_error(), (lo, hi)
    for thr in (-2, 256, 1000):
        assert call(thr=thr) == abi.RT_EINVAL and "threshold" in abi.last_error(), thr
        with pytest.raises(abi.RtError) as ei:
            tr.render_lens_adaptive_into(cam, W, H, depth, 2, 4, thr, A, R, F, bufs)
        assert ei.value.code == abi.RT_EINVAL and "threshold" in str(ei.value)
    for v in BAD:
        assert call(ap=v) == abi.RT_EINVAL and "aperture" in abi.last_error(), v
        assert call(ls=v) == abi.RT_EINVAL and "light_size" in abi.last_error(), v
    for v in BAD + (1.0000000000000002, 2.0):
        assert call(sh=v) == abi.RT_EINVAL and "shutter" in abi.last_error(), v
    assert call(wsp=None, wsn=ws.numel()) == abi.RT_EINVAL and "workspace" in abi.last_error()
    assert call(wsp=ws.data_ptr() + 8) == abi.RT_EINVAL and "workspace" in abi.last_error()
    assert call(wsn=ws.numel() - 1) == abi.RT_EINVAL and "workspace" in abi.last_error()
    assert call(wsn=0) == abi.RT_EINVAL and "workspace" in abi.last_error()
    for w, h in ((0, H), (W, 0), (-1, H), (W, -5), (65536, 65536), (2 ** 30, 1)):
        assert call(S_hi=8, w=w, h=h) == abi.RT_EINVAL and "size" in abi.last_error(), (w, h)
    # the S_hi camera overflows where the S_lo camera does not, and both
    for bx in (-(2 ** 29) - 1, -(2 ** 30) - 1):
        far = scenes.make_camera(W, H, 500.0 / W)
        far.bottom_x = bx
        assert call(c=far) == abi.RT_EINVAL and "overflow" in abi.last_error(), bx
    # the host entry point
    s_abi = sc.scene_of("c2")[0].to_abi()
    for lo, hi, thr, ap, ls, sh, word in ((3, 4, T, A, R, F, "samples"), (2, 5, T, A, R, F, "samples"),
                                          (4, 2, T, A, R, F, "samples_lo"), (2, 4, 300, A, R, F, "threshold"),
                                          (2, 4, T, -1.0, R, F, "aperture"), (2, 4, T, A, -1.0, F, "light_size"),
                                          (2, 4, T, A, R, 1.5, "shutter")):
        rc = L.rt_render_lens_adaptive(tr._ctx, ctypes.byref(s_abi), None, ctypes.byref(cam), W, H, depth, lo, hi, thr,
                                       ap, ls, sh, None, None, None, None, None, None)
        assert rc == abi.RT_EINVAL and word in abi.last_error(), word
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (bufs["refined"] == 9).all(), "a rejected call wrote pixels"
    assert call() == abi.RT_OK                                                    # the same buffers, good arguments
    got = _host(bufs)
    sc.assert_same_bits(got["rgb64f"], e["rgb"], "after the errors")
    assert np.array_equal(got["refined"], e["mask"].astype(np.uint8))
