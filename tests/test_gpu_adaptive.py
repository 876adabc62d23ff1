"""GPU: adaptive supersampling (rt_render_adaptive_dev / rt_render_adaptive, Tracer.render_adaptive, the CLI)
against the contract of include/rt_api.h evaluated on the CPU oracle's frames (tests/adaptive_common.py) and against
the fixtures made from the reference build (tests/golden/ssaa.npz).  Expected values never come from the code under
test.

Float images are compared bit for bit (NaNs by position: their sign and payload are unspecified); byte images, ray
counters and `refined` exactly.  Frames are 37 x 21 at pitch 500 / 37 unless said.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402

from . import adaptive_common as ac  # noqa: E402
from . import ssaa_common as sc  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 37, 21


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    t = Tracer(0)
    yield t
    t.close()


@pytest.fixture()
def fresh():
    """A context of its own: the tests of the per-view and per-workspace state."""
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    t = Tracer(0)
    yield t
    t.close()


def _host(bufs):
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items() if v is not None and k != "workspace"}
    if "raycount" in out:
        out["raycount"] = out["raycount"].view(np.uint32)
    return out


def _render(t, cam, w, h, depth, S, T):
    return _host(t.render_adaptive(cam, w, h, depth, S, T, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))


def _check_all(got, rgb, rc2, mask, what):
    """Every output of an adaptive render against the expected float64 frame, counters and mask."""
    assert np.array_equal(got["refined"], mask.astype(np.uint8)), what + " refined"
    sc.assert_same_bits(got["rgb64f"], rgb, what + " rgb64f")
    sc.assert_same_bits(got["rgba32f"], sc.to_rgba32f(rgb), what + " rgba32f")
    assert np.array_equal(got["rgba8"], sc.to_rgba8(rgb)), what + " rgba8"
    assert got["raycount"].shape == rc2.shape and np.array_equal(got["raycount"], rc2), what + " raycount"


def _check_expected(got, e, what):
    _check_all(got, e["rgb"], e["rc2"], e["mask"], what)


# 1. every refine instance, a mask that refines part of the frame ---------------------------------------------
@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_variants(tr, name, S):
    """c2 depth 1 and c5 depth 3: the opaque instance; demo depth 5: the transparent one; tree_demo depth 5: the
    ray-tree one.  A render that refines everything, nothing or another set of pixels cannot pass: enough unrefined
    pixels differ between the supersampled and the base frame, and enough refined ones."""
    T = 32
    e = ac.expected(name, W, H, S, T)
    assert not np.isnan(e["rgb"]).any()
    share = e["mask"].mean()
    diff = ac.differ(e["ss"], e["base"])
    n_unref, n_ref = int((diff & ~e["mask"]).sum()), int((diff & e["mask"]).sum())
    print(f"{name} S={S} T={T}: refined share {share:.3f}, unrefined-but-different {n_unref}, "
          f"refined-and-different {n_ref}")
    assert 0.3 <= share <= 0.7
    assert n_unref >= 15
    assert n_ref >= 200
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    _check_expected(_render(tr, e["cam"], W, H, depth, S, T), e, f"{name} S={S}")


# 2. T = -1 against the fixtures from the reference build -----------------------------------------------------
@pytest.mark.parametrize("name,S", sc.FIXTURES)
def test_refine_everything_is_the_ssaa_fixture(tr, name, S):
    want = sc.fixtures()[sc.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    cam = scenes.make_camera(sc.FIX_W, sc.FIX_H, 500.0 / sc.FIX_W)
    got = _host(tr.render_adaptive(cam, sc.FIX_W, sc.FIX_H, depth, S, -1, rgba32f=False, rgb64f=True))
    assert got["refined"].shape == (sc.FIX_H, sc.FIX_W) and (got["refined"] == 1).all()
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S}")


# ... and T = 32 against the adaptive fixtures
@pytest.mark.parametrize("name,S", ac.FIXTURES)
def test_adaptive_fixtures(tr, name, S):
    fx = ac.fixtures()
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    cam = scenes.make_camera(ac.FIX_W, ac.FIX_H, 500.0 / ac.FIX_W)
    got = _host(tr.render_adaptive(cam, ac.FIX_W, ac.FIX_H, depth, S, ac.FIX_T, rgba32f=False, rgb64f=True))
    assert np.array_equal(got["refined"], fx[sc.fixture_key(name, S) + "_mask"])
    sc.assert_same_bits(got["rgb64f"], fx[sc.fixture_key(name, S)], f"{name} S={S}")


# 3. T = 255 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", [("c2", 4), ("demo", 2)])
def test_refine_nothing_is_the_plain_render(tr, name, S):
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    base, base_rc, cam = ac.base_frame(name, W, H)
    plain = _host(tr.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True))
    assert plain["rgb64f"].tobytes() == base.tobytes()
    got = _render(tr, cam, W, H, depth, S, 255)
    for k in ("rgba32f", "rgba8", "rgb64f"):
        assert got[k].tobytes() == plain[k].tobytes(), k
    assert (got["refined"] == 0).all()
    assert np.array_equal(got["raycount"], sc.reduce_counts(base_rc, 1))


# 4. NaN frames ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
def test_nan_frames(tr, S):
    T = 32
    e = ac.expected("tree_c2", W, H, S, T)
    base_nan = np.isnan(e["base"]).any(axis=2)
    assert base_nan.sum() == 38
    assert (sc.to_rgba8(e["base"])[..., :3][np.isnan(e["base"])] == 0).all()      # the criterion's bytes of a NaN
    assert 0 < e["mask"].sum() < W * H
    scene, depth = sc.scene_of("tree_c2")
    assert depth == 3
    tr.set_scene(scene)
    got = _render(tr, e["cam"], W, H, depth, S, T)
    assert np.array_equal(np.isnan(got["rgb64f"]), np.isnan(e["rgb"]))
    _check_expected(got, e, f"tree_c2 S={S}")
    assert (got["rgba8"][..., :3][np.isnan(e["rgb"])] == 0).all()


# 5. the smallest shapes: neighbour indexing at the frame's edges, lists shorter than a wave ------------------
def _small_expected(w, h, S, T):
    """c2 on a w x h frame at pitch 500 / 37 (the camera of that size, not a crop)."""
    scene, depth = sc.scene_of("c2")
    cam = scenes.make_camera(w, h, 500.0 / 37)
    cam_s = sc.camera_ss(cam, S)
    base, base_rc = po.render(scene.to_abi(), cam, w, h, depth)
    hi, hi_rc = po.render(scene.to_abi(), cam_s, S * w, S * h, depth)
    rgb, rc2, mask = ac.combine(base, base_rc, sc.reduce_tree(hi, S), sc.reduce_counts(hi_rc, S), T)
    return cam, depth, rgb, rc2, mask


@pytest.mark.parametrize("T", [0, -1])
@pytest.mark.parametrize("w,h", [(1, 1), (9, 1), (1, 9), (8, 8), (9, 9)])
def test_small_frames(tr, w, h, T):
    S = 4
    cam, depth, rgb, rc2, mask = _small_expected(w, h, S, T)
    if (w, h) == (1, 1):
        assert not mask.any()
    elif T == -1:
        assert mask.all()
    scene, _ = sc.scene_of("c2")
    tr.set_scene(scene)
    _check_all(_render(tr, cam, w, h, depth, S, T), rgb, rc2, mask, f"{w}x{h} T={T}")


def test_several_classification_workgroups(tr):
    """131 x 100 = 13100 pixels: the classification pass compacts 8192 pixels per workgroup, so the list is filled by
    two workgroups (the second one partly empty, its last wave partial) and a row straddles their boundary."""
    w, h, S, T = 131, 100, 2, 32
    e = ac.expected("c2", w, h, S, T)
    assert w * h > 8192 and 0.05 < e["mask"].mean() < 0.95
    assert e["mask"].reshape(-1)[:8192].any() and e["mask"].reshape(-1)[8192:].any()
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    _check_expected(_render(tr, e["cam"], w, h, depth, S, T), e, f"{w}x{h}")
    e1 = ac.expected("c2", w, h, S, -1)
    _check_expected(_render(tr, e1["cam"], w, h, depth, S, -1), e1, f"{w}x{h} T=-1")


# 6. one context, one workspace, thresholds in turn -----------------------------------------------------------
def test_one_workspace_many_thresholds(fresh):
    """A stale counter or list, the first / calibration / cached base renders, and base bytes overwritten by the
    previous refine pass (the byte image is the criterion's input and the refine pass's output)."""
    S = 2
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    bufs = fresh.alloc_adaptive(W, H, S, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    for k, T in enumerate([-1, 32, 255, 32, -1, 32, 32, 32]):
        e = ac.expected("c2", W, H, S, T)
        fresh.render_adaptive_into(e["cam"], W, H, depth, S, T, bufs)
        _check_expected(_host(bufs), e, f"render {k} T={T}")


def test_workspace_base_bytes(fresh):
    """Without an rgba8 output the base bytes live in the workspace."""
    S, T = 4, 32
    e = ac.expected("c2", W, H, S, T)
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    bufs = fresh.alloc_adaptive(W, H, S, rgba32f=False, rgba8=False, rgb64f=True, raycount=False)
    for k in range(3):
        fresh.render_adaptive_into(e["cam"], W, H, depth, S, T, bufs)
        got = _host(bufs)
        assert np.array_equal(got["refined"], e["mask"].astype(np.uint8))
        sc.assert_same_bits(got["rgb64f"], e["rgb"], f"render {k}")
    n = int(bufs["workspace"][:4].cpu().numpy().view(np.uint32)[0])
    assert n == int(e["mask"].sum())


# 7. hipGraph capture -----------------------------------------------------------------------------------------
def test_graph_capture(fresh):
    S, T = 2, 32
    e = ac.expected("c2", W, H, S, T)
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    bufs = fresh.alloc_adaptive(W, H, S, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fresh.render_adaptive_into(e["cam"], W, H, depth, S, T, bufs, stream=s)   # warm-up outside the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fresh.render_adaptive_into(e["cam"], W, H, depth, S, T, bufs, stream=s)
    for k in range(3):
        for name, b in bufs.items():
            if b is not None and name != "workspace":
                b.zero_()
        g.replay()
        _check_expected(_host(bufs), e, f"replay {k}")


# 8. rt_render_adaptive: host buffers -------------------------------------------------------------------------
def test_render_adaptive_host_buffers(tr):
    S, T = 4, 32
    e = ac.expected("c2", W, H, S, T)
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    dev = _render(tr, e["cam"], W, H, depth, S, T)
    f32 = np.zeros((H, W, 4), np.float32)
    u8 = np.zeros((H, W, 4), np.uint8)
    f64 = np.zeros((H, W, 3), np.float64)
    ref = np.full((H, W), 7, np.uint8)
    st = abi.rt_stats()
    n = ctypes.c_uint64(0)
    s_abi = scene.to_abi()
    abi.check(abi.lib().rt_render_adaptive(tr._ctx, ctypes.byref(s_abi), ctypes.byref(e["cam"]), W, H, depth, S, T,
                                           ctypes.c_void_p(f32.ctypes.data), ctypes.c_void_p(u8.ctypes.data),
                                           ctypes.c_void_p(f64.ctypes.data), ctypes.c_void_p(ref.ctypes.data),
                                           ctypes.byref(st), ctypes.byref(n)), "rt_render_adaptive")
    assert f64.tobytes() == dev["rgb64f"].tobytes() and ref.tobytes() == dev["refined"].tobytes()
    assert f32.tobytes() == dev["rgba32f"].tobytes() and u8.tobytes() == dev["rgba8"].tobytes()
    sc.assert_same_bits(f64, e["rgb"], "rt_render_adaptive rgb64f")
    assert np.array_equal(ref, e["mask"].astype(np.uint8))
    nref = int(e["mask"].sum())
    assert n.value == nref and 0 < nref < W * H
    seg, sh = int(e["rc2"][..., 0].sum(dtype=np.uint64)), int(e["rc2"][..., 1].sum(dtype=np.uint64))
    prim = (W * H - nref) + nref * S * S
    assert st.primary_rays == prim
    assert st.reflect_rays == seg - prim and st.shadow_rays == sh
    # every pointer optional
    n.value = 0
    abi.check(abi.lib().rt_render_adaptive(tr._ctx, ctypes.byref(s_abi), ctypes.byref(e["cam"]), W, H, depth, S, T,
                                           None, None, None, None, None, ctypes.byref(n)), "rt_render_adaptive")
    assert n.value == nref


# 9. the CLI --------------------------------------------------------------------------------------------------
def _read_ppm(path):
    hdr, body = open(path, "rb").read().split(b"\n", 1)
    assert hdr.split() == [b"P6", str(W).encode(), str(H).encode(), b"255"]
    return np.frombuffer(body, np.uint8).reshape(H, W, 3)


def test_cli(tmp_path):
    e = ac.expected("c2", W, H, 2, 32)
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c2_adaptive.ppm"
    r = subprocess.run([exe, "--config", "c2", "--width", str(W), "--height", str(H), "--samples", "2", "--adaptive",
                        "32", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"{int(e['mask'].sum())} of {W * H} pixels refined" in r.stdout
    assert np.array_equal(_read_ppm(out), sc.to_rgba8(e["rgb"])[::-1, :, :3])     # PPM rows run top to bottom


# 10. argument errors -----------------------------------------------------------------------------------------
def _call_dev(t, cam, bufs, S, T, ws_bytes=None):
    """rt_render_adaptive_dev (c2, depth 1) into bufs["rgb64f"] with bufs["workspace"]."""
    ws = bufs["workspace"]
    return abi.lib().rt_render_adaptive_dev(
        t._ctx, ctypes.byref(cam), W, H, 1, S, T, None, None, ctypes.c_void_p(bufs["rgb64f"].data_ptr()), None, None,
        ctypes.c_void_p(ws.data_ptr()), ws.numel() if ws_bytes is None else ws_bytes,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_argument_errors(tr):
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    bufs = tr.alloc_adaptive(W, H, 2, rgba32f=False, rgb64f=True)
    need = bufs["workspace"].numel()
    for S in (0, 3, 16):
        assert _call_dev(tr, cam, bufs, S, 32) == abi.RT_EINVAL and "samples" in abi.last_error()
        with pytest.raises(abi.RtError) as ei:
            tr.alloc_adaptive(W, H, S)
        assert ei.value.code == abi.RT_EINVAL and "samples" in str(ei.value)
    for T in (-2, 256, 1000):
        assert _call_dev(tr, cam, bufs, 2, T) == abi.RT_EINVAL and "threshold" in abi.last_error()
        with pytest.raises(abi.RtError) as ei:
            tr.render_adaptive_into(cam, W, H, depth, 2, T, bufs)
        assert ei.value.code == abi.RT_EINVAL and "threshold" in str(ei.value)
    assert _call_dev(tr, cam, bufs, 2, 32, ws_bytes=need - 1) == abi.RT_EINVAL and "workspace" in abi.last_error()
    assert _call_dev(tr, cam, bufs, 2, 32, ws_bytes=0) == abi.RT_EINVAL and "workspace" in abi.last_error()
    rc = abi.lib().rt_render_adaptive_dev(tr._ctx, ctypes.byref(cam), W, H, 1, 2, 32, None, None,
                                          ctypes.c_void_p(bufs["rgb64f"].data_ptr()), None, None, None, need, None)
    assert rc == abi.RT_EINVAL and "workspace" in abi.last_error()
    far = scenes.make_camera(W, H, 500.0 / W)
    far.bottom_x = -(2 ** 30) - 1
    assert _call_dev(tr, far, bufs, 2, 32) == abi.RT_EINVAL and "overflow" in abi.last_error()
    s_abi = scene.to_abi()
    for S, T, word in ((3, 32, "samples"), (2, 256, "threshold")):
        rc = abi.lib().rt_render_adaptive(tr._ctx, ctypes.byref(s_abi), ctypes.byref(cam), W, H, depth, S, T, None, None,
                                          None, None, None, None)
        assert rc == abi.RT_EINVAL and word in abi.last_error()
    torch.cuda.synchronize()
    assert _call_dev(tr, cam, bufs, 2, 32) == abi.RT_OK     # the same buffers with good arguments
    torch.cuda.synchronize()
