"""GPU: depth of field (rt_render_dof_dev / rt_render_dof, Tracer.render_dof, the CLI) against the contract of
include/rt_api.h evaluated on rays traced by the CPU oracle (tests/dof_common.py) and against the fixtures made from
the reference build (tests/golden/dof.npz, tests/golden/ssaa.npz).  Expected values never come from the code under
test.

Float images are compared bit for bit (NaNs by position: their sign and payload are unspecified); byte images and
ray counters exactly.  Frames are 37 x 21 at pitch 500 / 37 unless said: partial 8 x 8 sample tiles in both axes at
S = 2 and S = 4, one pixel per wave at S = 8.  tests/test_dof_oracle.py shows that the lens changes these frames
in at least 30 % of their pixels, so a kernel that ignores it cannot pass.
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

from . import dof_common as dc  # noqa: E402
from . import ssaa_common as sc  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, A = 37, 21, 8.0


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    t = Tracer(0)
    yield t
    t.close()


@pytest.fixture()
def fresh():
    """A context of its own: the tests of the per-view state."""
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    t = Tracer(0)
    yield t
    t.close()


def _host(bufs):
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}
    if "raycount" in out:
        out["raycount"] = out["raycount"].view(np.uint32)
    return out


def _render(t, cam, w, h, depth, S, aperture):
    return _host(t.render_dof(cam, w, h, depth, S, aperture, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))


def _check_all(got, rgb, rc2, what):
    """Every output of a depth-of-field render against the expected float64 frame and counters."""
    sc.assert_same_bits(got["rgb64f"], rgb, what + " rgb64f")
    sc.assert_same_bits(got["rgba32f"], sc.to_rgba32f(rgb), what + " rgba32f")
    assert np.array_equal(got["rgba8"], sc.to_rgba8(rgb)), what + " rgba8"
    assert got["raycount"].shape == rc2.shape and np.array_equal(got["raycount"], rc2), what + " raycount"


# 1. every instance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_variants(tr, name, S):
    """c2 depth 1 and c5 depth 3: the opaque instance; demo depth 5: the FULL one; tree_demo depth 5: the ray-tree
    one."""
    e = dc.expected(name, W, H, S, A)
    assert not np.isnan(e["rgb"]).any()
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    _check_all(_render(tr, e["cam"], W, H, depth, S, A), e["rgb"], e["rc2"], f"{name} S={S}")


# 2. the fixtures from the reference build ----------------------------------------------------------------------
@pytest.mark.parametrize("name,S", dc.FIXTURES)
def test_dof_fixtures(tr, name, S):
    want = dc.fixtures()[sc.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    cam = scenes.make_camera(dc.FIX_W, dc.FIX_H, 500.0 / dc.FIX_W)
    got = _host(tr.render_dof(cam, dc.FIX_W, dc.FIX_H, depth, S, dc.FIX_A, rgba32f=False, rgb64f=True))
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S}")


@pytest.mark.parametrize("name,S", sc.FIXTURES)
def test_aperture_zero_is_the_ssaa_fixture(tr, name, S):
    """A = 0 runs the same kernel as any other aperture, so ssaa.npz checks it too."""
    want = sc.fixtures()[sc.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    cam = scenes.make_camera(sc.FIX_W, sc.FIX_H, 500.0 / sc.FIX_W)
    got = _host(tr.render_dof(cam, sc.FIX_W, sc.FIX_H, depth, S, 0.0, rgba32f=False, rgb64f=True, raycount=True))
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S}")
    assert np.array_equal(got["raycount"], sc.expected(name, sc.FIX_W, sc.FIX_H, S)["rc2"])


# 3. S = 1 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_one_sample_is_the_plain_render(tr, name):
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    want, want_rc = po.render(scene.to_abi(), cam, W, H, depth)
    plain = _host(tr.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True))
    assert plain["rgb64f"].tobytes() == want.tobytes()
    got = _render(tr, cam, W, H, depth, 1, A)
    for k in ("rgba32f", "rgba8", "rgb64f"):
        assert got[k].tobytes() == plain[k].tobytes(), k
    assert np.array_equal(got["raycount"], sc.reduce_counts(want_rc, 1))


# 4. NaN frames -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
def test_nan_frames(tr, S):
    e = dc.expected("tree_c2", W, H, S, A)
    nan_px = np.isnan(e["rgb"]).any(axis=2)
    assert 0 < nan_px.sum() <= 0.25 * W * H
    scene, depth = sc.scene_of("tree_c2")
    assert depth == 3
    tr.set_scene(scene)
    got = _render(tr, e["cam"], W, H, depth, S, A)
    assert np.array_equal(np.isnan(got["rgb64f"]), np.isnan(e["rgb"]))
    _check_all(got, e["rgb"], e["rc2"], f"tree_c2 S={S}")
    assert (got["rgba8"][..., :3][np.isnan(e["rgb"])] == 0).all()


# 5. focus ----------------------------------------------------------------------------------------------------
def test_focus(tr):
    S = 4
    e, e1 = dc.expected("c2", W, H, S, A, 0.5), dc.expected("c2", W, H, S, A)
    assert dc.differ(e["rgb"], e1["rgb"]).mean() >= 0.30
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    cam = scenes.focus_camera(scenes.make_camera(W, H, 500.0 / W), 0.5)
    got = _render(tr, cam, W, H, depth, S, A)
    _check_all(got, e["rgb"], e["rc2"], "focus 0.5")
    got1 = _render(tr, scenes.make_camera(W, H, 500.0 / W), W, H, depth, S, A)
    assert dc.differ(got["rgb64f"], got1["rgb64f"]).mean() >= 0.30


# 6. the smallest shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (9, 1), (1, 9), (8, 8), (9, 9)])
def test_small_frames(tr, w, h, S):
    """c2 on a w x h frame at pitch 500 / 37 (the camera of that size, not a crop)."""
    scene, depth = sc.scene_of("c2")
    cam = scenes.make_camera(w, h, 500.0 / 37)
    e = dc.render(scene, cam, w, h, depth, S, A)
    tr.set_scene(scene)
    _check_all(_render(tr, cam, w, h, depth, S, A), e["rgb"], e["rc2"], f"{w}x{h} S={S}")


# 7. each output alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("only", ["rgba32f", "rgba8", "rgb64f", "raycount"])
def test_nullable_outputs(tr, only):
    S = 2
    e = dc.expected("c2", W, H, S, A)
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    got = _host(tr.render_dof(e["cam"], W, H, depth, S, A, **{k: k == only for k in
                                                              ("rgba32f", "rgba8", "rgb64f", "raycount")}))
    assert list(got) == [only]
    want = {"rgba32f": sc.to_rgba32f(e["rgb"]), "rgba8": sc.to_rgba8(e["rgb"]), "rgb64f": e["rgb"],
            "raycount": e["rc2"]}[only]
    assert got[only].shape == want.shape and got[only].tobytes() == want.tobytes()


def test_no_outputs_is_a_no_op(tr):
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    rc = abi.lib().rt_render_dof_dev(tr._ctx, ctypes.byref(cam), W, H, depth, 2, A, None, None, None, None,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == abi.RT_OK
    torch.cuda.synchronize()


# 8. no per-view side effect ----------------------------------------------------------------------------------
def test_no_per_view_side_effect(fresh):
    """A view's first, calibration and cached renders, then depth-of-field frames of another aperture and another
    eye, then the view again: its cone and level masks and its tile order must still be the view's."""
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    want, want_rc = po.render(scene.to_abi(), cam, W, H, depth)
    frames = [_host(fresh.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
              for _ in range(3)]
    assert frames[0]["rgb64f"].tobytes() == want.tobytes()
    assert np.array_equal(frames[0]["raycount"], want_rc)
    other = scenes.make_camera(W, H, 500.0 / W)
    other.eye[0] += 40.0
    other.eye[1] += 25.0
    for c, S, ap in ((cam, 2, 3.0), (other, 4, A), (other, 2, 0.0)):
        e = dc.render(scene, c, W, H, depth, S, ap)
        _check_all(_render(fresh, c, W, H, depth, S, ap), e["rgb"], e["rc2"], f"S={S} A={ap}")
    frames.append(_host(fresh.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)))
    for k, f in enumerate(frames[1:]):
        for key in ("rgba32f", "rgba8", "rgb64f", "raycount"):
            assert f[key].tobytes() == frames[0][key].tobytes(), (k + 1, key)


# 9. hipGraph capture -----------------------------------------------------------------------------------------
def test_graph_capture(fresh):
    S = 2
    e = dc.expected("c2", W, H, S, A)
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    bufs = fresh.alloc_ss(W, H, None, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fresh.render_dof_into(e["cam"], W, H, depth, S, A, bufs, stream=s)       # warm-up outside the capture
    s.synchronize()
    _check_all(_host(bufs), e["rgb"], e["rc2"], "direct")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fresh.render_dof_into(e["cam"], W, H, depth, S, A, bufs, stream=s)
    for k in range(2):
        for b in bufs.values():
            if b is not None:
                b.zero_()
        g.replay()
        _check_all(_host(bufs), e["rgb"], e["rc2"], f"replay {k}")
        plain = _host(fresh.render(e["cam"], W, H, depth, rgb64f=True))          # another render in between
        assert plain["rgb64f"].shape == (H, W, 3)


# 10. rt_render_dof: host buffers and the CLI -------------------------------------------------------------------
def test_render_dof_host_buffers(tr):
    S = 4
    e = dc.expected("c2", W, H, S, A)
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    f32 = np.zeros((H, W, 4), np.float32)
    u8 = np.zeros((H, W, 4), np.uint8)
    f64 = np.zeros((H, W, 3), np.float64)
    st = abi.rt_stats()
    s_abi = scene.to_abi()
    abi.check(abi.lib().rt_render_dof(tr._ctx, ctypes.byref(s_abi), ctypes.byref(e["cam"]), W, H, depth, S, A,
                                      ctypes.c_void_p(f32.ctypes.data), ctypes.c_void_p(u8.ctypes.data),
                                      ctypes.c_void_p(f64.ctypes.data), ctypes.byref(st)), "rt_render_dof")
    sc.assert_same_bits(f64, e["rgb"], "rt_render_dof rgb64f")
    sc.assert_same_bits(f32, sc.to_rgba32f(e["rgb"]), "rt_render_dof rgba32f")
    assert np.array_equal(u8, sc.to_rgba8(e["rgb"]))
    seg, sh = int(e["rc2"][..., 0].sum(dtype=np.uint64)), int(e["rc2"][..., 1].sum(dtype=np.uint64))
    assert st.primary_rays == W * H * S * S
    assert st.reflect_rays == seg - W * H * S * S and st.shadow_rays == sh
    # every pointer optional
    abi.check(abi.lib().rt_render_dof(tr._ctx, ctypes.byref(s_abi), ctypes.byref(e["cam"]), W, H, depth, S, A,
                                      None, None, None, None), "rt_render_dof")


def _read_ppm(path):
    hdr, body = open(path, "rb").read().split(b"\n", 1)
    assert hdr.split() == [b"P6", str(W).encode(), str(H).encode(), b"255"]
    return np.frombuffer(body, np.uint8).reshape(H, W, 3)


@pytest.mark.parametrize("ratio", [None, 0.5])
def test_cli(tmp_path, ratio):
    e = dc.expected("c2", W, H, 2, A, 1.0 if ratio is None else ratio)
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c2_dof.ppm"
    args = [exe, "--config", "c2", "--width", str(W), "--height", str(H), "--samples", "2", "--aperture", "8",
            "--out", str(out)] + ([] if ratio is None else ["--focus", str(ratio)])
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "depth of field" in r.stdout and f"primary {W * H * 4}," in r.stdout
    assert np.array_equal(_read_ppm(out), sc.to_rgba8(e["rgb"])[::-1, :, :3])     # PPM rows run top to bottom


# 11. argument errors -----------------------------------------------------------------------------------------
def _call_dev(t, cam, out, w, h, S, aperture):
    return abi.lib().rt_render_dof_dev(t._ctx, ctypes.byref(cam), w, h, 1, S, aperture, None, None,
                                       ctypes.c_void_p(out.data_ptr()), None,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_argument_errors(tr):
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    bufs = tr.alloc_ss(W, H, None, rgba32f=False, rgb64f=True)
    out = bufs["rgb64f"]
    out.fill_(-7.0)
    for S in (0, 3, 16, -2):
        assert _call_dev(tr, cam, out, W, H, S, A) == abi.RT_EINVAL and "samples" in abi.last_error()
        with pytest.raises(abi.RtError) as ei:
            tr.render_dof_into(cam, W, H, depth, S, A, bufs)
        assert ei.value.code == abi.RT_EINVAL and "samples" in str(ei.value)
    for ap in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        assert _call_dev(tr, cam, out, W, H, 2, ap) == abi.RT_EINVAL and "aperture" in abi.last_error(), ap
        with pytest.raises(abi.RtError) as ei:
            tr.render_dof_into(cam, W, H, depth, 2, ap, bufs)
        assert ei.value.code == abi.RT_EINVAL and "aperture" in str(ei.value)
    for w, h in ((0, H), (W, 0), (-1, H), (W, -5), (65536, 65536), (2 ** 30, 1)):
        assert _call_dev(tr, cam, out, w, h, 8, A) == abi.RT_EINVAL and "size" in abi.last_error(), (w, h)
    far = scenes.make_camera(W, H, 500.0 / W)
    far.bottom_x = -(2 ** 30) - 1
    assert _call_dev(tr, far, out, W, H, 2, A) == abi.RT_EINVAL and "overflow" in abi.last_error()
    s_abi = scene.to_abi()
    for S, ap, word in ((3, A, "samples"), (2, -1.0, "aperture"), (2, float("nan"), "aperture")):
        rc = abi.lib().rt_render_dof(tr._ctx, ctypes.byref(s_abi), ctypes.byref(cam), W, H, depth, S, ap, None, None,
                                     None, None)
        assert rc == abi.RT_EINVAL and word in abi.last_error()
    rc = abi.lib().rt_render_dof(tr._ctx, ctypes.byref(s_abi), ctypes.byref(cam), 0, H, depth, 2, A, None, None, None,
                                 None)
    assert rc == abi.RT_EINVAL and "size" in abi.last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all(), "a rejected call wrote pixels"
    assert _call_dev(tr, cam, out, W, H, 2, A) == abi.RT_OK      # the same buffer with good arguments
    torch.cuda.synchronize()
    sc.assert_same_bits(out.cpu().numpy(), dc.expected("c2", W, H, 2, A)["rgb"], "after the errors")
