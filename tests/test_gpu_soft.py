"""GPU: soft shadows (rt_render_soft_dev / rt_render_soft, Tracer.render_soft, the CLI) against the contract of
include/rt_api.h evaluated on rays traced by the CPU oracle in scenes with displaced lights (tests/soft_common.py) and
against the fixtures made from the reference build (tests/golden/soft.npz, dof.npz, ssaa.npz).  Expected values never
come from the code under test.

Float images are compared bit for bit (NaNs by position: their sign and payload are unspecified); byte images and
ray counters exactly.  Frames are 37 x 21 at pitch 500 / 37 unless said: partial 8 x 8 sample tiles in both axes at
S = 2 and S = 4, one pixel per wave at S = 8.  tests/test_soft_oracle.py shows that a light size of 40 changes these
frames in at least 25 % of their pixels, and that the samples of at least 25 pixels of the depth-0 frame change their
shadowed state, so neither a kernel that ignores the light size nor one that filters the displaced shadow rays with
the point light's cone records can pass.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402

from . import dof_common as dc  # noqa: E402
from . import lens_gpu_common as lg  # noqa: E402
from . import soft_common as so  # noqa: E402
from . import ssaa_common as sc  # noqa: E402
from .lens_gpu_common import BAD, H, OUTS, W, _check_all, _host, _read_ppm, fresh, tr  # noqa: E402,F401

pytestmark = pytest.mark.gpu

A, R = 8.0, 40.0


def _render(t, cam, w, h, depth, S, aperture, light_size):
    return _host(t.render_soft(cam, w, h, depth, S, aperture, light_size, rgba32f=True, rgba8=True, rgb64f=True,
                               raycount=True))


# 1. every instance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_variants(tr, name, S):
    """c2 depth 1 and c5 depth 3 (64 spheres, two lights): the opaque instance; demo depth 5: the FULL one; tree_demo
    depth 5: the ray-tree one.  R = 40, A = 0."""
    e = so.expected(name, W, H, S, 0.0, R)
    assert not np.isnan(e["rgb"]).any()
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    _check_all(_render(tr, e["cam"], W, H, depth, S, 0.0, R), e["rgb"], e["rc2"], f"{name} S={S}")


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_lens_and_light_together(tr, name, S):
    e = so.expected(name, W, H, S, A, R)
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    _check_all(_render(tr, e["cam"], W, H, depth, S, A, R), e["rgb"], e["rc2"], f"{name} S={S} A={A}")


# 2. the penumbra ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 4, 8])
def test_penumbra(tr, S):
    """c2's scene at depth 0, where a pixel's value counts its lit samples: the displaced shadow rays must be tested
    against the spheres they meet, not against the ones the ray to the stored light position meets."""
    e, e0 = so.expected("c2", W, H, S, 0.0, R, None, 0), so.expected("c2", W, H, S, 0.0, 0.0, None, 0)
    flip = (so.shadowed(e) != so.shadowed(e0)).reshape(H, S, W, S).any(axis=(1, 3))
    assert flip.sum() >= 25
    scene, _ = sc.scene_of("c2")
    tr.set_scene(scene)
    got = _render(tr, e["cam"], W, H, 0, S, 0.0, R)
    _check_all(got, e["rgb"], e["rc2"], f"penumbra S={S}")
    got0 = _render(tr, e["cam"], W, H, 0, S, 0.0, 0.0)
    _check_all(got0, e0["rgb"], e0["rc2"], f"point light S={S}")


# 3. the fixtures from the reference build ----------------------------------------------------------------------
@pytest.mark.parametrize("name,S,Rf,Af,centres", so.FIXTURES)
def test_soft_fixtures(tr, name, S, Rf, Af, centres):
    want = so.fixtures()[so.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(so.scene_abi(scene, centres))
    cam = scenes.make_camera(so.FIX_W, so.FIX_H, 500.0 / so.FIX_W)
    got = _host(tr.render_soft(cam, so.FIX_W, so.FIX_H, depth, S, Af, Rf, rgba32f=False, rgb64f=True))
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S}")


@pytest.mark.parametrize("name,S", dc.FIXTURES)
def test_light_size_zero_is_the_dof_fixture(tr, name, S):
    """R = 0 runs the same kernel as any other light size, so dof.npz checks it too."""
    want = dc.fixtures()[sc.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    cam = scenes.make_camera(dc.FIX_W, dc.FIX_H, 500.0 / dc.FIX_W)
    got = _host(tr.render_soft(cam, dc.FIX_W, dc.FIX_H, depth, S, dc.FIX_A, 0.0, rgba32f=False, rgb64f=True,
                               raycount=True))
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S}")
    assert np.array_equal(got["raycount"], dc.expected(name, dc.FIX_W, dc.FIX_H, S, dc.FIX_A)["rc2"])


@pytest.mark.parametrize("name,S", sc.FIXTURES)
def test_both_zero_is_the_ssaa_fixture(tr, name, S):
    want = sc.fixtures()[sc.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    cam = scenes.make_camera(sc.FIX_W, sc.FIX_H, 500.0 / sc.FIX_W)
    got = _host(tr.render_soft(cam, sc.FIX_W, sc.FIX_H, depth, S, 0.0, 0.0, rgba32f=False, rgb64f=True,
                               raycount=True))
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S}")
    assert np.array_equal(got["raycount"], sc.expected(name, sc.FIX_W, sc.FIX_H, S)["rc2"])


# 4. S = 1 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_one_sample_is_the_plain_render(tr, name):
    lg.check_one_sample_is_the_plain_render(tr, name, lambda cam, depth: _render(tr, cam, W, H, depth, 1, A, R))


# 5. NaN frames -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
def test_nan_frames(tr, S):
    e = so.expected("tree_c2", W, H, S, 0.0, R)
    nan_px = np.isnan(e["rgb"]).any(axis=2)
    assert 0 < nan_px.sum() <= 0.25 * W * H
    scene, depth = sc.scene_of("tree_c2")
    assert depth == 3
    tr.set_scene(scene)
    lg.check_nan_frame(_render(tr, e["cam"], W, H, depth, S, 0.0, R), e, S)


# 6. a scene with no lights -----------------------------------------------------------------------------------
def test_no_lights(tr):
    scene, depth = sc.scene_of("c2")
    scene.lights = []
    cam = scenes.make_camera(W, H, 500.0 / W)
    e = so.render(scene, cam, W, H, depth, 2, 0.0, R)
    assert not e["rgb"].any() and not e["rc2"][..., 1].any() and e["rc2"][..., 0].any()
    tr.set_scene(scene)
    _check_all(_render(tr, cam, W, H, depth, 2, 0.0, R), e["rgb"], e["rc2"], "no lights")


# 7. the smallest shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (9, 1), (1, 9), (8, 8), (9, 9)])
def test_small_frames(tr, w, h, S):
    """c2 on a w x h frame at pitch 500 / 37 (the camera of that size, not a crop)."""
    scene, depth = sc.scene_of("c2")
    cam = scenes.make_camera(w, h, 500.0 / 37)
    e = so.render(scene, cam, w, h, depth, S, 0.0, R)
    tr.set_scene(scene)
    _check_all(_render(tr, cam, w, h, depth, S, 0.0, R), e["rgb"], e["rc2"], f"{w}x{h} S={S}")


# 8. each output alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("only", OUTS)
def test_nullable_outputs(tr, only):
    S = 2
    e = so.expected("c2", W, H, S, 0.0, R)
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    lg.check_nullable_output(only, e, lambda **flags: tr.render_soft(e["cam"], W, H, depth, S, 0.0, R, **flags))


def test_no_outputs_is_a_no_op(tr):
    lg.check_no_outputs_is_a_no_op(tr, "rt_render_soft_dev", A, R)


# 9. no side effect -------------------------------------------------------------------------------------------
def test_no_side_effect(fresh):
    """A view's first, calibration and cached renders and a lens frame; then soft-shadow frames of another light size
    and another eye; then the view and the lens frame again: the scene record (its light positions and cone records)
    and the per-view state must still be what they were."""
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    frames = lg.view_frames(fresh, scene, cam, depth)
    lens = _host(fresh.render_dof(cam, W, H, depth, 2, A, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
    sc.assert_same_bits(lens["rgb64f"], dc.expected("c2", W, H, 2, A)["rgb"], "lens frame")
    other = scenes.make_camera(W, H, 500.0 / W)
    other.eye[0] += 40.0
    other.eye[1] += 25.0
    for c, S, ap, ls in ((cam, 2, 0.0, 25.0), (other, 4, A, R), (other, 2, 0.0, 0.0)):
        e = so.render(scene, c, W, H, depth, S, ap, ls)
        _check_all(_render(fresh, c, W, H, depth, S, ap, ls), e["rgb"], e["rc2"], f"S={S} A={ap} R={ls}")
    lg.check_view_unchanged(frames, _host(fresh.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True,
                                                       raycount=True)))
    again = _host(fresh.render_dof(cam, W, H, depth, 2, A, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
    for key in OUTS:
        assert again[key].tobytes() == lens[key].tobytes(), key


# 10. hipGraph capture ----------------------------------------------------------------------------------------
def test_graph_capture(fresh):
    S = 2
    e = so.expected("c2", W, H, S, 0.0, R)
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    lg.check_graph_capture(fresh, e, depth,
                           lambda bufs, s: fresh.render_soft_into(e["cam"], W, H, depth, S, 0.0, R, bufs, stream=s))


# 11. rt_render_soft: host buffers and the CLI ------------------------------------------------------------------
def test_render_soft_host_buffers(tr):
    S = 4
    e = so.expected("c2", W, H, S, 0.0, R)
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    s_abi = scene.to_abi()
    lg.check_host_buffers(e, S, "rt_render_soft", lambda *out: abi.lib().rt_render_soft(
        tr._ctx, ctypes.byref(s_abi), ctypes.byref(e["cam"]), W, H, depth, S, 0.0, R, *out))
    # every pointer optional
    abi.check(abi.lib().rt_render_soft(tr._ctx, ctypes.byref(s_abi), ctypes.byref(e["cam"]), W, H, depth, S, 0.0, R,
                                       None, None, None, None), "rt_render_soft")


@pytest.mark.parametrize("aperture", [None, 8.0])
def test_cli(tmp_path, aperture):
    e = so.expected("c2", W, H, 2, 0.0 if aperture is None else aperture, R)
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c2_soft.ppm"
    args = [exe, "--config", "c2", "--width", str(W), "--height", str(H), "--samples", "2", "--light-size", "40",
            "--out", str(out)] + ([] if aperture is None else ["--aperture", "8"])
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if "soft shadows" in ln]
    assert len(line) == 1 and f"{W * H * 4} primary rays" in line[0], r.stdout
    assert np.array_equal(_read_ppm(out), sc.to_rgba8(e["rgb"])[::-1, :, :3])     # PPM rows run top to bottom


# 12. argument errors -----------------------------------------------------------------------------------------
def _call_dev(t, cam, out, w, h, S, aperture, light_size):
    return abi.lib().rt_render_soft_dev(t._ctx, ctypes.byref(cam), w, h, 1, S, aperture, light_size, None, None,
                                        ctypes.c_void_p(out.data_ptr()), None, lg.stream_ptr())


def test_argument_errors(tr):
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    bufs = tr.alloc_ss(W, H, None, rgba32f=False, rgb64f=True)
    out = bufs["rgb64f"]
    out.fill_(-7.0)
    for S in (0, 3, 16, -2):
        assert _call_dev(tr, cam, out, W, H, S, A, R) == abi.RT_EINVAL and "samples" in abi.last_error()
        with pytest.raises(abi.RtError) as ei:
            tr.render_soft_into(cam, W, H, depth, S, A, R, bufs)
        assert ei.value.code == abi.RT_EINVAL and "samples" in str(ei.value)
    for ap in BAD:
        assert _call_dev(tr, cam, out, W, H, 2, ap, R) == abi.RT_EINVAL and "aperture" in abi.last_error(), ap
    for ls in BAD:
        assert _call_dev(tr, cam, out, W, H, 2, A, ls) == abi.RT_EINVAL and "light_size" in abi.last_error(), ls
        with pytest.raises(abi.RtError) as ei:
            tr.render_soft_into(cam, W, H, depth, 2, A, ls, bufs)
        assert ei.value.code == abi.RT_EINVAL and "light_size" in str(ei.value)
    for w, h in ((0, H), (W, 0), (-1, H), (W, -5), (65536, 65536), (2 ** 30, 1)):
        assert _call_dev(tr, cam, out, w, h, 8, A, R) == abi.RT_EINVAL and "size" in abi.last_error(), (w, h)
    far = scenes.make_camera(W, H, 500.0 / W)
    far.bottom_x = -(2 ** 30) - 1
    assert _call_dev(tr, far, out, W, H, 2, A, R) == abi.RT_EINVAL and "overflow" in abi.last_error()
    s_abi = scene.to_abi()
    for S, ap, ls, word in ((3, A, R, "samples"), (2, -1.0, R, "aperture"), (2, A, -1.0, "light_size"),
                            (2, A, float("nan"), "light_size")):
        rc = abi.lib().rt_render_soft(tr._ctx, ctypes.byref(s_abi), ctypes.byref(cam), W, H, depth, S, ap, ls, None,
                                      None, None, None)
        assert rc == abi.RT_EINVAL and word in abi.last_error()
    rc = abi.lib().rt_render_soft(tr._ctx, ctypes.byref(s_abi), ctypes.byref(cam), 0, H, depth, 2, A, R, None, None,
                                  None, None)
    assert rc == abi.RT_EINVAL and "size" in abi.last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all(), "a rejected call wrote pixels"
    assert _call_dev(tr, cam, out, W, H, 2, A, R) == abi.RT_OK      # the same buffer with good arguments
    torch.cuda.synchronize()
    sc.assert_same_bits(out.cpu().numpy(), so.expected("c2", W, H, 2, A, R)["rgb"], "after the errors")
