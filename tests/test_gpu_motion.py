"""GPU: motion blur (rt_set_motion, rt_render_motion_dev / rt_render_motion, Tracer.render_motion, the CLI) against
the contract of include/rt_api.h evaluated on rays traced by the CPU oracle in scenes with displaced spheres
(tests/motion_common.py) and against the fixtures made from the reference build (tests/golden/motion.npz, soft.npz,
dof.npz, ssaa.npz).  Expected values never come from the code under test.

Float images are compared bit for bit (NaNs by position: their sign and payload are unspecified); byte images and
ray counters exactly.  Frames are 37 x 21 at pitch 500 / 37 unless said: partial 8 x 8 sample tiles in both axes at
S = 2 and S = 4, one pixel per wave at S = 8.  tests/test_motion_oracle.py shows that the motions used here change
these frames, and that the three discriminating frames cannot be rendered by a kernel that moves the spheres for
primary rays only or keeps the filter records of the stored centres.
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
from . import motion_common as mc  # noqa: E402
from . import soft_common as so  # noqa: E402
from . import ssaa_common as sc  # noqa: E402
from .lens_gpu_common import BAD, H, OUTS, W, _check_all, _host, _read_ppm, fresh, tr  # noqa: E402,F401

pytestmark = pytest.mark.gpu

A, R, F = 8.0, 40.0, 1.0
MOVES = mc.MOVES


def _render(t, cam, w, h, depth, S, aperture, light_size, shutter):
    return _host(t.render_motion(cam, w, h, depth, S, aperture, light_size, shutter, rgba32f=True, rgba8=True,
                                 rgb64f=True, raycount=True))


def _scene_run(t, scene, cam, w, h, depth, S, aperture, light_size, shutter, d, what):
    """Oracle route and GPU render of any scene, compared."""
    e = mc.render(scene, cam, w, h, depth, S, aperture, light_size, shutter, d)
    t.set_scene(scene)
    t.set_motion(d)
    _check_all(_render(t, cam, w, h, depth, S, aperture, light_size, shutter), e["rgb"], e["rc2"], what)
    return e


# 1. every instance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_variants(tr, name, S):
    """c2 depth 1 and c5 depth 3 (64 spheres, two lights, a moving sphere at index 40): the opaque instance; demo
    depth 5: the FULL one; tree_demo depth 5: the ray-tree one.  Horizontal (and oblique) motion, A = R = 0."""
    e = mc.expected(name, W, H, S, 0.0, 0.0, F, MOVES[name])
    assert not np.isnan(e["rgb"]).any()
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    tr.set_motion(e["d"])
    _check_all(_render(tr, e["cam"], W, H, depth, S, 0.0, 0.0, F), e["rgb"], e["rc2"], f"{name} S={S}")


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_lens_light_and_time_together(tr, name, S):
    e = mc.expected(name, W, H, S, A, R, 0.75, MOVES[name])
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    tr.set_motion(e["d"])
    _check_all(_render(tr, e["cam"], W, H, depth, S, A, R, 0.75), e["rgb"], e["rc2"], f"{name} S={S} A R F")


# 2. the frames a kernel that moves only some uses of the centre cannot pass --------------------------------------
@pytest.mark.parametrize("case", [mc.shadow_only_case, mc.reflection_only_case, mc.fast_small_case])
def test_discriminating_frames(tr, case):
    scene, depth, S, shutter, moves = case()
    cam = scenes.make_camera(W, H, 500.0 / W)
    d = mc.displacement(scene, moves)
    e = _scene_run(tr, scene, cam, W, H, depth, S, 0.0, 0.0, shutter, d, case.__name__)
    e0 = _scene_run(tr, scene, cam, W, H, depth, S, 0.0, 0.0, 0.0, d, case.__name__ + " frozen")
    assert dc.differ(sc.to_rgba8(e["rgb"]), sc.to_rgba8(e0["rgb"])).sum() >= 10


# 3. the fixtures from the reference build ----------------------------------------------------------------------
@pytest.mark.parametrize("key,name,S,Ff,Af,Rf,lights,moves", mc.FIXTURES)
def test_motion_fixtures(tr, key, name, S, Ff, Af, Rf, lights, moves):
    want = mc.fixtures()[key]
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene if lights is None else so.scene_abi(scene, lights))
    tr.set_motion(mc.displacement(scene, moves))
    cam = scenes.make_camera(mc.FIX_W, mc.FIX_H, 500.0 / mc.FIX_W)
    got = _host(tr.render_motion(cam, mc.FIX_W, mc.FIX_H, depth, S, Af, Rf, Ff, rgba32f=False, rgb64f=True))
    sc.assert_same_bits(got["rgb64f"], want, key)


@pytest.mark.parametrize("how", ["shutter 0", "d = 0", "no motion set"])
@pytest.mark.parametrize("name,S,Rf,Af,centres", so.FIXTURES)
def test_frozen_is_the_soft_fixture(tr, name, S, Rf, Af, centres, how):
    """F = 0, all d = 0 and a context without motion run the same kernel as any other frame."""
    want = so.fixtures()[so.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(so.scene_abi(scene, centres))
    tr.set_motion({"shutter 0": mc.displacement(scene, MOVES[name]), "d = 0": mc.displacement(scene, ()),
                   "no motion set": None}[how])
    cam = scenes.make_camera(so.FIX_W, so.FIX_H, 500.0 / so.FIX_W)
    got = _host(tr.render_motion(cam, so.FIX_W, so.FIX_H, depth, S, Af, Rf, 0.0 if how == "shutter 0" else 1.0,
                                 rgba32f=False, rgb64f=True, raycount=True))
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S} {how}")
    assert np.array_equal(got["raycount"], so.expected(name, so.FIX_W, so.FIX_H, S, Af, Rf, centres)["rc2"])


@pytest.mark.parametrize("name,S", dc.FIXTURES)
def test_frozen_without_panels_is_the_dof_fixture(tr, name, S):
    want = dc.fixtures()[sc.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    tr.set_motion(mc.displacement(scene, MOVES[name]))
    cam = scenes.make_camera(dc.FIX_W, dc.FIX_H, 500.0 / dc.FIX_W)
    got = _host(tr.render_motion(cam, dc.FIX_W, dc.FIX_H, depth, S, dc.FIX_A, 0.0, 0.0, rgba32f=False, rgb64f=True,
                                 raycount=True))
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S}")
    assert np.array_equal(got["raycount"], dc.expected(name, dc.FIX_W, dc.FIX_H, S, dc.FIX_A)["rc2"])


@pytest.mark.parametrize("name,S", sc.FIXTURES)
def test_frozen_pinhole_is_the_ssaa_fixture(tr, name, S):
    want = sc.fixtures()[sc.fixture_key(name, S)]
    scene, depth = sc.scene_of(name)
    tr.set_scene(scene)
    tr.set_motion(None)
    cam = scenes.make_camera(sc.FIX_W, sc.FIX_H, 500.0 / sc.FIX_W)
    got = _host(tr.render_motion(cam, sc.FIX_W, sc.FIX_H, depth, S, 0.0, 0.0, 1.0, rgba32f=False, rgb64f=True,
                                 raycount=True))
    sc.assert_same_bits(got["rgb64f"], want, f"{name} S={S}")
    assert np.array_equal(got["raycount"], sc.expected(name, sc.FIX_W, sc.FIX_H, S)["rc2"])


# 4. S = 1 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_one_sample_is_the_plain_render(tr, name):
    lg.check_one_sample_is_the_plain_render(tr, name, lambda cam, depth: _render(tr, cam, W, H, depth, 1, A, R, F),
                                            lambda scene: tr.set_motion(mc.displacement(scene, MOVES[name])))


# 5. sphere counts: one batch, the padding, a second batch, the >= 16 path, an index >= 64 ------------------------
def _grid_scene(n):
    """n spheres of radius 12 on the squares of the board in row-major order, at three heights."""
    sph = [scenes.SphereSpec(chr(ord("a") + (k // 8) % 8) + chr(ord("1") + k % 8), 12.0,
                             float((k % 3) * 20 + 45 * (k // 64))) for k in range(n)]
    return scenes.Scene(spheres=sph, lights=[scenes.LightSpec("b6", scenes.WHITE), scenes.LightSpec("g3", scenes.GREY)])


@pytest.mark.parametrize("n,movers", [(1, (0,)), (3, (2,)), (4, (3, 0)), (5, (4, 1)), (17, (16, 3)), (70, (66, 9))])
def test_sphere_counts(tr, n, movers):
    scene = _grid_scene(n)
    d = mc.displacement(scene, tuple((k, (35.0, 6.0 * (i + 1), -20.0)) for i, k in enumerate(movers)))
    cam = scenes.make_camera(W, H, 500.0 / W)
    e = _scene_run(tr, scene, cam, W, H, 2, 2, 0.0, 0.0, F, d, f"{n} spheres")
    e0 = mc.render(scene, cam, W, H, 2, 2, 0.0, 0.0, 0.0, d)
    assert dc.differ(e["rgb"], e0["rgb"]).any(), "the motion is not visible"


# 6. swept extents --------------------------------------------------------------------------------------------
def test_sphere_leaves_the_bounding_sphere(tr):
    """c2's sphere on h8 moves 400 outwards: past R - 1 of the bound centre (the swept hits_inside proof must fail,
    and rays from hit points out there take the cull test) and past R itself (the reference culls it there)."""
    scene, depth = sc.scene_of("c2")
    d = mc.displacement(scene, ((3, (300.0, 0.0, -265.0)),))
    out = [np.linalg.norm(mc.displaced_centres(scene, d, 4, F, a, b)[3]) for b in range(4) for a in range(4)]
    bound = scene.to_abi().radius                        # (scene-local centres are relative to the bound centre)
    assert min(out) < bound - 21.0 and max(out) > bound + 20.0 and any(bound - 21.0 < v < bound + 20.0 for v in out)
    cam = scenes.make_camera(W, H, 500.0 / W)
    e = _scene_run(tr, scene, cam, W, H, depth, 4, 0.0, 0.0, F, d, "leaving the bound")
    e0 = mc.render(scene, cam, W, H, depth, 4, 0.0, 0.0, 0.0, d)
    assert dc.differ(e["rgb"], e0["rgb"]).any()


def test_sphere_sweeps_through_the_board(tr):
    scene, depth = sc.scene_of("c2")
    d = mc.displacement(scene, ((4, (0.0, 70.0, 0.0)), (1, (20.0, -90.0, 0.0))))
    cam = scenes.make_camera(W, H, 500.0 / W)
    _scene_run(tr, scene, cam, W, H, depth, 4, 0.0, 0.0, F, d, "through the board")


def test_sweep_contains_a_light(tr):
    """The light above b6 stands at (60, 200, -60) in world coordinates; a sphere of radius 30 on c6, world
    (60, 60, -100), moving by (0, 150, 45) rises over it: the light is inside the sphere at its last times only."""
    scene = scenes.Scene(spheres=[scenes.SphereSpec("c6", 30.0), scenes.SphereSpec("e3", 20.0)],
                         lights=[scenes.LightSpec("b6", scenes.WHITE)])
    light = np.array(scene.lights[0].position())
    d = mc.displacement(scene, ((0, (0.0, 150.0, 45.0)),))
    inside = [np.linalg.norm(mc.world_centres(scene, mc.displaced_centres(scene, d, 4, F, a, b))[0] - light) < 30.0
              for b in range(4) for a in range(4)]
    assert any(inside) and not all(inside)
    cam = scenes.make_camera(W, H, 500.0 / W)
    _scene_run(tr, scene, cam, W, H, 1, 4, 0.0, 0.0, F, d, "light inside the sweep")


def test_empty_scene(tr):
    scene = scenes.Scene(spheres=[], lights=[scenes.LightSpec("b6", scenes.WHITE)])
    cam = scenes.make_camera(W, H, 500.0 / W)
    e = mc.render(scene, cam, W, H, 1, 2, 0.0, R, F, np.zeros((0, 3)))
    tr.set_scene(scene)
    assert abi.lib().rt_set_motion(tr._ctx, None, 0) == abi.RT_OK
    _check_all(_render(tr, cam, W, H, 1, 2, 0.0, R, F), e["rgb"], e["rc2"], "empty scene")
    tr.set_motion(np.zeros((0, 3)))
    _check_all(_render(tr, cam, W, H, 1, 2, 0.0, R, F), e["rgb"], e["rc2"], "empty scene, empty motion")


# 7. NaN frames -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
def test_nan_frames(tr, S):
    e = mc.expected("tree_c2", W, H, S, 0.0, 0.0, F, MOVES["tree_c2"])
    nan_px = np.isnan(e["rgb"]).any(axis=2)
    assert 0 < nan_px.sum() <= 0.25 * W * H
    scene, depth = sc.scene_of("tree_c2")
    assert depth == 3
    tr.set_scene(scene)
    tr.set_motion(e["d"])
    lg.check_nan_frame(_render(tr, e["cam"], W, H, depth, S, 0.0, 0.0, F), e, S)


# 8. a scene with no lights -----------------------------------------------------------------------------------
def test_no_lights(tr):
    scene, depth = sc.scene_of("c2")
    scene.lights = []
    cam = scenes.make_camera(W, H, 500.0 / W)
    d = mc.displacement(scene, MOVES["c2"])
    e = _scene_run(tr, scene, cam, W, H, depth, 2, 0.0, R, F, d, "no lights")
    assert not e["rgb"].any() and not e["rc2"][..., 1].any() and e["rc2"][..., 0].any()


# 9. the smallest shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (9, 1), (1, 9), (8, 8), (9, 9)])
def test_small_frames(tr, w, h, S):
    """c2 on a w x h frame at pitch 500 / 37 (the camera of that size, not a crop)."""
    scene, depth = sc.scene_of("c2")
    cam = scenes.make_camera(w, h, 500.0 / 37)
    _scene_run(tr, scene, cam, w, h, depth, S, 0.0, 0.0, F, mc.displacement(scene, MOVES["c2"]), f"{w}x{h} S={S}")


# 10. each output alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("only", OUTS)
def test_nullable_outputs(tr, only):
    S = 2
    e = mc.expected("c2", W, H, S, 0.0, 0.0, F, MOVES["c2"])
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    tr.set_motion(e["d"])
    lg.check_nullable_output(only, e,
                             lambda **flags: tr.render_motion(e["cam"], W, H, depth, S, 0.0, 0.0, F, **flags))


def test_no_outputs_is_a_no_op(tr):
    lg.check_no_outputs_is_a_no_op(tr, "rt_render_motion_dev", A, R, F)


# 11. the context's other state ---------------------------------------------------------------------------------
def test_no_side_effect(fresh):
    """A view's first, calibration and cached renders and a soft-shadow frame; then motion frames of two motions and
    another eye; then the view and the soft frame again: the scene record and the per-view state must still be what
    they were."""
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    frames = lg.view_frames(fresh, scene, cam, depth)
    soft = _host(fresh.render_soft(cam, W, H, depth, 2, A, R, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
    sc.assert_same_bits(soft["rgb64f"], so.expected("c2", W, H, 2, A, R)["rgb"], "soft frame")
    other = scenes.make_camera(W, H, 500.0 / W)
    other.eye[0] += 40.0
    other.eye[1] += 25.0
    for c, S, moves in ((cam, 2, MOVES["c2"]), (other, 4, ((7, (0.0, 30.0, 40.0)),)), (other, 2, ())):
        d = mc.displacement(scene, moves)
        fresh.set_motion(d)
        e = mc.render(scene, c, W, H, depth, S, A, R, F, d)
        _check_all(_render(fresh, c, W, H, depth, S, A, R, F), e["rgb"], e["rc2"], f"S={S} {moves}")
    fresh.set_motion(mc.displacement(scene, MOVES["c2"]))                            # left set: others ignore it
    lg.check_view_unchanged(frames, _host(fresh.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True,
                                                       raycount=True)))
    again = _host(fresh.render_soft(cam, W, H, depth, 2, A, R, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
    for key in OUTS:
        assert again[key].tobytes() == soft[key].tobytes(), key


def test_set_scene_clears_the_motion(fresh):
    """An identical scene keeps the motion; a changed one clears it (and the cleared frame is the soft frame)."""
    scene, depth = sc.scene_of("c2")
    e = mc.expected("c2", W, H, 2, 0.0, 0.0, F, MOVES["c2"])
    e0 = so.expected("c2", W, H, 2, 0.0, 0.0)
    assert dc.differ(e["rgb"], e0["rgb"]).any()
    fresh.set_scene(scene)
    fresh.set_motion(e["d"])
    fresh.set_scene(sc.scene_of("c2")[0])                                            # the same scene again
    _check_all(_render(fresh, e["cam"], W, H, depth, 2, 0.0, 0.0, F), e["rgb"], e["rc2"], "kept")
    fresh.set_scene(sc.scene_of("c5")[0])
    fresh.set_scene(scene)
    _check_all(_render(fresh, e["cam"], W, H, depth, 2, 0.0, 0.0, F), e0["rgb"], e0["rc2"], "cleared")
    fresh.set_motion(e["d"])
    fresh.set_motion(None)
    _check_all(_render(fresh, e["cam"], W, H, depth, 2, 0.0, 0.0, F), e0["rgb"], e0["rc2"], "cleared by (NULL, 0)")


# 12. hipGraph capture ----------------------------------------------------------------------------------------
def test_graph_capture(fresh):
    S = 2
    e = mc.expected("c2", W, H, S, 0.0, 0.0, F, MOVES["c2"])
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    fresh.set_motion(e["d"])
    lg.check_graph_capture(fresh, e, depth, lambda bufs, s: fresh.render_motion_into(e["cam"], W, H, depth, S, 0.0, 0.0,
                                                                                     F, bufs, stream=s))


# 13. rt_render_motion: host buffers and the CLI ----------------------------------------------------------------
def test_render_motion_host_buffers(tr):
    S = 4
    e = mc.expected("c2", W, H, S, 0.0, 0.0, F, MOVES["c2"])
    scene, depth = sc.scene_of("c2")
    s_abi = scene.to_abi()
    d = np.ascontiguousarray(e["d"])
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f64 = lg.check_host_buffers(e, S, "rt_render_motion", lambda *out: abi.lib().rt_render_motion(
        tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(e["cam"]), W, H, depth, S, 0.0, 0.0, F, *out))
    # every pointer optional; no displacement: the frozen frame
    abi.check(abi.lib().rt_render_motion(tr._ctx, ctypes.byref(s_abi), None, ctypes.byref(e["cam"]), W, H, depth, S,
                                         0.0, 0.0, F, None, None, ctypes.c_void_p(f64.ctypes.data), None),
              "rt_render_motion")
    sc.assert_same_bits(f64, so.expected("c2", W, H, S, 0.0, 0.0)["rgb"], "rt_render_motion without displacement")


@pytest.mark.parametrize("extra", [None, "panel and lens"])
def test_cli(tmp_path, extra):
    ap, ls = (0.0, 0.0) if extra is None else (8.0, 40.0)
    e = mc.expected("c2", W, H, 2, ap, ls, 0.5, MOVES["c2"])
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c2_motion.ppm"
    args = [exe, "--config", "c2", "--width", str(W), "--height", str(H), "--samples", "2", "--shutter", "0.5",
            "--move", "4:50,0,0", "--move", "0:0,12,-30", "--out", str(out)]
    args += [] if extra is None else ["--aperture", "8", "--light-size", "40"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if "motion blur" in ln]
    assert len(line) == 1 and f"{W * H * 4} primary rays" in line[0] and "2 moving spheres" in line[0], r.stdout
    assert np.array_equal(_read_ppm(out), sc.to_rgba8(e["rgb"])[::-1, :, :3])     # PPM rows run top to bottom


# 14. argument errors -----------------------------------------------------------------------------------------
def _call_dev(t, cam, out, w, h, S, aperture, light_size, shutter):
    return abi.lib().rt_render_motion_dev(t._ctx, ctypes.byref(cam), w, h, 1, S, aperture, light_size, shutter, None,
                                          None, ctypes.c_void_p(out.data_ptr()), None, lg.stream_ptr())


def test_argument_errors(tr):
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    e = mc.expected("c2", W, H, 2, A, R, F, MOVES["c2"])
    tr.set_motion(e["d"])
    cam = scenes.make_camera(W, H, 500.0 / W)
    bufs = tr.alloc_ss(W, H, None, rgba32f=False, rgb64f=True)
    out = bufs["rgb64f"]
    out.fill_(-7.0)
    L = abi.lib()
    for S in (0, 3, 16, -2):
        assert _call_dev(tr, cam, out, W, H, S, A, R, F) == abi.RT_EINVAL and "samples" in abi.last_error()
        with pytest.raises(abi.RtError) as ei:
            tr.render_motion_into(cam, W, H, depth, S, A, R, F, bufs)
        assert ei.value.code == abi.RT_EINVAL and "samples" in str(ei.value)
    for ap in BAD:
        assert _call_dev(tr, cam, out, W, H, 2, ap, R, F) == abi.RT_EINVAL and "aperture" in abi.last_error(), ap
    for ls in BAD:
        assert _call_dev(tr, cam, out, W, H, 2, A, ls, F) == abi.RT_EINVAL and "light_size" in abi.last_error(), ls
    for sh in BAD + (1.0000000000000002, 2.0):
        assert _call_dev(tr, cam, out, W, H, 2, A, R, sh) == abi.RT_EINVAL and "shutter" in abi.last_error(), sh
        with pytest.raises(abi.RtError) as ei:
            tr.render_motion_into(cam, W, H, depth, 2, A, R, sh, bufs)
        assert ei.value.code == abi.RT_EINVAL and "shutter" in str(ei.value)
    for w, h in ((0, H), (W, 0), (-1, H), (W, -5), (65536, 65536), (2 ** 30, 1)):
        assert _call_dev(tr, cam, out, w, h, 8, A, R, F) == abi.RT_EINVAL and "size" in abi.last_error(), (w, h)
    far = scenes.make_camera(W, H, 500.0 / W)
    far.bottom_x = -(2 ** 30) - 1
    assert _call_dev(tr, far, out, W, H, 2, A, R, F) == abi.RT_EINVAL and "overflow" in abi.last_error()
    # rt_set_motion: a wrong sphere count, a null array with a count, a non-finite displacement; the motion in force
    # stays
    d9 = np.zeros((9, 3))
    dptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))          # noqa: E731
    assert L.rt_set_motion(tr._ctx, dptr(d9), 9) == abi.RT_EINVAL and "n_spheres" in abi.last_error()
    assert L.rt_set_motion(tr._ctx, dptr(d9), 7) == abi.RT_EINVAL and "n_spheres" in abi.last_error()
    assert L.rt_set_motion(tr._ctx, dptr(d9), 0) == abi.RT_EINVAL and "n_spheres" in abi.last_error()
    assert L.rt_set_motion(tr._ctx, None, 8) == abi.RT_EINVAL and "displacement" in abi.last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        d8 = np.zeros((8, 3))
        d8[5, 1] = bad
        assert L.rt_set_motion(tr._ctx, dptr(d8), 8) == abi.RT_EINVAL and "displacement" in abi.last_error(), bad
        with pytest.raises(abi.RtError):
            tr.set_motion(d8)
    s_abi = scene.to_abi()
    dgood = np.ascontiguousarray(e["d"])
    for S, ap, ls, sh, dd, word in ((3, A, R, F, dgood, "samples"), (2, -1.0, R, F, dgood, "aperture"),
                                    (2, A, -1.0, F, dgood, "light_size"), (2, A, R, 1.5, dgood, "shutter"),
                                    (2, A, R, float("nan"), dgood, "shutter"), (2, A, R, F, d8, "displacement")):
        rc = L.rt_render_motion(tr._ctx, ctypes.byref(s_abi), dptr(dd), ctypes.byref(cam), W, H, depth, S, ap, ls, sh,
                                None, None, None, None)
        assert rc == abi.RT_EINVAL and word in abi.last_error(), word
    rc = L.rt_render_motion(tr._ctx, ctypes.byref(s_abi), dptr(dgood), ctypes.byref(cam), 0, H, depth, 2, A, R, F, None,
                            None, None, None)
    assert rc == abi.RT_EINVAL and "size" in abi.last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all(), "a rejected call wrote pixels"
    assert _call_dev(tr, cam, out, W, H, 2, A, R, F) == abi.RT_OK      # the same buffer, good arguments, the motion kept
    torch.cuda.synchronize()
    sc.assert_same_bits(out.cpu().numpy(), e["rgb"], "after the errors")
