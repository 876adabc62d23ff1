"""CPU: the shutter render's contract (include/rt_api.h: camera motion blur) on the oracle.  The symbols;
rt_camera_at (host only) against the numpy camera of tests/shutter_common.py; the zero-motion and F = 0 pins and the
plain-render pin on the numpy restatement; the fixtures made from the reference build (tests/golden/shutter.npz); the
conditions that make each case of tests/test_gpu_shutter.py discriminating; and the CLI's usage errors.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes

from . import dof_common as dc
from . import jitter_common as jc
from . import motion_common as mc
from . import shutter_common as hc
from . import ssaa_common as sc
from .test_jitter_oracle import SHAPES

W, H = 19, 11                                # the GPU tests' frame at S = 2: a 38 x 22 sample frame
A, R, F = 8.0, 40.0, 1.0
NAMED = ("dolly", "pan", "crane")
# the eye of test_gpu_shutter.py's swept-bound case: it leaves the range in which hits_ok holds (about 0.93e8 from the
# board for c2, rt_host.cpp hits_limit) on both sides of the exposure's middle: inside for |sigma| < 0.46
FAR_EYE = ((0.0, 2e8, 0.0), (0.0, 0.0, 0.0))


def _bits(cam):
    return bytes(cam)


def test_symbols_and_signatures():
    for name, n in (("rt_camera_at", 4), ("rt_render_shutter_dev", 17), ("rt_render_shutter", 18)):
        assert name in abi.SIGNATURES and len(abi.SIGNATURES[name][1]) == n and hasattr(abi.lib(), name)
    assert abi.lib().rt_abi_version() == 10
    assert ctypes.sizeof(abi.rt_camera_motion) == 6 * 8


@pytest.mark.parametrize("name", NAMED)
def test_camera_at_is_the_numpy_camera(name):
    L = abi.lib()
    cam = scenes.make_camera(W, H, 500.0 / W)
    cam.eye[0], cam.look_at[1] = 0.1, -0.3               # inexact sums
    m = hc.motion_abi(hc.MOTIONS[name])
    sigmas = [0.0, 1.0, -1.0, 0.75, -1.0 / 3.0, 1e-300, 0.1]
    sigmas += jc.samples(cam, 3, 2, 2, 16, 5, A, R, 0.7)["sigma"].reshape(-1).tolist()      # the times of a real frame
    for sg in sigmas:
        out = abi.rt_camera()
        assert L.rt_camera_at(ctypes.byref(cam), ctypes.byref(m), sg, ctypes.byref(out)) == abi.RT_OK
        assert _bits(out) == _bits(hc.camera_at(cam, hc.MOTIONS[name], sg)), (name, sg)
        assert _bits(scenes.camera_at(cam, m, sg)) == _bits(out)
    # sigma = 0 and a null motion: the camera itself (no -0.0 component here)
    for mo in (ctypes.byref(m), None):
        out = abi.rt_camera()
        assert L.rt_camera_at(ctypes.byref(cam), mo, 0.0 if mo else 0.5, ctypes.byref(out)) == abi.RT_OK
        assert _bits(out) == _bits(cam)
    # out == cam
    want = hc.camera_at(cam, hc.MOTIONS[name], 0.625)
    assert L.rt_camera_at(ctypes.byref(cam), ctypes.byref(m), 0.625, ctypes.byref(cam)) == abi.RT_OK
    assert _bits(cam) == _bits(want)


def test_camera_motion_helper():
    m = scenes.camera_motion(eye=(1.0, 2.0, 3.0), look_at=(4.0, 5.0, 6.0))
    assert list(m.eye) == [1.0, 2.0, 3.0] and list(m.look_at) == [4.0, 5.0, 6.0]
    z = scenes.camera_motion()
    assert list(z.eye) == [0.0] * 3 and list(z.look_at) == [0.0] * 3


def test_camera_at_errors():
    L = abi.lib()
    cam, out = scenes.make_camera(W, H, 1.0), abi.rt_camera()
    m = hc.motion_abi(hc.MOTIONS["crane"])
    for sg in (float("nan"), float("inf"), -float("inf")):
        assert L.rt_camera_at(ctypes.byref(cam), ctypes.byref(m), sg, ctypes.byref(out)) == abi.RT_EINVAL
        assert "sigma" in abi.last_error()
    for field, q, v in (("eye", 0, float("nan")), ("eye", 2, float("inf")), ("look_at", 1, -float("inf")),
                        ("look_at", 2, float("nan"))):
        bad = hc.motion_abi(hc.MOTIONS["crane"])
        getattr(bad, field)[q] = v
        assert L.rt_camera_at(ctypes.byref(cam), ctypes.byref(bad), 0.5, ctypes.byref(out)) == abi.RT_EINVAL
        assert "displacement" in abi.last_error()
    assert L.rt_camera_at(None, ctypes.byref(m), 0.5, ctypes.byref(out)) == abi.RT_EINVAL and "null" in abi.last_error()
    assert L.rt_camera_at(ctypes.byref(cam), ctypes.byref(m), 0.5, None) == abi.RT_EINVAL and "null" in abi.last_error()


def test_render_entry_points_reject_before_any_device_work():
    """Rule 7's checks that need no context state come after the context's: without a context the call names it."""
    L = abi.lib()
    cam = scenes.make_camera(W, H, 1.0)
    rc = L.rt_render_shutter_dev(None, ctypes.byref(cam), None, W, H, 1, 2, 4, 1, A, R, F, None, None, None, None, None)
    assert rc == abi.RT_EINVAL and "context" in abi.last_error()
    rc = L.rt_render_shutter(None, None, None, ctypes.byref(cam), None, W, H, 1, 2, 4, 1, A, R, F, None, None, None, None)
    assert rc == abi.RT_EINVAL and "context" in abi.last_error()


# ---- pins on the numpy restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,J", [("c2", 2, 4), ("demo", 2, 1)])
def test_zero_motion_and_closed_shutter_are_the_jittered_render(name, S, J):
    moves = mc.MOVES[name]
    e = jc.expected(name, W, H, S, J, 3, A, R, 0.75, moves)
    z = hc.expected(name, hc.ZERO, W, H, S, J, 3, A, R, 0.75, moves)
    assert z["hi"].tobytes() == e["hi"].tobytes() and np.array_equal(z["hi_rc"], e["hi_rc"])
    e0 = jc.expected(name, W, H, S, J, 3, A, R, 0.0, moves)
    c0 = hc.expected(name, "crane", W, H, S, J, 3, A, R, 0.0, moves)
    assert c0["hi"].tobytes() == e0["hi"].tobytes() and np.array_equal(c0["hi_rc"], e0["hi_rc"])


@pytest.mark.parametrize("name", ["pan", "crane"])
def test_pinhole_samples_are_pixels_of_plain_frames(name):
    """J = 1, A = R = 0, frozen spheres: sample (a, b) of pixel (i, j) is pixel (S i + a, S j + b) of the S W x S H
    frame po.render gives the supersample camera of the camera at sigma_n, n = a + S b."""
    S = 2
    e = hc.expected("c2", name, W, H, S, 1, 0, 0.0, 0.0, F)
    scene, depth = sc.scene_of("c2")
    hi, hi_rc = np.zeros_like(e["hi"]), np.zeros_like(e["hi_rc"])
    for b in range(S):
        for a in range(S):
            cam_n = sc.camera_ss(hc.camera_at(e["cam"], e["motion"], mc.time_of(S, F, a, b)), S)
            rgb, rc = po.render(scene.to_abi(), cam_n, S * W, S * H, depth)
            hi[b::S, a::S], hi_rc[b::S, a::S] = rgb[b::S, a::S], rc[b::S, a::S]
    assert hi.tobytes() == e["hi"].tobytes() and np.array_equal(hi_rc, e["hi_rc"])


@pytest.mark.parametrize("key,name,S,J,seed,Ff,Af,Rf,lights,moves,motion", hc.FIXTURES)
def test_fixtures_are_the_oracle_route(key, name, S, J, seed, Ff, Af, Rf, lights, moves, motion):
    e = hc.expected(name, motion, hc.FIX_W, hc.FIX_H, S, J, seed, Af, Rf, Ff, moves, lights)
    sc.assert_same_bits(hc.fixtures()[key], e["rgb"], key)


@pytest.mark.ref
def test_reference_build_agrees_with_the_oracle_route():
    """One fixture case again through the reference build, where there is one."""
    if not po.ref_available():
        pytest.skip("no reference build here")
    key, name, S, J, seed, Ff, Af, Rf, lights, moves, motion = hc.FIXTURES[1]
    scene, depth = sc.scene_of(name)
    cam = scenes.make_camera(hc.FIX_W, hc.FIX_H, 500.0 / hc.FIX_W)
    rgb = hc.render_ref(scene, cam, hc.MOTIONS[motion], hc.FIX_W, hc.FIX_H, depth, S, J, seed, Af, Rf, Ff,
                        mc.displacement(scene, moves), lights)
    e = hc.expected(name, motion, hc.FIX_W, hc.FIX_H, S, J, seed, Af, Rf, Ff, moves, lights)
    sc.assert_same_bits(rgb, e["rgb"], key)


# ---- the conditions that make the GPU cases discriminating ----------------------------------------------------------
@pytest.mark.parametrize("name", NAMED)
def test_named_motions_show_and_need_the_per_sample_camera(name):
    """The moved frame differs from the frozen one; pan and crane also from the frame with the sigma = 0 basis at the
    moved eye and look_at (a kernel that forgets the per-lane basis), dolly from the frame with only the start moved."""
    e = hc.expected("c2", name, W, H, 2, 4, 1, 0.0, 0.0, F)
    frozen = jc.expected("c2", W, H, 2, 4, 1, 0.0, 0.0, F)
    assert not np.isnan(e["rgb"]).any()
    assert dc.differ(e["rgb"], frozen["rgb"]).sum() >= 0.1 * W * H
    partial = hc.expected("c2", name, W, H, 2, 4, 1, 0.0, 0.0, F, mode="start_only" if name == "dolly" else "frozen_basis")
    assert dc.differ(e["rgb"], partial["rgb"]).sum() >= 10


@pytest.mark.parametrize("S,J,w,h", SHAPES)
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_instance_frames_differ_from_the_frozen_camera(name, S, J, w, h):
    e = hc.expected(name, "crane", w, h, S, J, 1, A, R, F, mc.MOVES[name])
    m = jc.expected(name, w, h, S, J, 1, A, R, F, mc.MOVES[name])
    assert not np.isnan(e["rgb"]).any()
    assert dc.differ(e["rgb"], m["rgb"]).sum() >= 0.1 * w * h


def test_far_eye_crosses_the_hits_ok_limit():
    """The eye of the swept-bound case is inside the limit at some of a wave's times and outside at others
    (rt_diag_flat_gates: hits_ok for an eye, by the expression the device evaluates per lane)."""
    from . import flat_tiles_common as fc
    S, J = 2, 16
    cam = scenes.make_camera(W, H, 500.0 / W)
    sm = hc.samples(cam, FAR_EYE, W, H, S, J, 1, 0.0, 0.0, F)
    ok = np.array([fc.flat_gates("c2", st.tolist())[1] for st in sm["starts"][:8, :8].reshape(-1, 3)])
    assert 8 <= ok.sum() <= 56                           # the first wave's 64 lanes: both kinds


def test_cli_usage_errors(tmp_path):
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    for args, word in ((["--eye-move", "1,2,3"], "--shutter"),
                       (["--look-move", "1,2,3", "--shutter", "1"], "--samples"),
                       (["--samples", "2", "--shutter", "1", "--eye-move", "1,2"], "DX,DY,DZ"),
                       (["--samples", "2", "--shutter", "1", "--look-move", "a,b,c"], "DX,DY,DZ"),
                       (["--samples", "4", "--shutter", "1", "--eye-move", "1,2,3", "--adaptive", "8"], "--adaptive"),
                       (["--samples", "4", "--shutter", "1", "--eye-move", "1,2,3", "--gpus", "2"], "--gpus")):
        r = subprocess.run([exe, "--config", "c2", "--out", str(tmp_path / "x.ppm")] + args, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert ("--eye-move" in r.stderr or "--look-move" in r.stderr) and word in r.stderr, (args, r.stderr)
        assert not (tmp_path / "x.ppm").exists()


def test_nan_frame_has_some_nans():
    e = hc.expected("tree_c2", "crane", W, H, 2, 4, 1, 0.0, 0.0, F, mc.MOVES["tree_c2"])
    nan_px = np.isnan(e["rgb"]).any(axis=2)
    assert 0 < nan_px.sum() <= 0.25 * W * H
