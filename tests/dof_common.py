"""Depth of field (rt_render_dof_dev): the contract of include/rt_api.h restated with numpy on rays traced by the CPU
oracle, shared by tests/test_dof_oracle.py, tests/test_gpu_dof.py and tests/golden/make_golden_dof.py.

Sample (a, b) of pixel (i, j) is the ray from the lens point e(a, b) = (eye + (A t_a) right) + (A t_b) up',
t_a = (2 a + 1 - S) / S, to the primary-ray end point sp_s(S i + a, S j + b) of the sample-grid camera
(rt_camera_supersample); its colour and counters are po.trace_rays' (the oracle's rayTraceRay on an arbitrary ray);
the S x S samples are reduced by ssaa_common.reduce_tree / reduce_counts.  Nothing here calls the code under test
except rt_camera_supersample (host only), which test_ssaa_oracle.py checks field by field; the focused camera is
computed here with numpy (test_dof_oracle.py checks rt_camera_focus against it).
"""
import functools
import os

import numpy as np

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes

from . import ssaa_common as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dof.npz")

# The committed fixtures (tests/golden/dof.npz, from the reference build): (scene, S), all 38 x 22 at pitch 500 / 38,
# aperture 8.
FIX_W, FIX_H, FIX_A = sc.FIX_W, sc.FIX_H, 8.0
FIXTURES = [("c2", 2), ("c2", 4), ("c5", 2), ("demo", 8), ("tree_demo", 2), ("tree_c2", 2)]


def fixtures():
    return dict(np.load(GOLDEN))


def focus_numpy(cam, ratio):
    """Rule 6 of the contract with numpy float64: look_at' = eye + ratio (look_at - eye), pitch' = ratio pitch;
    ratio 1.0 is a copy."""
    out = abi.rt_camera()
    out.eye[:], out.look_at[:], out.up[:] = cam.eye[:], cam.look_at[:], cam.up[:]
    out.pitch, out.bottom_x, out.bottom_y = cam.pitch, cam.bottom_x, cam.bottom_y
    if ratio != 1.0:
        eye, look = np.array(cam.eye[:], np.float64), np.array(cam.look_at[:], np.float64)
        out.look_at[:] = list(eye + np.float64(ratio) * (look - eye))
        out.pitch = float(np.float64(ratio) * np.float64(cam.pitch))
    return out


def rays(cam, W, H, S, A):
    """-> (starts, ends), each [S H, S W, 3] float64: the lens rays of a W x H frame of `cam` in sample-grid order."""
    cam_s = sc.camera_ss(cam, S)
    ends = po.screen_points(cam_s, S * W, S * H)
    right, upp = po.camera_basis(cam_s)
    eye = np.array(cam_s.eye[:], np.float64)
    A = np.float64(A)
    ta = (2 * (np.arange(S * W) % S) + 1 - S).astype(np.float64) / np.float64(S)
    tb = (2 * (np.arange(S * H) % S) + 1 - S).astype(np.float64) / np.float64(S)
    starts = (eye[None, None, :] + (A * ta)[None, :, None] * right[None, None, :]) \
        + (A * tb)[:, None, None] * upp[None, None, :]
    return np.ascontiguousarray(np.broadcast_to(starts, ends.shape)), np.ascontiguousarray(ends)


def render(scene, cam, W, H, depth, S, A):
    """The oracle route on any scenes.Scene and camera -> dict(hi, hi_rc, rgb, rc2)."""
    starts, ends = rays(cam, W, H, S, A)
    rgb, rc = po.trace_rays(scene.to_abi(), starts.reshape(-1, 3), ends.reshape(-1, 3), depth)
    hi, hi_rc = rgb.reshape(S * H, S * W, 3), rc.reshape(S * H, S * W)
    return {"hi": hi, "hi_rc": hi_rc, "rgb": sc.reduce_tree(hi, S), "rc2": sc.reduce_counts(hi_rc, S)}


def render_ref(scene, cam, W, H, depth, S, A):
    """The same rays through the reference's compiled rayTraceRay (po.ref_trace_rays) -> rgb [H, W, 3]."""
    starts, ends = rays(cam, W, H, S, A)
    rgb = po.ref_trace_rays(scene, starts.reshape(-1, 3), ends.reshape(-1, 3), depth)
    return sc.reduce_tree(rgb.reshape(S * H, S * W, 3), S)


@functools.lru_cache(maxsize=None)
def expected(name, W, H, S, A, ratio=1.0):
    """Computed once per case: the camera of a W x H frame at pitch 500 / W, focused at `ratio`.
    -> dict(hi, hi_rc, rgb, rc2, cam, depth); treat as read-only."""
    scene, depth = sc.scene_of(name)
    cam = focus_numpy(scenes.make_camera(W, H, 500.0 / W), ratio)
    out = render(scene, cam, W, H, depth, S, A)
    for a in out.values():
        a.setflags(write=False)
    out["cam"], out["depth"] = cam, depth
    return out


def differ(a, b):
    """Pixels [H, W] whose values differ in some channel (NaN against NaN counts as equal)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        both_nan = np.isnan(a) & np.isnan(b)
        return ((a != b) & ~both_nan).any(axis=2)
    return (a != b).any(axis=2)
