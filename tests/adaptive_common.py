"""Adaptive supersampling (rt_render_adaptive_dev): the contract of include/rt_api.h restated with numpy on frames
of the CPU oracle, shared by tests/test_adaptive_oracle.py, tests/test_gpu_adaptive.py and
tests/golden/make_golden_adaptive.py.

The base frame is po.render at the output size; the supersampled frame is ssaa_common.expected; a pixel is refined
iff the base RGBA8 (ssaa_common.to_rgba8) differs from an in-frame 4-neighbour's by more than T in some colour
channel; the result takes the supersampled value where refined and the base value elsewhere.  Nothing here calls
the code under test (ssaa_common.expected uses rt_camera_supersample, host only, which test_ssaa_oracle.py checks).
"""
import functools
import os

import numpy as np

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import scenes

from . import ssaa_common as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adaptive.npz")

# The committed fixtures (tests/golden/adaptive.npz, from the reference build): (scene, S) at 38 x 22, pitch 500 / 38,
# threshold 32.
FIX_W, FIX_H, FIX_T = sc.FIX_W, sc.FIX_H, 32
FIXTURES = [("c2", 2), ("demo", 4), ("tree_c2", 2)]


def fixtures():
    return dict(np.load(GOLDEN))


def refine_mask(rgba8, T):
    """The criterion: rgba8 [H, W, 4] uint8 (the base frame's bytes) -> bool [H, W]."""
    q = rgba8[..., :3].astype(np.int32)
    m = np.zeros(q.shape[:2], bool)
    dx = (np.abs(q[:, 1:] - q[:, :-1]) > T).any(axis=2)     # pixel (i, j) against (i + 1, j)
    m[:, 1:] |= dx
    m[:, :-1] |= dx
    dy = (np.abs(q[1:] - q[:-1]) > T).any(axis=2)           # pixel (i, j) against (i, j + 1)
    m[1:] |= dy
    m[:-1] |= dy
    return m


def combine(base, base_rc, ss, ss_rc2, T):
    """base [H, W, 3] float64 and its packed counters [H, W]; ss [H, W, 3] and its two-word counters [H, W, 2]
    -> (rgb [H, W, 3], rc2 [H, W, 2] uint32, mask bool [H, W])."""
    mask = refine_mask(sc.to_rgba8(base), T)
    rgb = np.where(mask[..., None], ss, base)
    rc2 = np.where(mask[..., None], ss_rc2, sc.reduce_counts(base_rc, 1))
    return rgb, rc2.astype(np.uint32), mask


@functools.lru_cache(maxsize=None)
def base_frame(name, W, H):
    """The oracle's one-sample frame at pitch 500 / W -> (rgb, packed counters, cam); read-only."""
    scene, depth = sc.scene_of(name)
    cam = scenes.make_camera(W, H, 500.0 / W)
    rgb, rc = po.render(scene.to_abi(), cam, W, H, depth)
    rgb.setflags(write=False)
    rc.setflags(write=False)
    return rgb, rc, cam


@functools.lru_cache(maxsize=None)
def expected(name, W, H, S, T):
    """-> dict(rgb, rc2, mask, base, ss, cam, depth) of the adaptive render; treat as read-only."""
    base, base_rc, cam = base_frame(name, W, H)
    e = sc.expected(name, W, H, S)
    rgb, rc2, mask = combine(base, base_rc, e["rgb"], e["rc2"], T)
    out = {"rgb": rgb, "rc2": rc2, "mask": mask, "base": base, "ss": e["rgb"]}
    for a in out.values():
        a.setflags(write=False)
    out["cam"], out["depth"] = cam, e["depth"]
    return out


def differ(a, b):
    """Pixels [H, W] whose float64 colours differ in their bits (NaN against NaN counts as equal)."""
    both_nan = np.isnan(a) & np.isnan(b)
    bits = np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)
    return (bits & ~both_nan).any(axis=2)
