"""Soft shadows (rt_render_soft_dev): the contract of include/rt_api.h restated with numpy on rays traced by the CPU
oracle, shared by tests/test_soft_oracle.py, tests/test_gpu_soft.py and tests/golden/make_golden_soft.py.

Sample (a, b) of pixel (i, j) is the lens ray of dof_common.rays (from e(a, b) to the sample-grid screen point of the
same (a, b)), traced in a copy of the scene whose light i sits at (L_i.x + (R t_a), L_i.y, L_i.z + (R t_b)),
t_a = (2 a + 1 - S) / S: one po.trace_rays call per (a, b) on the sub-lattice [b::S, a::S] of the sample grid; the
S x S samples are reduced by ssaa_common.reduce_tree / reduce_counts.  Nothing here calls the code under test except
rt_camera_supersample (host only, through dof_common.rays).
"""
import dataclasses
import functools
import os

import numpy as np

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import scenes

from . import dof_common as dc
from . import ssaa_common as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft.npz")

# The committed fixtures (tests/golden/soft.npz, from the reference build), all 38 x 22 at pitch 500 / 38:
# (scene, S, R, A, light centres).  Every centre is a corner of four board squares and R = 20 S, so the S x S points
# of a panel are centres of squares (40 apart): each sample's scene is one the reference harness can build.
FIX_W, FIX_H = sc.FIX_W, sc.FIX_H
FIXTURES = [
    ("c2", 2, 40.0, 0.0, ((40.0, 200.0, -40.0),)),
    ("c2", 4, 80.0, 8.0, ((40.0, 200.0, -80.0),)),
    ("c5", 2, 40.0, 0.0, ((40.0, 200.0, -40.0), (-40.0, 200.0, -240.0))),
    ("demo", 8, 160.0, 0.0, ((0.0, 200.0, -160.0),)),
    ("tree_demo", 2, 40.0, 8.0, ((40.0, 200.0, -40.0),)),
    ("tree_c2", 2, 40.0, 0.0, ((40.0, 200.0, -40.0),)),
]


def fixture_key(name, S):
    return sc.fixture_key(name, S)


def fixtures():
    return dict(np.load(GOLDEN))


def centres_of(scene):
    """The scene's own light positions -> [nl, 3] float64."""
    return np.array([lt.position() for lt in scene.lights], np.float64).reshape(-1, 3)


def displaced(centres, S, R, a, b):
    """Rule 2 with numpy float64: the lights sample (a, b) sees, [nl, 3]."""
    c = np.array(centres, np.float64).reshape(-1, 3)
    R = np.float64(R)
    ta = np.float64(2 * a + 1 - S) / np.float64(S)
    tb = np.float64(2 * b + 1 - S) / np.float64(S)
    out = c.copy()
    out[:, 0] = c[:, 0] + (R * ta)
    out[:, 2] = c[:, 2] + (R * tb)
    return out


def scene_abi(scene, lights):
    """scene.to_abi() with its lights at `lights` [nl, 3] (colours unchanged).  `scene` keeps the arrays alive."""
    s = scene.to_abi()
    assert s.n_lights == len(lights)
    for k, p in enumerate(lights):
        for q in range(3):
            s.lights[k].position[q] = float(p[q])
    return s


def square_of_light(p):
    """The board square whose light position (scenes.light_position_from_square) is p, or an error."""
    x, y, z = (float(v) for v in p)
    d, r = (x + 140.0) / 40.0, (-20.0 - z) / 40.0
    assert y == 200.0 and d == int(d) and r == int(r) and 0 <= d < 8 and 0 <= r < 8, p
    sq = chr(ord("a") + int(r)) + chr(ord("1") + int(d))
    assert scenes.light_position_from_square(sq) == (x, y, z), (sq, p)
    return sq


def render(scene, cam, W, H, depth, S, A, R, centres=None):
    """The oracle route on any scenes.Scene and camera -> dict(hi, hi_rc, rgb, rc2); centres: the lights' positions
    (default: the scene's own)."""
    centres = centres_of(scene) if centres is None else np.array(centres, np.float64).reshape(-1, 3)
    starts, ends = dc.rays(cam, W, H, S, A)
    hi = np.zeros((S * H, S * W, 3), np.float64)
    hi_rc = np.zeros((S * H, S * W), np.uint32)
    for b in range(S):
        for a in range(S):
            s_ab = scene_abi(scene, displaced(centres, S, R, a, b))
            st = np.ascontiguousarray(starts[b::S, a::S]).reshape(-1, 3)
            en = np.ascontiguousarray(ends[b::S, a::S]).reshape(-1, 3)
            rgb, rc = po.trace_rays(s_ab, st, en, depth)
            hi[b::S, a::S] = rgb.reshape(H, W, 3)
            hi_rc[b::S, a::S] = rc.reshape(H, W)
    return {"hi": hi, "hi_rc": hi_rc, "rgb": sc.reduce_tree(hi, S), "rc2": sc.reduce_counts(hi_rc, S)}


def render_ref(scene, cam, W, H, depth, S, A, R, centres):
    """The same samples through the reference's compiled rayTraceRay (po.ref_trace_rays) on scenes whose lights the
    reference harness places by square -> rgb [H, W, 3]."""
    starts, ends = dc.rays(cam, W, H, S, A)
    hi = np.zeros((S * H, S * W, 3), np.float64)
    for b in range(S):
        for a in range(S):
            lights = [scenes.LightSpec(square_of_light(p), lt.color)
                      for p, lt in zip(displaced(centres, S, R, a, b), scene.lights)]
            s_ab = dataclasses.replace(scene, lights=lights)
            st = np.ascontiguousarray(starts[b::S, a::S]).reshape(-1, 3)
            en = np.ascontiguousarray(ends[b::S, a::S]).reshape(-1, 3)
            hi[b::S, a::S] = po.ref_trace_rays(s_ab, st, en, depth).reshape(H, W, 3)
    return sc.reduce_tree(hi, S)


@functools.lru_cache(maxsize=None)
def expected(name, W, H, S, A, R, centres=None, depth=None):
    """Computed once per case: the camera of a W x H frame at pitch 500 / W; centres: a tuple of light positions
    (default: the scene's own); depth: default the case's.  -> dict(hi, hi_rc, rgb, rc2, cam, depth); read-only."""
    scene, d = sc.scene_of(name)
    depth = d if depth is None else depth
    cam = scenes.make_camera(W, H, 500.0 / W)
    out = render(scene, cam, W, H, depth, S, A, R, centres)
    for a in out.values():
        a.setflags(write=False)
    out["cam"], out["depth"] = cam, depth
    return out


def shadowed(e):
    """Depth 0, opaque scenes: the samples [S H, S W] that hit something and are in shadow.  The reference adds the
    ambient term only when the light is visible, so a hit sample is shadowed exactly when its colour is 0; a sample
    has a shadow ray exactly when it hit."""
    hit = (e["hi_rc"] >> 16) > 0
    return hit & (e["hi"] == 0.0).all(axis=2)
