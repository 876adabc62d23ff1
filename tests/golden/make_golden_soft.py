#!/usr/bin/env python3
"""Generate tests/golden/soft.npz: soft-shadow frames from the REFERENCE's own compiled rayTraceRay.

Each case builds the samples of include/rt_api.h (tests/soft_common.py render_ref): the lens rays of sample (a, b)
traced with po.ref_trace_rays (oracle/_ref/libref.so, see make_golden.py) in the scene whose lights sit at point (a, b)
of their panels, reduced by the pairwise tree (tests/ssaa_common.py reduce_tree).  The reference harness places lights
by board square: the cases centre every panel on a corner of four squares with R = 20 S, so every panel point is the
centre of a square.

All cases are 38 x 22 at pitch 500 / 38 (soft_common.FIXTURES); each stores the expected rgb64f [22, 38, 3] as
<scene>_s<S>.  Data only.

Run where the reference build exists (oracle/_ref/libref.so):  python tests/golden/make_golden_soft.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import pyoracle as po  # noqa: E402
from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from tests import soft_common as so  # noqa: E402
from tests import ssaa_common as sc  # noqa: E402


def main() -> None:
    po.build(ref=True)
    W, H = so.FIX_W, so.FIX_H
    out = {}
    for name, S, R, A, centres in so.FIXTURES:
        scene, depth = sc.scene_of(name)
        cam = scenes.make_camera(W, H, 500.0 / W)
        rgb = so.render_ref(scene, cam, W, H, depth, S, A, R, centres)
        out[so.fixture_key(name, S)] = rgb
        print(f"{name} S={S} R={R} A={A} depth {depth}: {int(np.isnan(rgb).any(axis=2).sum())} NaN pixels", flush=True)
    np.savez_compressed(so.GOLDEN, **out)
    print(f"wrote {so.GOLDEN}: {os.path.getsize(so.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
