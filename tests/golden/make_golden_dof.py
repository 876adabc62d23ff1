#!/usr/bin/env python3
"""Generate tests/golden/dof.npz: depth-of-field frames from the REFERENCE's own compiled rayTraceRay.

Each case builds the lens rays of include/rt_api.h (tests/dof_common.py rays: from e(a, b) on the square lens to the
sample-grid screen point of the same (a, b)), traces them with po.ref_trace_rays (oracle/_ref/libref.so, see
make_golden.py) and reduces them by the pairwise tree (tests/ssaa_common.py reduce_tree).

All cases are 38 x 22 at pitch 500 / 38, aperture 8 (dof_common.FIXTURES); each stores the expected rgb64f
[22, 38, 3] as <scene>_s<S>.  Data only.

Run where the reference build exists (oracle/_ref/libref.so):  python tests/golden/make_golden_dof.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import pyoracle as po  # noqa: E402
from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from tests import dof_common as dc  # noqa: E402
from tests import ssaa_common as sc  # noqa: E402


def main() -> None:
    po.build(ref=True)
    W, H, A = dc.FIX_W, dc.FIX_H, dc.FIX_A
    out = {}
    for name, S in dc.FIXTURES:
        scene, depth = sc.scene_of(name)
        cam = scenes.make_camera(W, H, 500.0 / W)
        rgb = dc.render_ref(scene, cam, W, H, depth, S, A)
        out[sc.fixture_key(name, S)] = rgb
        print(f"{name} S={S} depth {depth}: {int(np.isnan(rgb).any(axis=2).sum())} NaN pixels", flush=True)
    np.savez_compressed(dc.GOLDEN, **out)
    print(f"wrote {dc.GOLDEN}: {os.path.getsize(dc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
