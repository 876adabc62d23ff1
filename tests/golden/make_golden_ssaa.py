#!/usr/bin/env python3
"""Generate tests/golden/ssaa.npz: supersampled frames from the REFERENCE's own compiled rayTraceRay.

Each case is po.ref_render(scene, S W, S H, depth, pitch / S) (oracle/_ref/libref.so, see make_golden.py) reduced
by the pairwise tree of include/rt_api.h (tests/ssaa_common.py reduce_tree).  ref_render takes no camera, so the
cases use even W and H: there the sample-grid camera (bottom_x = S * (-W / 2)) is the reference's own camera of
the S W x S H frame (bottom_x = -(S W) / 2).

All cases are 38 x 22 at pitch 500 / 38 (ssaa_common.FIXTURES); each stores the expected rgb64f [22, 38, 3].

Run in the build container (needs /root/reference):  python tests/golden/make_golden_ssaa.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import pyoracle as po  # noqa: E402
from tests import ssaa_common as sc  # noqa: E402


def main() -> None:
    po.build(ref=True)
    W, H = sc.FIX_W, sc.FIX_H
    assert W % 2 == 0 and H % 2 == 0
    out = {}
    for name, S in sc.FIXTURES:
        scene, depth = sc.scene_of(name)
        hi = po.ref_render(scene, S * W, S * H, depth, (500.0 / W) / S)
        rgb = sc.reduce_tree(hi, S)
        out[sc.fixture_key(name, S)] = rgb
        nan_px = int(np.isnan(rgb).any(axis=2).sum())
        uneq = int((hi.reshape(H, S, W, S, 3) != hi.reshape(H, S, W, S, 3)[:, :1, :, :1]).any(axis=(1, 3, 4)).sum())
        print(f"{name} S={S} depth {depth}: {nan_px} NaN pixels, {uneq} of {W * H} pixels with unequal samples",
              flush=True)
    np.savez_compressed(sc.GOLDEN, **out)
    print(f"wrote {sc.GOLDEN}: {os.path.getsize(sc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
