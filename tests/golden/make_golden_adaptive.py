#!/usr/bin/env python3
"""Generate tests/golden/adaptive.npz: adaptively supersampled frames from the REFERENCE's own compiled rayTraceRay.

Each case takes the base frame po.ref_render(scene, W, H, depth, pitch) and the sample frame
po.ref_render(scene, S W, S H, depth, pitch / S) (oracle/_ref/libref.so, see make_golden.py), reduces the latter by
the pairwise tree (tests/ssaa_common.py reduce_tree) and combines the two by the criterion of include/rt_api.h
(tests/adaptive_common.py refine_mask) at threshold 32.  W and H are even, as in make_golden_ssaa.py.

All cases are 38 x 22 at pitch 500 / 38 (adaptive_common.FIXTURES); each stores the expected rgb64f [22, 38, 3] as
<scene>_s<S> and the refined mask [22, 38] uint8 as <scene>_s<S>_mask.  Data only.

Run where the reference build exists (oracle/_ref/libref.so):  python tests/golden/make_golden_adaptive.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import pyoracle as po  # noqa: E402
from tests import adaptive_common as ac  # noqa: E402
from tests import ssaa_common as sc  # noqa: E402


def main() -> None:
    po.build(ref=True)
    W, H, T = ac.FIX_W, ac.FIX_H, ac.FIX_T
    assert W % 2 == 0 and H % 2 == 0
    out = {}
    for name, S in ac.FIXTURES:
        scene, depth = sc.scene_of(name)
        base = po.ref_render(scene, W, H, depth, 500.0 / W)
        hi = po.ref_render(scene, S * W, S * H, depth, (500.0 / W) / S)
        mask = ac.refine_mask(sc.to_rgba8(base), T)
        rgb = np.where(mask[..., None], sc.reduce_tree(hi, S), base)
        out[sc.fixture_key(name, S)] = rgb
        out[sc.fixture_key(name, S) + "_mask"] = mask.astype(np.uint8)
        print(f"{name} S={S} depth {depth}: {int(mask.sum())} of {W * H} pixels refined, "
              f"{int(np.isnan(rgb).any(axis=2).sum())} NaN pixels", flush=True)
    np.savez_compressed(ac.GOLDEN, **out)
    print(f"wrote {ac.GOLDEN}: {os.path.getsize(ac.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
