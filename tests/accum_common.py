"""Progressive accumulation (rt_render_accum_dev): rules 2 and 3 of the contract in include/rt_api.h restated with numpy
float64 on the frames the shutter render's oracle route defines (tests/shutter_common.py expected, one frame per seed
(seed + p) mod 2^32), shared by tests/test_accum_oracle.py, tests/test_gpu_accum.py and
tests/golden/make_golden_accum.py.

The sum is sequential: acc = v_0, then one `+` per pass, left to right (a continued call starts from the accumulator the
passes before it left, which is the same chain); the mean is acc / np.float64(n).  Nothing here calls the code under
test.
"""
import functools
import os

import numpy as np

from . import shutter_common as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accum.npz")

# The committed fixtures (tests/golden/accum.npz, from the reference build), all 38 x 22 at pitch 500 / 38: the scene,
# lights, spheres and camera motion of a shutter_common.FIXTURES entry (by its key), the first seed and the number of
# passes summed from pass 0.  Each stores the accumulator under <key>_acc and the mean under <key>_mean.
FIXTURES = [
    ("c2_pan_k3", "c2_pan_s2_j2", 7, 3),
    ("c2_crane_wrap_k3", "c2_crane_s1_j4", 0xFFFFFFFF, 3),          # the seeds 0xFFFFFFFF, 0, 1
    ("tree_demo_pan_k2", "tree_demo_pan_s1_j4", 5, 2),
]
FIX_W, FIX_H = hc.FIX_W, hc.FIX_H


def fixtures():
    return dict(np.load(GOLDEN))


def shutter_fixture(key):
    """The shutter_common.FIXTURES entry `key` without its own seed: (name, S, J, F, A, R, lights, moves, motion)."""
    (row,) = [f for f in hc.FIXTURES if f[0] == key]
    _, name, S, J, _seed, F, A, R, lights, moves, motion = row
    return name, S, J, F, A, R, lights, moves, motion


def seed_of(seed, p):
    return (int(seed) + int(p)) & 0xFFFFFFFF


def accumulate(frames, counts, n0, K):
    """Rules 2 and 3 on the passes' values frames[p] ([H, W, 3] float64) and counters counts[p] ([H, W, 2] uint32),
    p = 0 .. n0 + K - 1.  -> dict(acc0: the accumulator after n0 passes (None for n0 = 0), acc and mean after n0 + K,
    rc2: the counters of the call's K passes, uint32 and wrapping)."""
    assert K >= 1 and n0 >= 0 and len(frames) == n0 + K == len(counts)
    acc = np.array(frames[0], np.float64, copy=True)
    acc0 = None
    for p in range(1, n0 + K):
        if p == n0:
            acc0 = acc.copy()
        acc = acc + frames[p]                                # one IEEE addition per channel and pass
    rc2 = np.zeros_like(counts[0], dtype=np.uint32)
    for p in range(n0, n0 + K):
        rc2 = rc2 + counts[p].astype(np.uint32)              # uint32 array sums wrap
    with np.errstate(invalid="ignore"):
        mean = acc / np.float64(n0 + K)                      # one IEEE division per channel
    return {"acc0": acc0, "acc": acc, "mean": mean, "rc2": rc2}


@functools.lru_cache(maxsize=None)
def expected(name, motion, W, H, S, J, seed, n0, K, A, R, F, moves=(), light_centres=None, depth=None, pitch_w=None):
    """Computed once per case from shutter_common.expected(...)["rgb"] / ["rc2"] of the seeds (seed + p) & 0xffffffff,
    p = 0 .. n0 + K - 1 (the arguments are that function's).
    -> dict(acc0, acc, mean, rc2, frames, cam, depth, d, motion); read-only."""
    es = [hc.expected(name, motion, W, H, S, J, seed_of(seed, p), A, R, F, moves, light_centres, depth, "lane", pitch_w)
          for p in range(n0 + K)]
    out = accumulate([e["rgb"] for e in es], [e["rc2"] for e in es], n0, K)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    out["frames"] = tuple(e["rgb"] for e in es)
    out["cam"], out["depth"], out["d"], out["motion"] = es[0]["cam"], es[0]["depth"], es[0]["d"], es[0]["motion"]
    return out
