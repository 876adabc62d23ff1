"""Converging accumulation (rt_render_converge_dev): rules 2 - 4 of the contract in include/rt_api.h restated with numpy
float64 on the frames the shutter render's oracle route defines (tests/shutter_common.py expected, one frame per seed
(seed + p) mod 2^32), shared by tests/test_converge_oracle.py, tests/test_gpu_converge.py and
tests/golden/make_golden_converge.py.

Every pixel carries (acc, sq, n) and is on the pass of its own n; before each of the call's K steps the stop rule is
evaluated on the state alone.  numpy evaluates `sq + v * v` as a product and a sum, one IEEE operation each (no fused
multiply-add), and the rule's expressions are spelled operator by operator.  Nothing here calls the code under test.
"""
import functools
import os

import numpy as np

from . import accum_common as ac
from . import shutter_common as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "converge.npz")
N_MAX = 2 ** 31

# The committed fixture (tests/golden/converge.npz, from the reference build), 38 x 22 at pitch 500 / 38: the scene,
# lights and camera motion of an accum_common.FIXTURES case's shutter fixture, its first seed, and (K, M, E) chosen so
# that the counts are mixed.  Stored under <key>_acc, _sq, _count and _mean.
FIXTURE = ("c2_crane_k12", "c2_crane_s1_j4", 0xFFFFFFFF, 12, 3, 1.0 / 8.0)
FIX_W, FIX_H = ac.FIX_W, ac.FIX_H


def fixtures():
    return dict(np.load(GOLDEN))


def stopped(acc, sq, n, M, E):
    """Rule 3 -> bool [H, W].  n: integer array."""
    n = np.asarray(n, np.int64)
    E = np.float64(E)
    nf = n.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        d = sq - (acc * acc) / nf                            # a multiplication, a division, a subtraction
        lim = (E * E) * (nf * (n - 1).astype(np.float64)[..., None])     # three multiplications
        held = (d > lim).any(axis=2)                         # a NaN d compares false
    return (n == N_MAX) | ((n >= M) & ~held)


def zero_state(H, W):
    """A new sum: n = 0 everywhere; acc and sq are NaN there, as buffers the call must not read."""
    return (np.full((H, W, 3), np.nan), np.full((H, W, 3), np.nan), np.zeros((H, W), np.int64))


def converge(frame_of, state, K, M, E):
    """Rules 2 - 4 from `state` = (acc, sq, n) with frame_of(p) -> (v_p [H, W, 3] float64, counters [H, W, 2] uint32).
    -> dict(acc, sq, n (int64), mean, rc2 (uint32, wrapping), active, received: the passes each pixel got in the call)."""
    acc, sq, n = (np.array(state[0], np.float64, copy=True), np.array(state[1], np.float64, copy=True),
                  np.array(state[2], np.int64, copy=True))
    rc2 = np.zeros(n.shape + (2,), np.uint32)
    n0 = n.copy()
    assert K >= 1
    for _ in range(K):
        live = ~stopped(acc, sq, n, M, E)
        if not live.any():
            break
        for p in np.unique(n[live]):
            v, c = frame_of(int(p))
            m = live & (n == p)
            if p == 0:
                acc[m] = v[m]
                sq[m] = v[m] * v[m]
            else:
                acc[m] = acc[m] + v[m]
                sq[m] = sq[m] + (v[m] * v[m])                # the product is rounded before the sum
            rc2[m] = rc2[m] + c[m].astype(np.uint32)
        n[live] += 1
    assert (n >= 1).all()
    with np.errstate(invalid="ignore"):
        mean = acc / n.astype(np.float64)[..., None]         # one IEEE division per channel
    return {"acc": acc, "sq": sq, "n": n, "mean": mean, "rc2": rc2, "received": n - n0,
            "active": int((~stopped(acc, sq, n, M, E)).sum())}


def state_of(r):
    return r["acc"], r["sq"], r["n"]


def frames(name, motion, W, H, S, J, seed, A, R, F, moves=(), light_centres=None, depth=None, pitch_w=None):
    """frame_of(p) on shutter_common.expected (cached there) with the seed (seed + p) mod 2^32."""
    def frame_of(p):
        e = hc.expected(name, motion, W, H, S, J, ac.seed_of(seed, p), A, R, F, moves, light_centres, depth, "lane",
                        pitch_w)
        return e["rgb"], e["rc2"]
    return frame_of


@functools.lru_cache(maxsize=None)
def expected(name, motion, W, H, S, J, seed, K, M, E, A, R, F, moves=(), light_centres=None, depth=None, pitch_w=None):
    """One call from a zeroed count, computed once per case.  -> converge()'s dict plus cam, depth, d, motion and
    frame_of; read-only arrays."""
    frame_of = frames(name, motion, W, H, S, J, seed, A, R, F, moves, light_centres, depth, pitch_w)
    out = converge(frame_of, zero_state(H, W), K, M, E)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    e = hc.expected(name, motion, W, H, S, J, ac.seed_of(seed, 0), A, R, F, moves, light_centres, depth, "lane", pitch_w)
    out["cam"], out["depth"], out["d"], out["motion"], out["frame_of"] = e["cam"], e["depth"], e["d"], e["motion"], frame_of
    return out


def tile_counts(n, S):
    """The pass counts grouped by the wave that owns them: a list of 1-D arrays, one per 8 x 8 tile of the sample
    grid, (8 / S) x (8 / S) output pixels each (fewer at the frame's edges)."""
    t = 8 // S
    H, W = n.shape
    return [n[y:y + t, x:x + t].ravel() for y in range(0, H, t) for x in range(0, W, t)]
