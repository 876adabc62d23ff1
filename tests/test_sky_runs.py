"""The run plan of a cached view's dispatch on the CPU (rt_diag_sky_run_plan: the host evaluation of the function the
device's table kernel runs, rt_cone.hpp sky_run_at): a tile that is not sky is one dispatch position, a maximal
streak of sky tiles of a tile row is cut into runs of at most R, one position each.

Checked on the host verdicts (rt_diag_sky_tiles) of real views and on synthetic grids: every tile is covered exactly
once; runs hold sky tiles only, stay in their row and are at most R long; and the position count is what a numpy
restatement gives."""
import ctypes

import numpy as np
import pytest

from ray_tracer_fragment_shader_amd import abi

from . import sky_common as sk
from .sky_runs_common import plan

SCENES = ["c2", "c5", "noboard", "rise"]
SIZES = [(320, 184), (321, 203), (64, 40), (200, 96)]
RUNS = [1, 4, 16, 64]


def positions_numpy(sky, R):
    """Per row: the tiles that are not sky, plus ceil(length / R) for every maximal streak of sky tiles."""
    total = 0
    for row in np.asarray(sky, bool):
        edges = np.diff(np.concatenate(([0], row.astype(np.int8), [0])))
        lengths = np.flatnonzero(edges == -1) - np.flatnonzero(edges == 1)
        total += int((~row).sum()) + int(((lengths + R - 1) // R).sum())
    return total


def check_plan(sky, R):
    sky = np.asarray(sky, np.uint8)
    run, n = plan(sky, R)
    ty, tx = sky.shape
    covered = np.zeros((ty, tx), np.int32)
    heads = 0
    for y in range(ty):
        for x in range(tx):
            r = int(run[y, x])
            assert r >= -1, f"tile ({x}, {y}) was not planned"
            if r == 0:                                   # a tracing tile: a position of its own
                assert sky[y, x] == 0
                covered[y, x] += 1
                heads += 1
            elif r > 0:                                  # the head of a run
                assert r <= R and x + r <= tx, f"run of {r} at ({x}, {y}) of a row of {tx}, R = {R}"
                assert sky[y, x:x + r].all(), f"run of {r} at ({x}, {y}) holds a tile that is not sky"
                assert (run[y, x + 1:x + r] == -1).all()
                covered[y, x:x + r] += 1
                heads += 1
    assert (covered == 1).all(), "every tile belongs to exactly one position"
    assert n == heads == positions_numpy(sky, R)
    if R == 1:
        assert n == sky.size
    return n


@pytest.fixture(scope="module")
def verdicts():
    out = {}
    for name in SCENES:
        sa = sk.scene_named(name).to_abi()
        for W, H in SIZES:
            out[(name, W, H)] = sk.host_verdict(sa, sk.camera(W, H), W, H)
    return out


@pytest.mark.parametrize("R", RUNS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_plan_of_host_verdicts(verdicts, name, size, R):
    sky = verdicts[(name, size[0], size[1])]
    n = check_plan(sky, R)
    assert sky.sum() > 0
    if R > 1:
        assert n < sky.size, "compaction is real at every listed size"


def test_counts_of_todays_verdict(verdicts):
    """The counts the run table was sized by."""
    c2 = verdicts[("c2", 320, 184)]
    assert c2.size == 920
    assert plan(c2, 16)[1] == 462
    assert plan(c2, 4)[1] == 549
    assert plan(verdicts[("noboard", 320, 184)], 16)[1] == 199
    small = verdicts[("c2", 64, 40)]
    assert (small.size, plan(small, 16)[1]) == (40, 31)


def _streak_grid(R):
    """Rows of 3 R + 4 tiles with one streak each: R - 1, R, R + 1 long inside the row, then R - 1, R, R + 1 and one
    tile long ending at the row end, and a whole row."""
    tx = 3 * R + 4
    rows = []
    for length in (R - 1, R, R + 1):
        if length < 1:
            continue
        row = np.zeros(tx, np.uint8)
        row[2:2 + length] = 1
        rows.append(row)
    for length in (R - 1, R, R + 1, 1, tx):
        if length < 1:
            continue
        row = np.zeros(tx, np.uint8)
        row[tx - length:] = 1
        rows.append(row)
    return np.stack(rows)


@pytest.mark.parametrize("R", [1, 2, 4, 16, 64])
def test_synthetic_grids(R):
    ty, tx = 9, 41
    assert check_plan(np.ones((ty, tx), np.uint8), R) == ty * ((tx + R - 1) // R)         # all sky
    assert check_plan(np.zeros((ty, tx), np.uint8), R) == ty * tx                          # no sky
    checker = (np.add.outer(np.arange(ty), np.arange(tx)) & 1).astype(np.uint8)
    assert check_plan(checker, R) == ty * tx                                               # streaks of one tile
    column = np.array([[1], [0], [1], [1], [0]], np.uint8)                                 # a single column of tiles
    assert check_plan(column, R) == 5
    g = _streak_grid(R)
    check_plan(g, R)
    run, _ = plan(g, R)
    if R > 1:
        # a streak of R + 1 is a run of R and a run of 1; one of R a single run; a streak ending at the row end
        # ends its last run there
        row = [r for r in range(g.shape[0]) if g[r, 2:2 + R + 1].all() and not g[r, 2 + R + 1]][0]
        assert run[row, 2] == R and run[row, 2 + R] == 1
        assert run[-1, 0] == min(R, g.shape[1])
    rng = np.random.default_rng(7)
    for p in (0.1, 0.5, 0.9):
        check_plan((rng.random((13, 37)) < p).astype(np.uint8), R)


def test_bad_arguments():
    sky = np.zeros((2, 2), np.uint8)
    run = np.zeros((2, 2), np.int32)
    n = ctypes.c_int()
    L = abi.lib()
    assert L.rt_diag_sky_run_plan(sky.ctypes.data, 2, 2, 0, run.ctypes.data, ctypes.byref(n)) == abi.RT_EINVAL
    assert L.rt_diag_sky_run_plan(None, 2, 2, 4, run.ctypes.data, ctypes.byref(n)) == abi.RT_EINVAL
    assert L.rt_diag_sky_run_plan(sky.ctypes.data, 0, 2, 4, run.ctypes.data, ctypes.byref(n)) == abi.RT_EINVAL
    assert L.rt_diag_disp_count(None, None, None, None) == abi.RT_EINVAL
