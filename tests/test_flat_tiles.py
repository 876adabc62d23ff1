"""The flat-tile yardstick on the CPU: the oracle's per-tile truth the GPU tests compare the calibration's verdicts with
(flat_tiles_common.oracle_truth: po.intersect on the primary, shadow and reflected rays of the clamped 8 x 8 tiles), with
its counts at the GPU tests' shapes pinned; and the layout of the dispatch record's word (rt_diag_disp_sky_word, the
function the device's table kernels run): flat is set only beside sphere-free, and no run length reaches either bit."""
import pytest

from ray_tracer_fragment_shader_amd import abi

from . import flat_tiles_common as fc


@pytest.mark.parametrize("key", sorted(fc.ORACLE_COUNTS), ids=lambda k: f"{k[0]}-{k[1]}x{k[2]}")
def test_oracle_counts(key):
    """Tiles all of whose 64 lanes hit the board, are lit by every light and have a missing reflected ray; and tiles
    with any primary hit."""
    name, W, H = key
    t = fc.oracle_truth(name, W, H)
    got = (int(t["flat"].sum()), int(t["any_hit"].sum()))
    print(f"{name} {W}x{H}: {got[0]} flat tiles of {got[1]} with a hit; {int(t['board'].sum())} all-board tiles")
    assert got == fc.ORACLE_COUNTS[key]
    assert not (t["flat"] & ~t["board"]).any() and not (t["board"] & ~t["any_hit"]).any()


def test_c2_64x40_has_hits_but_no_flat_tile():
    """The small frame the GPU tests use for "the class does not occur": its one all-board tile is shadowed or
    reflects a sphere, so it is not sphere-free either, and no other tile can be flat."""
    t = fc.oracle_truth("c2", 64, 40)
    assert t["any_hit"].any() and int(t["board"].sum()) == 1 and not t["flat"].any()


def test_noboard_has_no_flat_tile():
    t = fc.oracle_truth("noboard", 320, 184)
    assert not t["board"].any() and not t["flat"].any()


def test_clamped_tiles():
    """A tile of the last column / row is judged on its valid pixels: the clamped lanes repeat the last one."""
    import numpy as np
    px = np.ones((9, 10), bool)
    assert fc.tiles_all_clamped(px).shape == (2, 2) and fc.tiles_all_clamped(px).all()
    px[8, 9] = False                                       # the one valid pixel row of tile row 1, its last column
    g = fc.tiles_all_clamped(px)
    assert g.tolist() == [[True, True], [True, False]]
    assert fc.tiles_any(~px).tolist() == [[False, False], [False, True]]


def test_record_word_layout():
    runs = [0, 1, 2, 15, 16, 255, 4096, fc.RUN_MAX]
    for run in runs:                                        # tiles outside the classes: the word is the run length
        for flat in (0, 1):                                 # (flat without sphere-free marks nothing)
            w = fc.sky_word(run, 0, flat)
            assert w == run and w & (fc.SPHERE_FREE_BIT | fc.FLAT_BIT) == 0
    assert fc.sky_word(0, 1, 0) == fc.SPHERE_FREE_BIT
    assert fc.sky_word(0, 1, 1) == fc.SPHERE_FREE_BIT | fc.FLAT_BIT
    for sf in (0, 1):
        for flat in (0, 1):
            w = fc.sky_word(0, sf, flat)
            assert not (w & fc.FLAT_BIT) or (w & fc.SPHERE_FREE_BIT), "flat implies sphere-free"
            assert w & ~(fc.SPHERE_FREE_BIT | fc.FLAT_BIT) == 0, "a marked record holds no run length"
    assert fc.RUN_MAX < fc.FLAT_BIT < fc.SPHERE_FREE_BIT


def test_gates_on_the_host():
    """The wave-uniform gates through the function the device runs (rt_diag_flat_gates).  The origin-skip limit of the
    tests' scenes is reached by finite cameras (the GPU tests render from both sides of it).  hits_ok is not: for every
    eye inside the limit it is on, and it goes off only far beyond it — so no view of these scenes has flat tiles with
    hits_ok off, and what the device can be shown there is only that such a view has no flat tile
    (test_gpu_flat_tiles.py::test_eye_without_hits_ok).  That trace_flat needs no hits_ok is its proof's business: every
    test hits_ok guards returns "not blocked" / "no hit" on both of its branches under skip == 0."""
    import math
    for name in ("c2", "c3", "rise"):
        g, h, y = fc.flat_gates(name, (0.0, 100.0, 200.0))
        assert (g, h) == (1, 1) and y > 0
        sc = fc.sk.scene_named(name).to_abi()
        eps2 = sc.small_number * sc.small_number
        assert y == (eps2 / 2 / 2.0 ** -50 - 5 * abs(fc.sk.board_y(sc)) - 1) / 3      # rt_host.cpp board_skip_y
        for ey, want in ((y, 1), (-y, 1), (math.nextafter(y, math.inf), 0), (-math.nextafter(y, math.inf), 0),
                         (2 * y, 0), (1e10, 0), (0.0, 1), (-100.0, 1), (math.nan, 0), (math.inf, 0)):
            assert fc.flat_gates(name, (0.0, ey, 200.0))[0] == want, (name, ey)
        # hits_ok inside the gate: on at every height up to the limit (and sideways as far)
        for ey in (0.0, 100.0, -300.0, 1e3, 1e5, 0.5 * y, y, -y):
            assert fc.flat_gates(name, (0.0, ey, 200.0))[1] == 1, (name, ey)
        assert fc.flat_gates(name, (y, 100.0, -y))[1] == 1
        assert fc.flat_gates(name, (0.0, 1e10, 200.0)) [:2] == (0, 0)                   # the GPU test's far eye
    assert fc.flat_gates("noboard", (0.0, 100.0, 200.0))[0] == 0                       # no board: never flat


def test_record_word_bad_arguments():
    assert fc.sky_word(fc.RUN_MAX + 1, 0, 0) == abi.RT_EINVAL
    assert fc.sky_word(3, 1, 0) == abi.RT_EINVAL             # a sphere-free tile traces: no run
    assert abi.lib().rt_diag_disp_sky_word(0, 0, 0, None) == abi.RT_EINVAL
    assert abi.lib().rt_diag_flat_tiles(None, None, None) == abi.RT_EINVAL
    assert abi.lib().rt_diag_flat_tile_grid(None, None, 0) == abi.RT_EINVAL
    assert abi.lib().rt_diag_flat_gates(None, None, None, None, None) == abi.RT_EINVAL
