"""CPU checks of the tangent constructions (tests/tangent_common.py) the GPU tests of tests/test_gpu_tangent.py render:

* the oracle equals the reference build bit for bit on every constructed target ray against its blocker scene, over
  the whole penetration ladder (where the reference build is present): the oracle had never been pinned to the
  reference at tangency from arbitrary origins;
* the constructions are sensitive — the blocker decides the target pixel on the hit side of tangency and is invisible
  to it on the other — so the GPU tests cannot pass vacuously; at most a quarter of the cases of a kind may fail this,
  and every corner lane keeps a case;
* the sky-tile verdict (rt_diag_sky_tiles, the host evaluation of wave_axis / cone_keeps / edge_misses) is sound at
  tangency: no proved tile holds a pixel the oracle says hits, in particular not the target's tile.
"""
import dataclasses

import numpy as np
import pytest

from oracle import pyoracle as po

from . import sky_common as sk
from . import tangent_common as tc
from .test_sky_tiles import _check_sound

KINDS = [("primary", 0), ("shadow", 0), ("shadow", 1), ("reflection", 0)]
KIND_IDS = ["primary", "shadow-light0", "shadow-light1", "reflection"]
FIELDS = ("hit", "material", "point", "normal", "reflected_end", "transmitted_end")


# ------------------------------------------------------------------------------------- oracle against the reference
@pytest.mark.ref
@pytest.mark.parametrize("kind,light", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", ["s3l2", "c3", "s19", "c5"])
def test_oracle_equals_reference_on_tangent_rays(name, kind, light):
    """Every constructed case (kept or not) and every rung: the target ray and the target pixel's primary ray, through
    po.intersect and po.trace_rays (depth 0 and 2), against the reference's own intersection and rayTraceRay on the
    same spheres."""
    if not po.ref_available():
        pytest.skip("no reference build here")
    f = tc.base_frame(name)
    hits = 0
    for n_case, c in enumerate(tc.cases(name, kind, light)):
        starts = np.array([c.p, f["eye"]], np.float64)
        ends = np.array([c.end, f["sp"][c.j, c.i]], np.float64)
        for pen in tc.PENS:
            sc, _ = tc.with_blocker(f["scene"], ("last", "first")[n_case % 2], c.centre(pen), c.r)
            sa = sc.to_abi()
            cen, rad = tc.centres_radii(sc)
            got = po.intersect(sa, starts, ends)
            want = po.ref_intersect_at(sc, cen, rad, starts, ends)
            for k in FIELDS:
                assert np.array_equal(got[k], want[k], equal_nan=True), (c.label(), pen, k)
            for depth in (0, 2):
                rgb, _ = po.trace_rays(sa, starts, ends, depth)
                assert np.array_equal(rgb, po.ref_trace_rays_at(sc, cen, rad, starts, ends, depth), equal_nan=True), \
                    (c.label(), pen, depth)
            hits += int(got["hit"][0])
    assert hits > 0


@pytest.mark.ref
@pytest.mark.parametrize("r", tc.FAR_RADII)
def test_oracle_equals_reference_on_rays_tangent_to_a_placed_blocker(r):
    """The blocker of the GPU test's ray lists stands on a board square, so the reference harness places it itself:
    rays tangent to it by the ladder from origins 50 and 300 away and from the far origins (1e3, 1e5, 3e6), through
    po.intersect and po.trace_rays (depth 0 and 2) against the reference's own."""
    if not po.ref_available():
        pytest.skip("no reference build here")
    base = tc.base_scene("c3")
    sc = dataclasses.replace(base, spheres=list(base.spheres) + [tc.far_spec(r)])
    same, _ = tc.with_blocker(base, "last", tc.far_centre(), r)
    assert tc.centres_radii(sc)[0].tobytes() == tc.centres_radii(same)[0].tobytes()
    hits = 0
    for scale in (50.0, 300.0) + tc.FAR_SCALES:
        s, e = tc.tangent_rays(tc.far_centre(), r, scale)
        got = po.intersect(sc.to_abi(), s, e)
        want = po.ref_intersect(sc, s, e)
        for k in FIELDS:
            assert np.array_equal(got[k], want[k], equal_nan=True), (scale, k)
        for depth in (0, 2):
            rgb, _ = po.trace_rays(sc.to_abi(), s, e, depth)
            assert np.array_equal(rgb, po.ref_trace_rays(sc, s, e, depth), equal_nan=True), (scale, depth)
        hits += int(got["hit"].sum())
    assert 0 < hits < 5 * len(s)


# ------------------------------------------------------------------------------------------------- sensitivity
# the placements of the blocker the GPU ladders render, per base scene
PLACEMENTS = {"s3l2": ("last", "first"), "c3": ("last", "first"), "s19": ("last", "first"),
              "c5": ("last", "replace_last")}


@pytest.mark.parametrize("kind,light", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_cases_are_sensitive(name, kind, light):
    """In every scene the GPU ladders render (the blocker appended, first, or in place of the last sphere): at most a
    quarter of the constructed cases are dropped, every corner lane keeps one, the kept cases hold radii up to 150, and
    each kept case's pixel at pen = +1e-9 differs from the one at -1e-9."""
    for where in PLACEMENTS[name]:
        keep, n = tc.kept(name, kind, light, where)
        assert n >= 24
        assert 4 * len(keep) >= 3 * n, f"{where}: {len(keep)} of {n}"
        lanes = {c.lane for c in keep}
        assert set(tc.CORNER_LANES) <= lanes, (where, lanes)
        if kind == "primary":
            assert tc.INTERIOR_LANE in lanes
            assert {tc.SKY, tc.BOARD} <= {c.behind for c in keep}
        assert max(c.r for c in keep) >= 20.0 and min(c.r for c in keep) <= 5.0
        for c in keep:
            assert tc.target_pixel(name, c, 1e-9, where=where) != tc.target_pixel(name, c, -1e-9, where=where), \
                (where, c.label())


def test_one_light_bases_share_the_two_light_cases():
    """s3 / c2 differ from s3l2 / c3 by the second light only: the primary and reflection targets are the same rays."""
    for one, two in (("s3", "s3l2"), ("c2", "c3")):
        for kind in ("primary", "reflection"):
            assert tc.cases(one, kind) == tc.cases(two, kind)
            for where in ("last", "first"):
                assert len(tc.kept(one, kind, 0, where)[0]) * 4 >= 3 * tc.kept(one, kind, 0, where)[1]


def test_board_edge_eyes_straddle_the_edge():
    """Each case: two adjacent doubles of one eye coordinate, the corner pixel on the board from one and missing
    everything from the other; cases on both axes and on several lanes."""
    for name in ("c2", "s19"):
        cases = tc.board_edge_eyes(name)
        assert len(cases) >= 4 and {ax for _, _, ax, _ in cases} == {0, 1}
        assert len({(j % 8) * 8 + i % 8 for i, j, _, _ in cases}) >= 3
        sa = tc.base_frame(name)["sa"]
        for i, j, axis, eyes in cases:
            a, b = eyes[0][axis], eyes[1][axis]
            assert abs(int(np.array([a]).view(np.int64)[0]) - int(np.array([b]).view(np.int64)[0])) == 1
            outcomes = [tc._pixel_hits(sa, e, i, j)[0] for e in eyes]
            assert outcomes[0] == 1 and outcomes[1] == 0 and 0 < sum(outcomes) < len(outcomes), (i, j, outcomes)


@pytest.mark.parametrize("a,b", [(0, 0), (1, 1)], ids=["first-sample", "last-sample"])
def test_motion_cases_are_sensitive(a, b):
    """The moving blocker of test_gpu_tangent.test_motion_sweep_ends decides its pixel at the end of its sweep."""
    for i, j, r in tc.MOTION_PIXELS:
        assert tc.is_sensitive(lambda pen: tc.motion_pixel(i, j, a, b, r, pen)), (i, j, r)


# ------------------------------------------------------------------------------------ sky verdict at tangency
@pytest.mark.parametrize("name,where", [("c2", "last"), ("c2", "first"), ("s19", "last"), ("c5", "replace_last")])
def test_sky_verdict_sound_with_tangent_blockers(name, where):
    """Scenes the early-out covers (8 .. 64 padded spheres).  Every kept primary case with pen > 0: the target pixel
    hits the blocker, so the verdict of its tile is 0; over all tiles of these frames no proved tile contains a pixel
    that hits (test_sky_tiles._check_sound); and the verdict still proves tiles, so the check is not vacuous."""
    f = tc.base_frame(name)
    keep, _ = tc.kept(name, "primary", 0, where)
    proved = 0
    for c in keep:
        for pen in (p for p in tc.PENS if p > 0):
            sc, _ = tc.with_blocker(f["scene"], where, c.centre(pen), c.r)
            sa = sc.to_abi()
            assert sk.host_verdict(sa, tc.camera(), tc.W, tc.H)[c.j // 8, c.i // 8] == 0, (c.label(), pen)
            proved += _check_sound(sa, tc.W, tc.H, None)[0]
    assert proved > 0


@pytest.mark.parametrize("name,where", [("c2", "last"), ("s19", "first"), ("c5", "replace_last")])
def test_far_camera_cases_and_sky_verdict(name, where):
    """The far camera (tangent_common.camera(far=True)): its primary cases see the blocker at pen = +1e-3 and not at
    -1e-3, on every corner lane, and the host's verdict, whose FP32 camera is a third of a pixel off there, proves no
    tile that holds a hit."""
    keep, n = tc.kept_far(name)
    assert 4 * len(keep) >= 3 * n and set(tc.CORNER_LANES) <= {c.lane for c in keep}
    f = tc.base_frame(name, True)
    for c in keep:
        for pen in (1e-3, 1e-6, -1e-6):
            sc, _ = tc.with_blocker(f["scene"], where, c.centre(pen), c.r)
            sa = sc.to_abi()
            proved = sk.host_verdict(sa, f["cam"], tc.W, tc.H).astype(bool)
            truth = sk.tiles_all_miss(sk.oracle_rc(sa, f["cam"], tc.W, tc.H, 1))
            assert not (proved & ~truth).any(), (c.label(), pen, np.argwhere(proved & ~truth)[:4].tolist())


@pytest.mark.parametrize("name", ["c2", "s19"])
def test_sky_verdict_sound_at_board_edge_eyes(name):
    f = tc.base_frame(name)
    proved = 0
    for i, j, _, eyes in tc.board_edge_eyes(name):
        for eye in eyes:
            if tc._pixel_hits(f["sa"], eye, i, j)[0]:
                assert sk.host_verdict(f["sa"], tc.camera(eye), tc.W, tc.H)[j // 8, i // 8] == 0, (i, j, eye)
            proved += _check_sound(f["sa"], tc.W, tc.H, eye)[0]
    assert proved > 0
