"""GPU: every conservative culling test pinned at tangency.  The scenes of tests/tangent_common.py hold one sphere (the
blocker) tangent to a ray a bound reasons about — a hair inside and a hair outside, pen = +-1e-3 .. +-1e-12 and 0 — and
every render path that culls must agree with the oracle, which has no filters, bit for bit.  tests/test_tangent_oracle.py
pins the oracle to the reference build on the same rays and shows that the blocker decides the target pixel, so a sphere
or a board skipped wrongly is a pixel wrong here.

Every (case, rung) is rendered four times in a row on one context — first render, calibration, two cached renders (which
read the cached primary cone masks, sky verdicts, sky runs and level masks) — and its target ray and target pixel's
primary ray also go through the ray-list entry points (rt_intersect_dev, rt_trace_rays_dev at depth 0 and 2).

Which cases sit on which bound (every kept case has rungs at |pen| <= 1e-9 on both sides):

  sphere_reject32, K (S^2 + r^2)          reflection and shadow rays of test_render_ladder[s3*] (secondary rays of scenes
                                          without wave masks), every ray list, test_ray_lists_far_origins (the S term)
  DevSpherePrimF (per-eye primary filter) primary cases of every base, test_render_ladder[s3-*-primary] with nothing else
  primary_cone_mask: wave_axis,           primary cases at lanes 0, 7, 56, 63 of c2 / c3 (fast kernels), s19 and c5
    sphere_cone_record, cone_keeps        (culling kernels), first render (in kernel) and cached renders (per-tile copy)
  wave_axis' slack (cone_camera)          test_far_camera_ladder: a camera whose FP32 image is a third of a pixel off
  sky verdict: edge_misses,               test_board_edge_eyes (both sides of the board's edges, sky runs and
    board_edge_record, sky runs           RT_SKY_RUN_MAX=0), primary sky cases of c2 / s19 / c5-replace_last
  ray_bundle_mask / ray_bundle_part       reflection cases of s19 and c5 at corner lanes (first / last `on` lane), depth 2, 3
  shadow_bundle_mask, DevSphereLightF     shadow cases of s19 and c5, light 0 and light 1 (the li * ns stride), blocker
                                          near the hit, mid-way and next to the light
  per-tile level masks                    renders 3 and 4 of the shadow and reflection cases: c2 / c3 (written by the
                                          separate culling launch, read by the fast kernels), s19 and c5
  the masks' last bit, sphere_bits        c5-replace_last (index 63) and c5-last (index 64, 65 spheres)
  padding batches                         blocker first (index 0) and last; c2-last and c5-last open a new batch of 4
  motion_filter, rt_set_motion            test_motion_sweep_ends (the swept records at both ends of the sweep)
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer, decode_hits  # noqa: E402

from . import motion_common as mc  # noqa: E402
from . import tangent_common as tc  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = tc.W, tc.H
HIT_FIELDS = ("hit", "material", "point", "normal", "reflected_end")


def _tracer():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return Tracer(0)


@pytest.fixture(scope="module")
def tr():
    t = _tracer()
    yield t
    t.close()


class Findings:
    """Mismatches collected over a ladder, so a failing bound is reported with every rung it loses."""

    def __init__(self):
        self.msgs = []
        self.checked = 0

    def same(self, got, want, what):
        self.checked += 1
        if not np.array_equal(got, want, equal_nan=True):
            self.msgs.append(what)

    def done(self):
        assert self.checked > 0
        assert not self.msgs, f"{len(self.msgs)} of {self.checked} comparisons differ: " + "; ".join(self.msgs[:12])


def _four_renders(t, find, sa, cam, depth, what):
    """First render, calibration and two cached renders of the scene the context holds against po.render."""
    want, want_rc = po.render(sa, cam, W, H, depth)
    for k in range(4):
        b = t.render(cam, W, H, depth, rgba32f=False, rgb64f=True, raycount=True)
        torch.cuda.synchronize()
        find.same(b["rgb64f"].cpu().numpy(), want, f"{what} depth {depth} render {k} rgb64f")
        find.same(b["raycount"].cpu().numpy().view(np.uint32), want_rc, f"{what} depth {depth} render {k} raycount")


def _ray_lists(t, find, sa, starts, ends, what, depths=(0, 2)):
    """rt_intersect_dev and rt_trace_rays_dev on the scene the context holds against po.intersect / po.trace_rays."""
    S, E = torch.tensor(starts, device="cuda"), torch.tensor(ends, device="cuda")
    got = decode_hits(t.intersect(S, E))
    want = po.intersect(sa, starts, ends)
    for k in HIT_FIELDS:
        find.same(got[k], want[k], f"{what} intersect {k}")
    for depth in depths:
        rgb, rc = t.trace_rays(S, E, depth)
        want_rgb, want_rc = po.trace_rays(sa, starts, ends, depth)
        find.same(rgb.cpu().numpy(), want_rgb, f"{what} trace_rays depth {depth} colours")
        find.same(rc.cpu().numpy().view(np.uint32), want_rc, f"{what} trace_rays depth {depth} ray counts")
    return want


def _ladder(t, name, where, case_list, depths, far=False):
    f = tc.base_frame(name, far)
    cam = f["cam"]
    find = Findings()
    for c in case_list:
        starts = np.array([c.p, f["eye"]], np.float64)
        ends = np.array([c.end, f["sp"][c.j, c.i]], np.float64)
        for pen in tc.PENS:
            sc, _ = tc.with_blocker(f["scene"], where, c.centre(pen), c.r)
            sa = sc.to_abi()
            t.set_scene(sa)
            what = f"{name}-{where} {c.label()} pen {pen:g}"
            for depth in depths:
                _four_renders(t, find, sa, cam, depth, what)
            _ray_lists(t, find, sa, starts, ends, what)
    find.done()


# (base scene, where the blocker goes, kind, light): what each base exercises is in the module docstring
LADDERS = [
    ("s3", "last", "primary", 0), ("s3l2", "first", "shadow", 1), ("s3", "last", "reflection", 0),
    ("c2", "last", "primary", 0), ("c2", "first", "primary", 0), ("c2", "last", "shadow", 0),
    ("c3", "first", "shadow", 1), ("c2", "last", "reflection", 0), ("c3", "first", "reflection", 0),
    ("s19", "last", "primary", 0), ("s19", "first", "primary", 0), ("s19", "last", "shadow", 0),
    ("s19", "first", "shadow", 1), ("s19", "last", "reflection", 0), ("s19", "first", "reflection", 0),
    ("c5", "replace_last", "primary", 0), ("c5", "last", "primary", 0), ("c5", "replace_last", "shadow", 1),
    ("c5", "last", "shadow", 0), ("c5", "replace_last", "reflection", 0), ("c5", "last", "reflection", 0),
]


@pytest.mark.parametrize("name,where,kind,light", LADDERS, ids=[f"{a}-{b}-{c}{d if c == 'shadow' else ''}"
                                                                for a, b, c, d in LADDERS])
def test_render_ladder(tr, name, where, kind, light):
    """Every kept case of the kind over the whole ladder: depth 1 for primary and shadow cases, 2 and 3 for
    reflection cases."""
    keep, _ = tc.kept(name, kind, light, where)
    _ladder(tr, name, where, keep, (2, 3) if kind == "reflection" else (1,))


@pytest.mark.parametrize("name,where", [("c2", "last"), ("s19", "first"), ("c5", "replace_last")])
def test_far_camera_ladder(tr, name, where):
    """The primary cases seen by tangent_common.camera(far=True): eye and look_at 3e4 away and 10 apart, so the FP32
    camera of the per-wave tests is off by about a third of a pixel and only wave_axis' `slack` keeps the primary cone
    mask and the sky verdict from culling the blocker at a tile's corner."""
    keep, _ = tc.kept_far(name)
    _ladder(tr, name, where, keep, (1,), far=True)


@pytest.mark.parametrize("name,env", [("c2", None), ("s19", None), ("c2", "RT_SKY_RUN_MAX")])
def test_board_edge_eyes(monkeypatch, name, env):
    """No blocker: a tile-corner pixel that hits the board from one eye and misses everything from the adjacent double,
    with the eyes 2^10 and 2^20 doubles either side — each eye a new view: first render, calibration, two cached
    renders (sky verdicts and sky runs; RT_SKY_RUN_MAX=0: whole streaks), at depth 1."""
    if env:
        monkeypatch.setenv(env, "0")                     # (read when the context is created; restored by the fixture)
    t = _tracer()
    try:
        f = tc.base_frame(name)
        t.set_scene(f["sa"])
        find = Findings()
        outcomes = []
        for i, j, axis, eyes in tc.board_edge_eyes(name):
            for eye in eyes:
                outcomes.append(tc._pixel_hits(f["sa"], eye, i, j)[0])
                _four_renders(t, find, f["sa"], tc.camera(eye), 1, f"{name} px({i},{j}) eye {eye}")
        assert 0 < sum(outcomes) < len(outcomes)
        find.done()
    finally:
        t.close()


@pytest.mark.parametrize("env", ["RT_WG_STAGING", "RT_SCENE_IN_LDS"])
@pytest.mark.parametrize("kind,light", [("primary", 0), ("shadow", 1), ("reflection", 0)])
def test_workgroup_variants_at_tangency(monkeypatch, env, kind, light):
    """One case of each kind (a corner lane, c3's 8 spheres and two lights) under the 256-thread A/B variants, each on
    a context of its own."""
    keep, _ = tc.kept("c3", kind, light)
    case = [c for c in keep if c.lane in tc.CORNER_LANES and c.r <= 6.0][1]
    monkeypatch.setenv(env, "1")
    t = _tracer()
    try:
        _ladder(t, "c3", "last", [case], (2,) if kind == "reflection" else (1,))
    finally:
        t.close()


def test_ray_lists_far_origins(tr):
    """sphere_reject32's S term: rays tangent, by the ladder, to blockers of r = 0.5, 20 and 150 from origins at
    distances 1e3, 1e5 and 3e6, pointed back at them; c3's scene with its bounding sphere (the far origins are culled
    by it unless they point through it) and with radius 0 (cull off, so every far ray reaches the blocker's test).
    At every origin scale the blocker is hit by some rays and missed by others."""
    base = tc.base_scene("c3")
    base_abi = base.to_abi()
    base_abi.radius = 0.0
    find = Findings()
    for scale in tc.FAR_SCALES:
        changed = []
        for r in tc.FAR_RADII:
            sc, _ = tc.with_blocker(base, "last", tc.far_centre(), r)
            s, e = tc.tangent_rays(tc.far_centre(), r, scale)
            for radius in (None, 0.0):
                sa = sc.to_abi()
                if radius is not None:
                    sa.radius = radius
                tr.set_scene(sa)
                want = _ray_lists(tr, find, sa, s, e, f"r {r:g} scale {scale:g} bound {radius}")
            without = po.intersect(base_abi, s, e)
            changed.append((want["hit"] != without["hit"]) | (want["point"] != without["point"]).any(axis=1))
        changed = np.concatenate(changed)
        assert 0 < int(changed.sum()) < len(changed), scale
    find.done()


# ----------------------------------------------------------------------------------------------------- motion
@pytest.mark.parametrize("a,b", [(0, 0), (1, 1)], ids=["first-sample", "last-sample"])
def test_motion_sweep_ends(tr, a, b):
    """The lens kernel's MOTION kind, 16 x 16 pixels, S = 2, pinhole, point lights: the moving blocker (|d| = 8 r)
    touches one sample's primary ray at that sample's time, the first (sigma = -3F/4) or the last (+3F/4): the ends of
    the sweep the swept filter records must cover.  The frame and counters equal the mean of oracle traces on the
    displaced scenes bit for bit over the ladder, and the blocker decides the pixel (the sensitivity condition of
    tangent_common on this frame)."""
    MW, MH, MS, MF = tc.MOTION_W, tc.MOTION_H, tc.MOTION_S, tc.MOTION_F
    cam = tc.motion_camera()
    find = Findings()
    n_sensitive = 0
    for i, j, r in tc.MOTION_PIXELS:
        pixel = {}
        for pen in tc.PENS:
            sc, disp = tc.motion_case(i, j, a, b, r, pen)
            e = mc.render(sc, cam, MW, MH, 1, MS, 0.0, 0.0, MF, disp)
            pixel[pen] = e["rgb"][j, i].tobytes() + e["rc2"][j, i].tobytes()
            tr.set_scene(sc)
            tr.set_motion(disp)
            got = tr.render_motion(cam, MW, MH, 1, MS, 0.0, 0.0, MF, rgba32f=False, rgb64f=True, raycount=True)
            torch.cuda.synchronize()
            what = f"px({i},{j}) sample ({a},{b}) r {r:g} pen {pen:g}"
            find.same(got["rgb64f"].cpu().numpy(), e["rgb"], what + " rgb64f")
            find.same(got["raycount"].cpu().numpy().view(np.uint32), e["rc2"], what + " raycount")
        n_sensitive += tc.is_sensitive(pixel.__getitem__)
    assert n_sensitive >= 2
    find.done()
