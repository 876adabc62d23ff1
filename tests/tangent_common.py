"""Inputs built to sit on the margins of the conservative culling tests (numpy and the CPU oracle only, no GPU): shared
by tests/test_tangent_oracle.py and tests/test_gpu_tangent.py.

A *blocker* is one extra sphere in a base scene, placed tangent to a *target ray* the culling bounds reason about.  For
a target ray with origin p, unit direction u and a unit n orthogonal to u, the blocker of radius r at parameter t with
penetration `pen` has the world centre

    p + t u + r (1 - pen) n

so with pen > 0 the ray dips pen r into the sphere and with pen < 0 it passes pen r outside.  PENS is the ladder every
case is run over.  Target rays come from the oracle on the base scene (po.screen_points, po.intersect):

  primary     the ray of a pixel at a corner lane (0, 7, 56, 63) or an interior lane of a whole 8 x 8 tile, n pointing
              away from the tile's centre in the image plane: the corner lane is the only lane of its wave that can
              reach the blocker.  Sky pixels of the base frame and pixels that hit the board behind the blocker.
  shadow      the segment from a pixel's primary hit q (board or sphere) to a light, the blocker at 0.05, 0.5 and 0.95 of
              its length.
  reflection  the ray from q to the oracle's reflected_end, the blocker at t = 5, 30 and 150.
  board edge  no blocker: eyes found by bisecting one eye coordinate between an eye from which a tile-corner pixel hits
              the board and one from which it misses everything, down to adjacent doubles, with the eyes 2^10 and 2^20
              ulps either side.

Beside them: the primary cases seen by a far camera whose FP32 image is a third of a pixel off (camera(far=True)),
ray lists tangent to a blocker from origins up to 3e6 away (tangent_rays), and a moving blocker that touches one
sample's ray at the end of its sweep (motion_case).

A case is *sensitive* when the oracle's target pixel at pen = +1e-12 differs from the pixel at pen = -1e-3 and every
negative pen gives the -1e-3 pixel: the blocker decides the pixel on the hit side of tangency and is invisible to it on
the other.  kept() drops the others (a blocker hidden behind something, a target the oracle's own rounding decides
the other way) and prints the counts.
"""
import dataclasses
import functools

import numpy as np

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import scenes

from . import dof_common as dc
from . import motion_common as mc

W, H = 64, 48                                          # 8 x 6 whole tiles at the canonical framing
PENS = (1e-3, -1e-3, 1e-6, -1e-6, 1e-9, -1e-9, 1e-12, -1e-12, 0.0)
CORNER_LANES = (0, 7, 56, 63)
INTERIOR_LANE = 27
BOARD, SPHERE = "board", "sphere"                      # what a pixel's primary ray hits in the base frame
SKY = "sky"


@dataclasses.dataclass
class FreeSphere(scenes.SphereSpec):
    """A sphere at any scene-local centre (scenes.SphereSpec places spheres on board squares)."""
    xyz: tuple = (0.0, 0.0, 0.0)

    def center(self):
        return tuple(float(v) for v in self.xyz)


# ------------------------------------------------------------------------------------------------- base scenes
_EXTRA_11 = ("a1", "c1", "g1", "h3", "a3", "d5", "h5", "b7", "f7", "c8", "e8")
_TWO = [scenes.LightSpec("b6", scenes.WHITE), scenes.LightSpec("g3", scenes.GREY)]


def base_scene(name):
    """s3 / s3l2: 3 spheres, one / two lights (no wave masks: the per-eye FP32 filter, sphere_reject32 on secondary
    rays, the light-cone records).  c2 / c3: the benchmark's 8 spheres, one / two lights (with the blocker 9 -> padded
    12: fast kernels, primary cone mask, sky tiles, level masks from the separate culling launch).  s19: c2's spheres
    and 11 smaller ones, two lights (with the blocker 20: the culling kernels).  c5: the benchmark's 64 spheres, two
    lights."""
    if name in ("c2", "c3", "c5"):
        return scenes.CONFIGS[name].scene()
    if name in ("s3", "s3l2"):
        return scenes.Scene(spheres=[scenes.SphereSpec(sq, 20.0) for sq in scenes.SQUARES_8[:3]],
                            lights=_TWO[: 1 if name == "s3" else 2])
    if name == "s19":
        sph = [scenes.SphereSpec(sq, 20.0) for sq in scenes.SQUARES_8]
        sph += [scenes.SphereSpec(sq, 8.0, 30.0 * (k % 2)) for k, sq in enumerate(_EXTRA_11)]
        return scenes.Scene(spheres=sph, lights=list(_TWO))
    raise KeyError(name)


FAR_BACK, FAR_LOOK = 3e4, 10.0


def camera(eye=None, far=False):
    """The canonical camera of a W x H frame (optionally from another eye); far: the same view from 3e4 further back
    along the view axis with look_at 10 ahead of the eye and the pitch scaled, so the frame still spans the board.  Eye
    and look_at then agree in their leading digits, the FP32 camera of the per-wave tests (rt_cone.hpp cone_camera)
    loses about 2^-12 of direction, a third of a pixel, and only its `slack` term keeps the primary cone mask and the
    sky verdict sound."""
    cam = scenes.make_camera(W, H, 500.0 / W)
    if far:
        e, look = np.array(cam.eye[:], np.float64), np.array(cam.look_at[:], np.float64)
        dist = float(np.linalg.norm(look - e))
        d = (look - e) / dist
        e = e - FAR_BACK * d
        cam.eye[:] = [float(v) for v in e]
        cam.look_at[:] = [float(v) for v in e + FAR_LOOK * d]
        cam.pitch = cam.pitch * FAR_LOOK / (FAR_BACK + dist)
    if eye is not None:
        cam.eye[:] = [float(v) for v in eye]
    return cam


def scene_position(scene):
    return np.array(scene.to_abi().position[:], np.float64)


def with_blocker(base, where, world_centre, radius):
    """`base` with the blocker as one more sphere — where: "last" (appended), "first" (index 0, the others shifted) or
    "replace_last" (instead of the last sphere) — centred at world_centre (stored scene-local: world minus the scene's
    position).  -> (scenes.Scene, blocker index); the Scene keeps the arrays of its to_abi() alive."""
    local = np.array(world_centre, np.float64) - scene_position(base)
    blk = FreeSphere("a1", float(radius), 0.0, tuple(local))
    sph = list(base.spheres)
    if where == "last":
        sph, idx = sph + [blk], len(sph)
    elif where == "first":
        sph, idx = [blk] + sph, 0
    elif where == "replace_last":
        sph, idx = sph[:-1] + [blk], len(sph) - 1
    else:
        raise KeyError(where)
    return dataclasses.replace(base, spheres=sph), idx


def centres_radii(scene):
    """Scene-local centres [n, 3] and radii [n] (po.ref_trace_rays_at / po.ref_intersect_at)."""
    return (np.array([sp.center() for sp in scene.spheres], np.float64).reshape(-1, 3),
            np.array([sp.radius for sp in scene.spheres], np.float64))


# ------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    kind: str            # "primary", "shadow", "reflection"
    i: int               # the target pixel
    j: int
    behind: str          # what the pixel's primary ray hits in the base frame: SKY, BOARD, SPHERE
    p: tuple             # the target ray: origin, unit direction, the unit normal the blocker stands on
    u: tuple
    n: tuple
    end: tuple           # the ray as the reference takes it, Line(p, end)
    t: float
    r: float
    light: int = -1      # shadow cases: the light's index

    @property
    def lane(self):
        return (self.j % 8) * 8 + self.i % 8

    def centre(self, pen):
        p, u, n = (np.array(v, np.float64) for v in (self.p, self.u, self.n))
        return (p + np.float64(self.t) * u) + (np.float64(self.r) * (1.0 - np.float64(pen))) * n

    def label(self):
        return f"{self.kind} px({self.i},{self.j}) lane {self.lane} {self.behind} t={self.t:.4g} r={self.r:g}"


def _unit(v):
    v = np.array(v, np.float64)
    return v / np.sqrt((v * v).sum())


def _perp(u, variant):
    """A unit vector orthogonal to u; variant 0..3 turns it by quarter turns about u."""
    e = np.zeros(3)
    e[int(np.argmin(np.abs(u)))] = 1.0
    a = _unit(np.cross(u, e))
    b = _unit(np.cross(u, a))
    return (a, b, -a, -b)[variant % 4]


@functools.lru_cache(maxsize=None)
def base_frame(name, far=False):
    """The oracle on the base scene: screen points, and what every pixel's primary ray hits."""
    sc = base_scene(name)
    sa = sc.to_abi()
    cam = camera(far=far)
    sp = po.screen_points(cam, W, H)
    eye = np.array(cam.eye[:], np.float64)
    h = po.intersect(sa, np.tile(eye, (W * H, 1)), sp.reshape(-1, 3))
    hit = h["hit"].reshape(H, W) != 0
    mat = h["material"].reshape(H, W)
    what = np.full((H, W), SKY, dtype=object)
    what[hit & (mat < 2)] = BOARD
    what[hit & (mat >= 2)] = SPHERE
    out = {"scene": sc, "sa": sa, "cam": cam, "eye": eye, "sp": sp, "what": what, "point": h["point"].reshape(H, W, 3),
           "reflected_end": h["reflected_end"].reshape(H, W, 3), "bc": np.array(sa.position[:], np.float64),
           "R": float(sa.radius), "lights": [np.array(sa.lights[k].position[:], np.float64) for k in range(sa.n_lights)]}
    return out


def _tiles():
    """The frame's tiles in a fixed scattered order, so the cases spread over the frame."""
    tl = [(tx, ty) for ty in range(H // 8) for tx in range(W // 8)]
    return sorted(tl, key=lambda t: ((t[0] * 5 + t[1] * 3) % 7, t[0], t[1]))


def _pixel(tile, lane):
    return tile[0] * 8 + lane % 8, tile[1] * 8 + lane // 8


def _inside_t(f, p, u, n, r, t_max):
    """The smallest parameter t (of 33 tried) at which the blocker lies inside the scene's bounding sphere and ends
    before t_max, or None."""
    dP = f["bc"] - p
    uD = float(u @ dP)
    disc = uD * uD - float(dP @ dP) + f["R"] ** 2
    if disc <= 0.0:
        return None
    lo = max(uD - np.sqrt(disc), 2.0 * r) + r
    hi = min(uD + np.sqrt(disc), t_max - 1.5 * r)
    for t in np.linspace(lo, hi, 33) if hi > lo else ():
        c = p + t * u + r * n
        if np.linalg.norm(c - f["bc"]) + r <= f["R"] - 1.0:
            return float(t)
    return None


def _primary_case(f, tile, lane, r):
    i, j = _pixel(tile, lane)
    behind = f["what"][j, i]
    if behind == SPHERE:
        return None
    p, end = f["eye"], f["sp"][j, i]
    u = _unit(end - p)
    x0, y0 = tile[0] * 8, tile[1] * 8
    centre = 0.25 * (f["sp"][y0, x0] + f["sp"][y0, x0 + 7] + f["sp"][y0 + 7, x0] + f["sp"][y0 + 7, x0 + 7])
    m = end - centre
    n = _unit(m - (m @ u) * u)
    t_max = np.linalg.norm(f["point"][j, i] - p) if behind == BOARD else np.inf
    t = _inside_t(f, p, u, n, r, t_max)
    if t is None:
        return None
    return Case("primary", i, j, behind, tuple(p), tuple(u), tuple(n), tuple(end), t, r)


@functools.lru_cache(maxsize=None)
def primary_cases(name, far=False):
    """Per lane (the four corners and an interior one) four sky pixels and four board pixels, r = 5 and 6 in turn: 40
    cases; then r = 20 and r = 150 at lanes 0 and 63."""
    f = base_frame(name, far)
    out = []
    for lane in CORNER_LANES + (INTERIOR_LANE,):
        for behind in (SKY, BOARD):
            got = 0
            for tile in _tiles():
                c = _primary_case(f, tile, lane, 5.0 + (got % 2))
                if c is not None and c.behind == behind:
                    out.append(c)
                    got += 1
                    if got == 4:
                        break
    for lane, r in ((0, 20.0), (63, 20.0), (0, 150.0), (63, 150.0)):
        for tile in _tiles():
            c = _primary_case(f, tile, lane, r)
            if c is not None:
                out.append(c)
                break
    return tuple(out)


def _secondary_pixels(f, lit_by=None):
    """Per corner lane one pixel that hits the board and one that hits a sphere (a second board pixel where no sphere
    lies under that lane of any tile); with lit_by, only pixels the light reaches in the base scene."""
    def usable(i, j):
        if lit_by is None:
            return True
        q = f["point"][j, i]
        return not po.intersect(f["sa"], q[None, :], f["lights"][lit_by][None, :])["hit"][0]

    out = []
    for lane in CORNER_LANES:
        found = {BOARD: [], SPHERE: []}
        for tile in _tiles():
            i, j = _pixel(tile, lane)
            what = f["what"][j, i]
            if what in found and len(found[what]) < 2 and usable(i, j):
                found[what].append((i, j, what))
        out += (found[BOARD][:1] + found[SPHERE][:1] + found[BOARD][1:])[:2]
    return out


@functools.lru_cache(maxsize=None)
def shadow_cases(name, light=0):
    """Eight pixels lit by `light`, the blocker at 0.05, 0.5 and 0.95 of the way to it, r = 5 and 6 in turn: 24 cases;
    then r = 0.5 next to the hit (twice), r = 20 and r = 150 mid-way."""
    f = base_frame(name)
    L = f["lights"][light]
    out = []
    px = _secondary_pixels(f, light)
    for k, (i, j, behind) in enumerate(px):
        q = f["point"][j, i]
        u = _unit(L - q)
        dist = float(np.linalg.norm(L - q))
        for m, frac in enumerate((0.05, 0.5, 0.95)):
            out.append(Case("shadow", i, j, behind, tuple(q), tuple(u), tuple(_perp(u, k + m)), tuple(L), frac * dist,
                            5.0 + ((k + m) % 2), light))
    for k, (frac, r) in enumerate(((0.05, 0.5), (0.05, 0.5), (0.5, 20.0), (0.5, 150.0))):
        i, j, behind = px[(3 * k) % len(px)]
        q = f["point"][j, i]
        u = _unit(L - q)
        out.append(Case("shadow", i, j, behind, tuple(q), tuple(u), tuple(_perp(u, k + 1)), tuple(L),
                        frac * float(np.linalg.norm(L - q)), r, light))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reflection_cases(name):
    """Eight pixels, the blocker on the reflected ray at t = 5, 30 and 150, r = 5 and 6 in turn: 24 cases; then
    r = 0.5 at t = 5 (twice) and r = 20 at t = 30."""
    f = base_frame(name)
    out = []
    px = _secondary_pixels(f)
    for k, (i, j, behind) in enumerate(px):
        q, end = f["point"][j, i], f["reflected_end"][j, i]
        u = _unit(end - q)
        for m, t in enumerate((5.0, 30.0, 150.0)):
            out.append(Case("reflection", i, j, behind, tuple(q), tuple(u), tuple(_perp(u, k + m)), tuple(end), t,
                            5.0 + ((k + m) % 2)))
    for k, (t, r) in enumerate(((5.0, 0.5), (5.0, 0.5), (30.0, 20.0))):
        i, j, behind = px[(3 * k + 1) % len(px)]
        q, end = f["point"][j, i], f["reflected_end"][j, i]
        u = _unit(end - q)
        out.append(Case("reflection", i, j, behind, tuple(q), tuple(u), tuple(_perp(u, k + 2)), tuple(end), t, r))
    return tuple(out)


DEPTH = {"primary": 1, "shadow": 1, "reflection": 2}


def cases(name, kind, light=0):
    if kind == "primary":
        return primary_cases(name)
    if kind == "shadow":
        return shadow_cases(name, light)
    return reflection_cases(name)


def target_pixel(name, case, pen, depth=None, where="last", far=False):
    """The oracle's colour and ray counter of the case's pixel with the blocker at `pen` -> bytes."""
    f = base_frame(name, far)
    sc, _ = with_blocker(f["scene"], where, case.centre(pen), case.r)
    rgb, rc = po.trace_rays(sc.to_abi(), f["eye"][None, :], f["sp"][case.j, case.i][None, :],
                            DEPTH[case.kind] if depth is None else depth)
    return rgb.tobytes() + rc.tobytes()


def is_sensitive(pixel_of):
    """pixel_of(pen) -> bytes: the sensitivity condition of the module docstring."""
    out = pixel_of(-1e-3)
    return pixel_of(1e-12) != out and all(pixel_of(pen) == out for pen in PENS if pen < 0)


@functools.lru_cache(maxsize=None)
def kept(name, kind, light=0, where="last"):
    """The sensitive cases of cases(name, kind, light) in the scene with the blocker placed `where` (the scene a test
    renders: "replace_last" has one sphere fewer), and the number constructed; prints the counts."""
    every = cases(name, kind, light)
    keep = tuple(c for c in every if is_sensitive(functools.lru_cache(maxsize=None)(
        lambda pen, c=c: target_pixel(name, c, pen, where=where))))
    print(f"tangent cases {name}-{where} {kind}{'' if kind != 'shadow' else f' light {light}'}: "
          f"{len(keep)} of {len(every)} sensitive")
    return keep, len(every)


@functools.lru_cache(maxsize=None)
def kept_far(name):
    """The primary cases of the far camera whose pixel differs between pen = +1e-3 and -1e-3.  (From 3e4 away the
    oracle's own rounding of the discriminant, 2^-52 |dP|^2, is a dip of about 1e-8 r: the rungs below that fall
    either way, and are compared like any other.)"""
    every = primary_cases(name, True)
    keep = tuple(c for c in every if target_pixel(name, c, 1e-3, far=True) != target_pixel(name, c, -1e-3, far=True))
    print(f"tangent cases {name} primary, far camera: {len(keep)} of {len(every)} sensitive")
    return keep, len(every)


# ------------------------------------------------------------------------------------------- board-edge eyes
def _pixel_hits(sa, eye, i, j):
    """-> (hit, material) of pixel (i, j) seen from `eye`."""
    cam = camera(eye)
    sp = po.screen_points(cam, W, H)[j, i]
    h = po.intersect(sa, np.array(eye, np.float64)[None, :], sp[None, :])
    return int(h["hit"][0]), int(h["material"][0])


def _ulps(x, k):
    """The double k places above x in value (below it for k < 0); x != 0, no sign change."""
    v = np.array([x], np.float64).view(np.int64)
    return float((v + (k if x > 0 else -k)).view(np.float64)[0])


@functools.lru_cache(maxsize=None)
def board_edge_eyes(name):
    """For tile-corner pixels that hit the board near an edge: one eye coordinate (x, or y for a pixel with a sky pixel
    above or below it) bisected between the canonical eye, from which the pixel hits the board, and a moved eye from
    which it misses everything, until the two are adjacent doubles.  -> a list of (i, j, axis, eyes): both eyes and the
    eyes 2^10 and 2^20 doubles either side, six eyes; one case per corner lane and axis where the frame has one."""
    f = base_frame(name)
    sa = f["sa"]
    out = []
    for lane in CORNER_LANES:
        for axis in (0, 1):
            for tile in _tiles():
                i, j = _pixel(tile, lane)
                if f["what"][j, i] != BOARD:
                    continue
                # (y: a pixel of the board's first or last row in the frame; x: any — the frame's tile corners miss the
                # board's slanted sides, and the bisection finds the edge the moving eye pushes the pixel across)
                if axis == 1 and not any(0 <= j + dj < H and f["what"][j + dj, i] == SKY for dj in (-1, 1)):
                    continue
                eyes = _bisect_eye(sa, f["eye"], i, j, axis)
                if eyes is not None:
                    out.append((i, j, axis, eyes))
                    break
    return out


def _bisect_eye(sa, eye0, i, j, axis):
    def eye_at(v):
        e = np.array(eye0, np.float64)
        e[axis] = v
        return e

    def on_board(v):
        hit, mat = _pixel_hits(sa, eye_at(v), i, j)
        return hit != 0 and mat < 2, hit == 0

    a = b = None
    for step in (1, 2, 4, 8, 16, 32, 64, 128):
        for s in (step, -step):
            # (the canonical eye has x = 0: start one step of 2^-20 beside it, on the side the eye moves to, so the
            # bisection never crosses zero)
            a0 = float(eye0[axis]) if eye0[axis] != 0.0 else np.copysign(2.0 ** -20, s)
            if (a0 + s > 0) == (a0 > 0) and on_board(a0)[0] and on_board(a0 + s)[1]:
                a, b = a0, a0 + s
                break
        if b is not None:
            break
    if b is None:
        return None
    for _ in range(80):
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        board, miss = on_board(m)
        if board:
            a = m
        elif miss:
            b = m
        else:
            return None                                  # (a sphere comes between: not a board-to-sky transition)
    if abs(np.array([a]).view(np.int64)[0] - np.array([b]).view(np.int64)[0]) != 1:
        return None
    out = [a, b]
    up = 1 if a > b else -1                              # a lies this way from b, by value
    for k in (2 ** 10, 2 ** 20):
        out += [_ulps(a, up * k), _ulps(b, -up * k)]
    return [tuple(eye_at(v)) for v in out]


# -------------------------------------------------------------------------------------------- ray lists, far origins
FAR_SPEC = ("e4", 60.0)                                # the blocker's board square and y offset: above the board,
                                                       # clear of the other spheres, and a place the reference harness
                                                       # can put a sphere by square
FAR_SCALES = (1e3, 1e5, 3e6)                           # distances of the ray origins (sphere_reject32's S term)
FAR_RADII = (0.5, 20.0, 150.0)


def far_spec(r):
    return scenes.SphereSpec(FAR_SPEC[0], float(r), FAR_SPEC[1])


def far_centre():
    """World centre of far_spec()."""
    return np.array(far_spec(1.0).center(), np.float64) + scene_position(base_scene("c3"))


def tangent_rays(centre, r, scale, n_dirs=12, seed=0):
    """Rays tangent, by the ladder, to the sphere (centre, r) from origins at distance `scale` from the tangent point,
    pointed back at it: -> (starts, ends) [n_dirs * len(PENS), 3].  The ray of direction u and normal n passes through
    T = centre - r (1 - pen) n and is given as Line(T - scale u, T): the direction the tracers recompute from the two
    points then carries one rounding of the far origin's coordinates, not `scale` of them."""
    rng = np.random.default_rng(seed)
    centre = np.array(centre, np.float64)
    starts, ends = [], []
    for k in range(n_dirs):
        u = _unit(rng.normal(size=3))
        n = _perp(u, k)
        for pen in PENS:
            T = centre - (np.float64(r) * (1.0 - np.float64(pen))) * n
            p = T - np.float64(scale) * u
            starts.append(p)
            ends.append(T)
    return np.array(starts), np.array(ends)


# ----------------------------------------------------------------------------------------------------- motion
MOTION_W = MOTION_H = 16
MOTION_S, MOTION_F = 2, 1.0
MOTION_PIXELS = ((5, 11, 5.0), (8, 11, 6.0), (11, 12, 20.0))      # (i, j, r): sky pixels above the board's far edge


def motion_camera():
    return scenes.make_camera(MOTION_W, MOTION_H, 500.0 / MOTION_W)


def motion_case(i, j, a, b, r, pen):
    """c2 with a moving blocker tangent, by `pen`, to the primary ray of sample (a, b) of pixel (i, j) at that sample's
    own time sigma (motion_common.time_of): it stands on the side n of the ray and moves by d = -sign(sigma) 8 r n, so
    sigma is the end of its sweep nearest the ray and every other time sees it further away.
    -> (scene with the blocker last, displacement [n_spheres, 3])."""
    S = MOTION_S
    starts, ends = dc.rays(motion_camera(), MOTION_W, MOTION_H, S, 0.0)
    p, end = starts[S * j + b, S * i + a], ends[S * j + b, S * i + a]
    u = _unit(end - p)
    n = _perp(u, a + b)
    sigma = float(mc.time_of(S, MOTION_F, a, b))
    d = -np.sign(sigma) * 8.0 * r * n
    t = float(np.linalg.norm(np.array([0.0, 40.0, -160.0]) - p))        # abreast of the board's centre
    at_sigma = (p + t * u) + (np.float64(r) * (1.0 - np.float64(pen))) * n
    sc, idx = with_blocker(base_scene("c2"), "last", at_sigma - sigma * d, r)
    disp = np.zeros((len(sc.spheres), 3))
    disp[idx] = d
    return sc, disp


def motion_pixel(i, j, a, b, r, pen):
    """The oracle route's value and counters of pixel (i, j) of the motion frame -> bytes."""
    sc, disp = motion_case(i, j, a, b, r, pen)
    e = mc.render(sc, motion_camera(), MOTION_W, MOTION_H, 1, MOTION_S, 0.0, 0.0, MOTION_F, disp)
    return e["rgb"][j, i].tobytes() + e["rc2"][j, i].tobytes()
