"""Scene descriptors: the reference's g_scene built from the same inputs the app uses, plus the canonical
benchmark scenes of SURVEY.md Appendix B.

A :class:`Scene` mirrors what ``loadScene`` / ``initScene2`` produce in the reference
(/root/reference/Hw4/MySdlApplication.cpp:1430-1539): a CheckerBoard inserted first, then spheres in
order, and the per-frame light list ``draw()`` builds (:1552-1554).  Every coordinate comes from the C
ABI's host helpers (rt_convert_string_coordinate, rt_light_position_from_square), which restate
``convertStringCoordinate`` (:1326-1346) with the reference's operation order.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from . import abi

# Enum of the reference (MySdlApplication.cpp:16).
LIGHT, TETRAHEDRON, CUBE, SPHERE, CYLINDER, CONE = range(6)

WHITE = (1.0, 1.0, 1.0)
GREY = (0.5, 0.5, 0.5)
SQUARES_8 = ("d7", "b2", "f5", "h8", "c4", "e2", "g6", "a5")


def convert_string_coordinate(square: str) -> Tuple[float, float, float]:
    out = (ctypes.c_double * 3)()
    abi.check(abi.lib().rt_convert_string_coordinate(square.encode(), out), "rt_convert_string_coordinate")
    return tuple(out)


def light_position_from_square(square: str) -> Tuple[float, float, float]:
    out = (ctypes.c_double * 3)()
    abi.check(abi.lib().rt_light_position_from_square(square.encode(), out), "rt_light_position_from_square")
    return tuple(out)


@dataclass
class SphereSpec:
    square: str
    radius: float
    y_offset: float = 0.0     # added as Point(0, y_offset, 0) after convertStringCoordinate

    def center(self) -> Tuple[float, float, float]:
        x, y, z = convert_string_coordinate(self.square)
        # Point + Point(0.0, y_offset, 0.0): same additions as the reference operator+ (:196-197)
        return (x + 0.0, y + self.y_offset, z + 0.0)


@dataclass
class LightSpec:
    square: Optional[str]          # None: g_lightPosition's default (0,0,0) (:573), as with no light entry
    color: Tuple[float, float, float] = WHITE

    def position(self) -> Tuple[float, float, float]:
        if self.square is None:
            return (0.0, 0.0, 0.0)
        return light_position_from_square(self.square)


@dataclass
class MeshSpec:
    """Tetrahedron(p, edge) / Cube(p, edge) at convertStringCoordinate(square) (MySdlApplication.cpp:863-950),
    placed in g_scene's child list after `after_spheres` spheres."""
    kind: int                      # abi.RT_MESH_TETRAHEDRON / abi.RT_MESH_CUBE
    square: str
    after_spheres: int = 0
    edge: float = 40.0             # SQUARE_EDGE_SIZE, as loadScene/initScene use


@dataclass
class Scene:
    """A g_scene: board (first child) + spheres and meshes, and the light list of one frame."""
    spheres: List[SphereSpec] = field(default_factory=list)
    lights: List[LightSpec] = field(default_factory=list)
    has_board: bool = True
    meshes: List[MeshSpec] = field(default_factory=list)
    # material overrides: index (MATERIALS order) -> (ambient, diffuse, specular, transparency, refraction);
    # the others keep the reference's globals (MySdlApplication.cpp:583-588)
    materials: Optional[Dict[int, tuple]] = None
    _keep: list = field(default_factory=list, repr=False)

    def to_abi(self) -> abi.rt_scene:
        L = abi.lib()
        s = abi.rt_scene()
        abi.check(L.rt_scene_init_reference(ctypes.byref(s)), "rt_scene_init_reference")
        s.has_board = 1 if self.has_board else 0
        ns, nl = len(self.spheres), len(self.lights)
        sph = (abi.rt_sphere * max(ns, 1))()
        for k, sp in enumerate(self.spheres):
            sph[k].center = abi.vec3(sp.center())
            sph[k].radius = float(sp.radius)
        lts = (abi.rt_light * max(nl, 1))()
        for k, lt in enumerate(self.lights):
            lts[k].color = abi.vec3(lt.color)
            lts[k].position = abi.vec3(lt.position())
        nm = len(self.meshes)
        msh = (abi.rt_mesh * max(nm, 1))()
        for k, m in enumerate(self.meshes):
            msh[k].kind = m.kind
            msh[k].after_spheres = m.after_spheres
            msh[k].position = abi.vec3(convert_string_coordinate(m.square))
            msh[k].edge = float(m.edge)
        for k, m in (self.materials or {}).items():
            mat = getattr(s, MATERIALS[k])
            amb, dif, spe, tra, refr = m
            mat.ambient, mat.diffuse, mat.specular = abi.vec3(amb), abi.vec3(dif), abi.vec3(spe)
            mat.transparency, mat.refraction = abi.vec3(tra), float(refr)
        s.n_spheres, s.n_lights, s.n_meshes = ns, nl, nm
        s.spheres = ctypes.cast(sph, ctypes.POINTER(abi.rt_sphere))
        s.lights = ctypes.cast(lts, ctypes.POINTER(abi.rt_light))
        s.meshes = ctypes.cast(msh, ctypes.POINTER(abi.rt_mesh))
        self._keep = [sph, lts, msh]     # keep the arrays alive as long as the Scene
        return s

    def children(self) -> List[Tuple[str, int]]:
        """g_scene child order after the board: ('S', k) spheres and ('M', m) meshes."""
        out, m = [], 0
        for k in range(len(self.spheres) + 1):
            while m < len(self.meshes) and self.meshes[m].after_spheres <= k:
                out.append(("M", m))
                m += 1
            if k < len(self.spheres):
                out.append(("S", k))
        out.extend(("M", i) for i in range(m, len(self.meshes)))
        return out

    def material_values(self) -> List[float]:
        """The five materials as 5 x 13 doubles (ambient, diffuse, specular, transparency, refraction), the
        layout of oracle/ref_harness.cpp's ref_set_materials."""
        s = self.to_abi()
        out: List[float] = []
        for name in MATERIALS:
            m = getattr(s, name)
            out += list(m.ambient) + list(m.diffuse) + list(m.specular) + list(m.transparency) + [m.refraction]
        return out

    # the reference harness (oracle/_ref) rebuilds the same scene from the reference's own classes
    def ref_args(self):
        if not self.has_board:
            raise ValueError("the reference harness always inserts the board")
        ns, nl, nm = len(self.spheres), len(self.lights), len(self.meshes)
        toks = []
        for kind, i in self.children():
            if kind == "S":
                toks.append("S" + self.spheres[i].square)
            else:
                m = self.meshes[i]
                toks.append(("T" if m.kind == abi.RT_MESH_TETRAHEDRON else "C") + m.square)
        children = "".join(toks).encode()
        yoff = (ctypes.c_double * max(ns, 1))(*[sp.y_offset for sp in self.spheres])
        rad = (ctypes.c_double * max(ns, 1))(*[sp.radius for sp in self.spheres])
        edges = (ctypes.c_double * max(nm, 1))(*[m.edge for m in self.meshes])
        if any(lt.square is None for lt in self.lights):
            raise ValueError("the reference harness places lights by square")
        lsq = "".join(lt.square for lt in self.lights).encode()
        lcol = (ctypes.c_double * max(3 * nl, 1))(*[c for lt in self.lights for c in lt.color])
        return (children, len(toks), yoff, rad, edges, lsq, lcol, nl)


# rt_scene material fields in the reference's global order (g_whiteSquare, g_blackSquare, g_sphereMaterial,
# g_tetrahedronMaterial, g_cubeMaterial: MySdlApplication.cpp:583-588)
MATERIALS = ("white_square", "black_square", "sphere_material", "tetrahedron_material", "cube_material")


def load_scene(entries: Sequence[Tuple[str, int]]) -> Scene:
    """loadScene semantics (MySdlApplication.cpp:1495-1539) via the C ABI: later duplicates win, entries
    are visited in std::map<string> order, the last light wins, one white light.  Cylinders / cones raise
    RtError(RT_EUNSUPPORTED) (reference stubs)."""
    L = abi.lib()
    n = len(entries)
    squares = (ctypes.c_char_p * max(n, 1))(*[e[0].encode() for e in entries])
    types = (ctypes.c_int32 * max(n, 1))(*[int(e[1]) for e in entries])
    s = abi.rt_scene()
    buf = (abi.rt_sphere * max(n, 1))()
    mbuf = (abi.rt_mesh * max(n, 1))()
    light = abi.rt_light()
    abi.check(L.rt_load_scene(squares, types, n, ctypes.byref(s), buf, max(n, 1), mbuf, max(n, 1),
                              ctypes.byref(light)), "rt_load_scene")
    board = {}
    for sq, t in entries:
        board[sq] = t
    spheres, meshes, lights_sq = [], [], []
    for sq in sorted(board):                 # std::map<string> order = byte order of the 2-char keys
        t = board[sq]
        if t == SPHERE:
            spheres.append(SphereSpec(sq, 20.0))
        elif t in (TETRAHEDRON, CUBE):
            meshes.append(MeshSpec(abi.RT_MESH_TETRAHEDRON if t == TETRAHEDRON else abi.RT_MESH_CUBE, sq,
                                   after_spheres=len(spheres)))
        elif t == LIGHT:
            lights_sq.append(sq)
    # draw() always pushes one light; with no light entry g_lightPosition keeps its default (0,0,0)
    scene = Scene(spheres=spheres, lights=[LightSpec(lights_sq[-1] if lights_sq else None)], meshes=meshes)
    scene._abi_loaded = (s, buf, mbuf, light)
    return scene


@dataclass(frozen=True)
class Config:
    name: str
    width: int
    height: int
    n_spheres: int
    n_lights: int
    depth: int
    gpus: int = 1

    @property
    def pitch(self) -> float:
        return 500.0 / self.width          # canonical framing

    def scene(self) -> Scene:
        if self.name == "demo":
            # initScene (MySdlApplication.cpp:1387-1428): board, tetrahedron b4, sphere d7 (r 20), cube a7
            return Scene(spheres=[SphereSpec("d7", 20.0)], lights=[LightSpec("b6", WHITE)],
                         meshes=[MeshSpec(abi.RT_MESH_TETRAHEDRON, "b4", 0), MeshSpec(abi.RT_MESH_CUBE, "a7", 1)])
        if self.n_spheres == 64:
            sph = [SphereSpec(chr(ord("a") + r) + chr(ord("1") + c), 10.0, float(((r + c) % 3) * 25))
                   for r in range(8) for c in range(8)]
        else:
            sph = [SphereSpec(sq, 20.0) for sq in SQUARES_8[: self.n_spheres]]
        lights = [LightSpec("b6", WHITE), LightSpec("g3", GREY)][: self.n_lights]
        return Scene(spheres=sph, lights=lights)

    def camera(self, width: Optional[int] = None, height: Optional[int] = None) -> abi.rt_camera:
        """draw()'s camera; for a reduced-resolution render the pitch follows 500/width."""
        w = width or self.width
        h = height or self.height
        return make_camera(w, h, 500.0 / w)


def make_camera(width: int, height: int, pitch: float) -> abi.rt_camera:
    cam = abi.rt_camera()
    abi.check(abi.lib().rt_camera_init_reference(ctypes.byref(cam), width, height, float(pitch)),
              "rt_camera_init_reference")
    return cam


def focus_camera(cam: abi.rt_camera, ratio: float) -> abi.rt_camera:
    """rt_camera_focus: `cam` with its focal plane (the plane through look_at, for Tracer.render_dof) at `ratio`
    times its distance from the eye and the pitch scaled with it, so the view is the same."""
    out = abi.rt_camera()
    abi.check(abi.lib().rt_camera_focus(ctypes.byref(cam), float(ratio), ctypes.byref(out)), "rt_camera_focus")
    return out


# BASELINE.json configs (SURVEY.md §8 shorthand)
CONFIGS = {
    "c1": Config("c1", 640, 480, 3, 1, 0),
    "c2": Config("c2", 1920, 1080, 8, 1, 1),
    "c3": Config("c3", 3840, 2160, 8, 2, 2),
    "c4": Config("c4", 3840, 2160, 8, 2, 2, gpus=8),
    "c5": Config("c5", 7680, 4320, 64, 2, 3, gpus=8),
    # the reference app's own demo frame: initScene's objects, 500x500 window, unit pitch, MAX_DEPTH 5
    "demo": Config("demo", 500, 500, 1, 1, 5),
}

# Ray-tree scenes (tests only): a material that both transmits and reflects makes rayTraceRay recurse into
# two children per hit (MySdlApplication.cpp:1238-1247).  The app's own materials never do; these override
# the reference's material globals (the reference build's harness sets the same values: ref_set_materials).
GLASS = ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (1.0, 1.0, 1.0), (0.4, 0.3, 0.2), 1.3)
TREE_CASES = {
    # name: (base config, material overrides, depth, full-size frame for the fixtures' hash)
    "tree_c2": ("c2", {2: GLASS}, 3, (1920, 1080)),
    "tree_demo": ("demo", {3: ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (0.5, 0.5, 0.5), 2.0 / 3.0)}, 5,
                  (500, 500)),
    "tree_c3": ("c3", {0: ((0.1, 0.1, 0.1), (0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (0.25, 0.25, 0.25), 1.0),
                       2: ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (1.0, 1.0, 1.0), (0.6, 0.6, 0.6), 1.5)}, 4, (1280, 720)),
}


def tree_case(name: str):
    """-> (scene, config, depth, (W, H)) of a TREE_CASES entry."""
    base, mats, depth, wh = TREE_CASES[name]
    cfg = CONFIGS[base]
    sc = cfg.scene()
    sc.materials = dict(mats)
    return sc, cfg, depth, wh


# Pinned actual-traced ray counts (from the reference's rayTraceRay)
PINNED_RAYS = {"c1": 380_817, "c2": 3_684_271, "c3": 18_956_255, "c5": 90_722_787,
               # the demo frame is not in SURVEY.md; pinned by the restatement, which matches the reference
               # build bit for bit on this frame (tests/test_oracle.py)
               "demo": 358_434}


def camera_motion(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, 0.0)) -> abi.rt_camera_motion:
    """The half-extents of a camera's move during the exposure (Tracer.render_shutter): at shutter time sigma in
    (-1, 1) the eye is at cam.eye + sigma * eye and looks at cam.look_at + sigma * look_at."""
    m = abi.rt_camera_motion()
    m.eye, m.look_at = abi.vec3(eye), abi.vec3(look_at)
    return m


def camera_at(cam: abi.rt_camera, motion: Optional[abi.rt_camera_motion], sigma: float) -> abi.rt_camera:
    """rt_camera_at: the camera of Tracer.render_shutter's samples at shutter time `sigma`."""
    out = abi.rt_camera()
    abi.check(abi.lib().rt_camera_at(ctypes.byref(cam), ctypes.byref(motion) if motion is not None else None,
                                     float(sigma), ctypes.byref(out)), "rt_camera_at")
    return out


def rows(band_height: int = 1, n_ranks: int = 1, rank: int = 0, frames: int = 1) -> abi.rt_rows:
    r = abi.rt_rows()
    r.band_height, r.n_ranks, r.rank, r.frames = band_height, n_ranks, rank, frames
    return r


def local_rows(height: int, r: Optional[abi.rt_rows]) -> int:
    out = ctypes.c_int()
    abi.check(abi.lib().rt_local_rows(height, ctypes.byref(r) if r is not None else None, ctypes.byref(out)),
              "rt_local_rows")
    return out.value
