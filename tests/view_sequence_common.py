"""Seeded call sequences on one long-lived context (tests/test_view_sequence.py on the CPU, tests/test_gpu_view_sequence.py
on the GPU): the vocabulary of steps, the generator, a restatement of the view cache's documented rule (rt_ctx.hpp, the
comments of rt_plain.hip render_plan_view) as a host-side Model, the oracle's expectation of every step, and the
comparison of a step's outputs with it.

A step is a plain dict (JSON-able, so that a sequence has a digest).  Every rendering step carries its whole view:
  op      render | render_ss | render_packed | render_adaptive | render_host      (the calls that share the view key)
          motion | jitter | lens_adaptive                                         (the calls that promise to touch no view state)
          capture | replay                                                        (a plain render captured into a graph)
  scene   the scene in force (set by the last set_scene step), size [W, H], cam (a name of CAMS) made for the frame
          size cam_size (the frame's own, or after a change of the size alone the earlier frame's), depth,
          rows [band, ranks, rank, frames] or None, outs (a name of OUTSETS), fmt (render_packed's byte format:
          "native" GRAY8 / RGB8, or "rgba8"), stream 0 (the null stream), 1 or 2 (side streams)
and the others are {"op": "set_scene", "scene": name} (an equal scene is rt_set_scene's no-op) and {"op": "tile_order"}
(rt_diag_tile_order 1, then 0 again).

Nothing here calls the code under test except host-only helpers (rt_camera_supersample, rt_local_rows,
rt_scene_achromatic, rt_diag_sky_tiles).  Expectations come from the CPU oracle through the functions the other tests
already share (ssaa_common, adaptive_common, motion_common, jitter_common, lens_adaptive_common): no second oracle.
"""
import ctypes
import functools
import hashlib
import json

import numpy as np

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes

from . import adaptive_common as ac
from . import jitter_common as jc
from . import lens_adaptive_common as la
from . import motion_common as mc
from . import sky_common as sk
from . import ssaa_common as sc

BELOW, STEEP = (0.0, -50.0, 200.0), (0.0, 300.0, 10.0)      # the eyes of test_sky_tiles.py: under the board, steeply above

# ---- the vocabulary ----------------------------------------------------------------------------------------------------
SCENES = ("c2", "rise", "c5", "c1", "demo", "tree_demo")
# 64x40 and 61x37 are both 8 x 5 tiles; 160x96 has 240 tiles and grows the per-tile buffers; 128x80 is the sample grid
# of a 64x40 frame with S = 2 (a plain render of it differs from the supersampled one in the key's sample count alone)
SIZES = ((64, 40), (61, 37), (72, 40), (33, 17), (160, 96), (128, 80))
EYE_FIXED = ("look_a", "look_b", "up", "up_b", "pitch_half", "pitch_double", "bottom_x", "bottom_y_minus", "bottom_y_plus")
MOVED = ("orbit3", "below", "steep")
CAMS = ("base",) + EYE_FIXED + MOVED
DEPTHS = (0, 1, 2, 3, 5)
ROWS = (None, (8, 2, 0, 1), (8, 2, 1, 1), (5, 3, 1, 1), (8, 2, 0, 2))
OUTS = ("rgba32f", "rgba8", "rgb64f", "raycount")
OUTSETS = {"all": (1, 1, 1, 1), "bench": (1, 1, 0, 0), "parity": (0, 0, 1, 1), "bytes": (0, 1, 0, 0)}
VIEW_OPS = ("render", "render_ss", "render_packed", "render_adaptive", "render_host")
SAMPLED_OPS = ("motion", "jitter", "lens_adaptive")
CALL_KINDS = ("render", "render_ss", "render_ss_rows", "render_packed", "render_adaptive", "render_host")
BRANCHES = ("first", "calibration", "cached", "other", "captured")
KEY_FIELDS = ("eye", "look_at", "up", "pitch", "bottom", "size", "depth", "rows", "scene", "outputs", "format", "samples")
CAMERA_FIELDS = ("eye", "look_at", "up", "pitch", "bottom")
DISCRIMINATING_FIELDS = ("eye", "look_at", "up", "pitch", "bottom", "scene", "rows")
SS = 2                      # render_ss and render_adaptive: samples per axis
ADAPTIVE_T = 8
LENS = dict(S=2, J=4, seed=7, A=2.0, R=10.0, F=1.0, lo=1, hi=2, T=8)      # the sampled calls' arguments
SENTINEL = 0xA5
REPLAY_AFTER = 3            # a graph is replayed at least this many steps after its capture

# the committed sequences: test -> seeds (all of 48 steps).  The seeds were chosen, among the 300 from 101, 201, 301 and
# 401 on whose sequence meets the per-seed branch floors of test_view_sequence.py (about one in six does), so that
# together they meet its floors with some room; that test pins their digests and holds the floors.
STEPS = 48
SEEDS = {"sequence": (117, 219, 245, 326, 364, 372), "bursts": (438, 458), "moving_order": (360, 471),
         "tile_order_policy": (511,)}
MOVING_KNOBS = dict(moving_order=True, recalibrate=3)

_MOVES = dict(mc.MOVES, rise=mc.MOVES["c2"], c1=((0, (0.0, 12.0, -30.0)),))


@functools.lru_cache(maxsize=None)
def scene_pair(name):
    """-> (scenes.Scene, its rt_scene): built once, the Scene keeps the record's arrays alive."""
    if name in ("c2", "rise", "c5"):
        s = sk.scene_named(name)
    elif name in scenes.TREE_CASES:
        s = scenes.tree_case(name)[0]
    else:
        s = scenes.CONFIGS[name].scene()
    return s, s.to_abi()


@functools.lru_cache(maxsize=None)
def scene_facts(name):
    """What render_plan_view reads of the uploaded scene -> (padded spheres, lights, opaque, achromatic)."""
    s, s_abi = scene_pair(name)
    a = ctypes.c_int()
    abi.check(abi.lib().rt_scene_achromatic(ctypes.byref(s_abi), ctypes.byref(a)), "rt_scene_achromatic")
    return (len(s.spheres) + 3) // 4 * 4, len(s.lights), not s.meshes and not s.materials, bool(a.value)


def camera_named(name, W, H):
    """The canonical camera of a W x H frame, or one of its variants: the eye-fixed ones change look_at, up, pitch or
    the bottom corner alone; the moved ones the eye alone."""
    cam = sk.camera(W, H)
    if name == "look_a":
        cam.look_at = abi.vec3((cam.look_at[0] + 60.0, cam.look_at[1] + 40.0, cam.look_at[2]))
    elif name == "look_b":
        cam.look_at = abi.vec3((cam.look_at[0], cam.look_at[1] - 60.0, cam.look_at[2]))
    elif name == "up":
        cam.up = abi.vec3((0.5, 1.0, 0.0))
    elif name == "up_b":
        cam.up = abi.vec3((-0.5, 1.0, 0.0))
    elif name == "pitch_half":
        cam.pitch = cam.pitch / 2.0
    elif name == "pitch_double":
        cam.pitch = cam.pitch * 2.0
    elif name == "bottom_x":
        cam.bottom_x += 24
    elif name == "bottom_y_minus":
        cam.bottom_y -= 16
    elif name == "bottom_y_plus":
        cam.bottom_y += 16
    elif name == "orbit3":
        cam.eye = abi.vec3(sk.orbit_eyes()[3])
    elif name == "below":
        cam.eye = abi.vec3(BELOW)
    elif name == "steep":
        cam.eye = abi.vec3(STEEP)
    elif name != "base":
        raise KeyError(name)
    return cam


def rows_of(key):
    return scenes.rows(*key) if key else None


# ---- the generator -----------------------------------------------------------------------------------------------------
_MUTATIONS = (("cam", 0.18), ("size", 0.08), ("depth", 0.06), ("rows", 0.09), ("outs", 0.05), ("op", 0.10), ("fmt", 0.03),
              ("samples", 0.04), ("scene", 0.07), ("scene_again", 0.04), ("sampled", 0.07), ("tile_order", 0.02),
              ("capture", 0.15), ("replay", 0.09), ("stream", 0.02))


def _pick(rng, seq, other_than=()):
    seq = [v for v in seq if v != other_than]
    return seq[int(rng.integers(len(seq)))]


def _tile_rows(H, rows):
    return (scenes.local_rows(H, rows_of(rows)) + 7) // 8


def _normalise(v):
    """The view made one its call accepts: full frames for the adaptive render, one frame for the supersampled one; the
    packed call writes the byte image alone and the host call the FP64 image and the counters (rt_stats)."""
    if v["op"] == "render_adaptive":
        v["rows"] = None
    if v["op"] == "render_ss" and v["rows"] and v["rows"][3] > 1:
        v["rows"] = [v["rows"][0], v["rows"][1], v["rows"][2], 1]
    if v["op"] == "render_packed":
        v["outs"] = "bytes"
    if v["op"] == "render_host":
        v["outs"] = "parity"
    return v


def generate(seed, n=STEPS):
    """A deterministic list of n steps.  Half the steps repeat the previous render (else no view would ever be
    calibrated and rendered from the cache); the others change ONE thing — a camera field, the size, the depth, the row
    plan, the output set, the call, the scene — or put a call between two renders of a view that must leave it alone."""
    rng = np.random.default_rng(seed)
    names, weights = zip(*_MUTATIONS)
    weights = np.array(weights) / sum(weights)
    scene = "c2"
    steps = [{"op": "set_scene", "scene": scene}]
    view = {"op": "render", "scene": scene, "size": [64, 40], "cam_size": [64, 40], "cam": "base", "depth": 1,
            "rows": None, "outs": "all", "fmt": "native", "stream": 0}
    rendered = False
    graphs = []                                     # [slot, step of the capture, view]: replayable while the scene stays
    while len(steps) < n:
        if rendered and rng.random() < 0.5:
            steps.append(dict(view))
            continue
        m = names[int(rng.choice(len(names), p=weights))]
        if m == "scene" or m == "scene_again":
            if m == "scene":
                scene = _pick(rng, SCENES, scene)
                graphs = []                         # (a graph holds the old scene record's kernels and pointers)
            steps.append({"op": "set_scene", "scene": scene})
            view["scene"] = scene
            continue
        if m == "tile_order":
            steps.append({"op": "tile_order"})
            continue
        if m == "sampled":
            steps.append(dict(view, op=_pick(rng, SAMPLED_OPS), rows=None, outs="all"))
            continue
        if m == "capture":
            # (not in the first quarter: once a render was captured every render prepares its eye, and the rule that a
            # render prepares only a new eye would go untested)
            if len(graphs) >= 2 or len(steps) < n // 4:
                continue
            slot = sum(1 for s in steps if s["op"] == "capture")
            cap = dict(view, op="capture", outs="all", slot=slot, stream=int(rng.integers(1, 3)))
            graphs.append([slot, len(steps), cap])
            steps.append(cap)
            continue
        if m == "replay":
            ready = [g for g in graphs if len(steps) - g[1] >= REPLAY_AFTER]
            if not ready:
                continue
            g = ready[int(rng.integers(len(ready)))]
            steps.append(dict(g[2], op="replay"))
            continue
        if m == "cam":
            # one camera field at a time: from the canonical camera to a variant, from a variant back
            # (a third of the variants chosen are the two eyes whose views differ from the canonical one in their sky)
            if view["cam"] != "base" and rng.random() >= 0.3:
                view["cam"] = "base"
            else:
                view["cam"] = _pick(rng, ("below", "steep") if rng.random() < 0.33 else CAMS[1:], view["cam"])
        elif m == "size":
            # the new frame through the old frame's camera (the size alone changes: a crop or a wider window), or with
            # the canonical camera of its own size
            view["size"] = list(_pick(rng, SIZES, tuple(view["size"])))
            if rng.random() < 0.5:
                view["cam_size"] = list(view["size"])
        elif m == "depth":
            view["depth"] = _pick(rng, DEPTHS, view["depth"])
        elif m == "rows":
            # (more often than not to a plan with as many tile rows, where the tile grid does not tell the two apart)
            now = tuple(view["rows"]) if view["rows"] else None
            H = view["size"][1] * (SS if view["op"] == "render_ss" else 1)
            same = [r for r in ROWS if r != now and _tile_rows(H, r) == _tile_rows(H, now)]
            r = _pick(rng, same) if same and rng.random() < 0.6 else _pick(rng, ROWS, now)
            view["rows"] = list(r) if r else None
        elif m == "outs":
            view["outs"] = _pick(rng, tuple(OUTSETS), view["outs"])
        elif m == "op" and view["op"] == "render_packed" and rng.random() < 0.4:
            view["fmt"] = "rgba8" if view["fmt"] == "native" else "native"
        elif m == "op":
            view["op"] = "render_ss" if view["op"] != "render_ss" and rng.random() < 0.4 else _pick(rng, VIEW_OPS, view["op"])
        elif m == "samples":
            # rt_render_dev and the adaptive render's base pass with all four outputs: keys that differ in the sample
            # count's tag alone
            view["op"] = "render_adaptive" if view["op"] == "render" else "render"
            view["outs"] = "all"
        elif m == "fmt":
            if view["op"] == "render_packed":
                view["fmt"] = "rgba8" if view["fmt"] == "native" else "native"
            else:
                view["op"] = "render_packed"
        elif m == "stream":
            view["stream"] = _pick(rng, (0, 1, 2), view["stream"])
        _normalise(view)
        steps.append(dict(view))
        rendered = True
    return steps


def digest(steps):
    return hashlib.sha256(json.dumps(steps, sort_keys=True).encode()).hexdigest()[:16]


def call_kind(step):
    return "render_ss_rows" if step["op"] == "render_ss" and step["rows"] else step["op"]


# ---- what a step asks render_dev_impl for ------------------------------------------------------------------------------
def plan(step):
    """The one render_dev_impl call behind a step, or None (the sampled calls, set_scene, tile_order, replay): a dict of
    the scene's name, the camera, width, height, depth and row plan the call is keyed by (the sample grid's for a
    supersampled render), which outputs it writes (float, byte, FP64, counters), their formats, and the sample count's
    tag in the key (0: a plain instance)."""
    op = step["op"]
    if op not in VIEW_OPS and op != "capture":
        return None
    W, H = step["size"]
    cam = camera_named(step["cam"], *step["cam_size"])
    rows = tuple(step["rows"]) if step["rows"] else None
    outs = OUTSETS[step["outs"]]
    p = {"scene": step["scene"], "cam": cam, "W": W, "H": H, "depth": step["depth"], "rows": rows, "outs": outs,
         "format": ("rgba32f", "rgba8"), "samples": 0, "S": 1, "capturing": op == "capture"}
    if op == "render_ss":
        p.update(cam=sc.camera_ss(cam, SS), W=SS * W, H=SS * H, samples=2, S=SS)       # (tag: log2 S + 1)
        if rows and rows[1] > 1:
            p["rows"] = (rows[0] * SS,) + rows[1:]
    elif op == "render_packed":
        native = "gray8" if scene_facts(step["scene"])[3] else "rgb8"
        p.update(outs=(0, 1, 0, 0), format=("rgba32f", native if step["fmt"] == "native" else "rgba8"))
    elif op == "render_adaptive":
        # the base pass: rt_render_ss_dev with S = 1 — rt_render_dev's instances, or with counters the supersampled
        # ones; its byte image is always written (the caller's, or the workspace's)
        p.update(cam=sc.camera_ss(cam, 1), outs=(outs[0], 1, outs[2], outs[3]), samples=1 if outs[3] else 0)
    elif op == "render_host":
        p.update(outs=(0, 0, 1, 1))
    p["local_rows"] = scenes.local_rows(p["H"], rows_of(p["rows"]))
    p["tiles_x"], p["tiles_y"] = (p["W"] + 7) // 8, (p["local_rows"] + 7) // 8
    p["tiles"] = p["tiles_x"] * p["tiles_y"]
    return p


def _key(p, gen, forget):
    c = p["cam"]
    f = {"eye": tuple(c.eye), "look_at": tuple(c.look_at), "up": tuple(c.up), "pitch": c.pitch,
         "bottom": (c.bottom_x, c.bottom_y), "size": (p["W"], p["H"]), "depth": p["depth"],
         "rows": p["rows"] or (0, 0, 0, 0), "scene": gen, "outputs": p["outs"], "format": p["format"],
         "samples": p["samples"]}
    key = tuple((k, f[k]) for k in KEY_FIELDS if k not in forget)
    # the tile grid follows from the size and the row plan: a model that forgets either has no grid to tell views apart by
    return key if forget & {"size", "rows"} else key + (("tiles", (p["tiles_x"], p["tiles_y"])),)


def _shape(key):
    return tuple(kv for kv in key if kv[0] not in CAMERA_FIELDS)


class Model:
    """The documented rule of the view cache, restated: for each step the branch render_plan_view takes (first,
    calibration, cached, other camera, captured), whether the eye's records are prepared, whether the calibration
    records cone masks and level masks, and the calibrated view the diagnostics describe after the step (view()).
    `forget`: key fields this model leaves out of the key — the true model forgets
    none; one that forgets a field calls a render cached where the library must not."""

    def __init__(self, forget=(), moving_order=False, recalibrate=8, cone_cache=True, level_masks=True):
        self.forget = frozenset(forget)
        self.moving_order, self.recalibrate = moving_order, recalibrate
        self.cone_cache, self.level_masks = cone_cache, level_masks
        self.scene, self.gen = None, 0
        self.order_key = self.seen_key = None        # None: not valid
        self.order_plan = None                       # the calibrated view (a forgetful model's stale view)
        self.cone_valid = False
        self.classes = self.flat = False             # ... has tile classes (rt_class_kernel) / flat verdicts (rt_flat_kernel)
        self.stale = 0
        self.eye = None                              # None: not valid
        self.ever_captured = False

    def view(self):
        """The calibrated view as rt_diag_sky_count, rt_diag_tile_classes and rt_diag_flat_tiles describe it: the last
        completed calibration, until the next calibration starts or a tile_order step -> dict(plan, cone, classes,
        flat), or None."""
        if self.order_key is None:
            return None
        return {"plan": self.order_plan, "cone": self.cone_valid, "classes": self.classes, "flat": self.flat}

    def step(self, step):
        """-> dict(branch, prepare, calibrate, cone, lmask, plan, view); branch None for a step without a
        render_dev_impl call; view: view() after the step."""
        out = self._step(step)
        out["view"] = self.view()
        return out

    def _step(self, step):
        out = {"branch": None, "prepare": False, "calibrate": False, "cone": False, "lmask": False, "plan": None}
        op = step["op"]
        if op == "set_scene":
            if step["scene"] != self.scene:          # (an equal record keeps the device copy, the eye and the view)
                self.scene, self.gen, self.eye = step["scene"], self.gen + 1, None
            return out
        if op == "tile_order":
            self.order_key = self.seen_key = None
            return out
        p = plan(step)
        if p is None:
            return out
        out["plan"] = p
        assert p["scene"] == self.scene, "a render step names the scene in force"
        if p["capturing"]:                           # self-contained: identity order, its own prepare launch, no key
            self.ever_captured = True
            out.update(branch="captured", prepare=True)
            return out
        n_padded, n_lights, opaque, _ = scene_facts(p["scene"])
        key = _key(p, self.gen, self.forget)
        same_shape = self.order_key is not None and _shape(key) == _shape(self.order_key)
        if self.order_key is not None and key == self.order_key:
            out["branch"] = "cached"
        elif same_shape and self.moving_order:       # the last calibrated order, re-timed every recalibrate-th render
            out["branch"] = "other"
            self.stale += 1
            if self.recalibrate > 0 and self.stale >= self.recalibrate:
                out["calibrate"] = True
                self._calibrated(key, p, False)
        elif self.seen_key is not None and key == self.seen_key:
            lm_stride = p["depth"] + (p["depth"] + 1) * n_lights if opaque and self.level_masks and self.cone_cache else 0
            if lm_stride > 24:
                lm_stride = 0
            cone = self.cone_cache and n_padded >= 8 and opaque
            out.update(branch="calibration", calibrate=True, cone=cone, lmask=cone and lm_stride > 0)
            # render_build_dispatch: the classes of a fast-kernel view (< 16 padded spheres: no culling kernel) with
            # level masks; the flat verdicts where the kernel instance reads the bit (rt_render.hpp class_instance:
            # not supersampled, and not packed from depth 2)
            classes = out["lmask"] and n_padded < 16
            packed = bool(p["outs"][1]) and p["format"][1] != "rgba8"
            self._calibrated(key, p, cone, classes, classes and p["samples"] == 0 and not (packed and p["depth"] >= 2))
        else:                                        # identity order; by default a moving camera's views come here too
            out["branch"] = "other" if same_shape else "first"
            self.seen_key = key
        eye = tuple(p["cam"].eye)
        out["prepare"] = self.ever_captured or self.eye != eye
        self.eye = eye
        return out

    def _calibrated(self, key, p, cone, classes=False, flat=False):
        self.order_key, self.order_plan, self.cone_valid, self.stale = key, p, cone, 0
        self.classes, self.flat = classes, flat


def sky_verdict(p):
    """rt_diag_sky_tiles of a plan's view -> uint8 [tile rows, tiles_x]."""
    return sk.host_verdict(scene_pair(p["scene"])[1], p["cam"], p["W"], p["H"], rows_of(p["rows"]))


# ---- the oracle's outputs of a step --------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _plain(scene, cam_key, W, H, depth, rows):
    rgb, rc = po.render(scene_pair(scene)[1], camera_named(*cam_key), W, H, depth, rows_of(rows))
    return _frozen({"rgb": rgb, "rc": rc})


@functools.lru_cache(maxsize=None)
def _supersampled(scene, cam_key, W, H, depth, rows):
    cam_s = sc.camera_ss(camera_named(*cam_key), SS)
    rows_s = (rows[0] * SS,) + rows[1:] if rows and rows[1] > 1 else rows
    hi, hi_rc = po.render(scene_pair(scene)[1], cam_s, SS * W, SS * H, depth, rows_of(rows_s))
    return _frozen({"rgb": sc.reduce_tree(hi, SS), "rc2": sc.reduce_counts(hi_rc, SS), "hi_rc": hi_rc})


def _images(rgb, counters, outs=(1, 1, 1, 1)):
    full = {"rgba32f": sc.to_rgba32f(rgb), "rgba8": sc.to_rgba8(rgb), "rgb64f": rgb, "raycount": counters}
    return {k: full[k] for k, on in zip(OUTS, outs) if on}


@functools.lru_cache(maxsize=None)
def _expected(op, scene, cam_key, W, H, depth, rows, outs, fmt):
    s, _ = scene_pair(scene)
    cam = camera_named(*cam_key)
    if op in ("render", "capture", "replay", "render_host", "render_packed"):
        e = _plain(scene, cam_key, W, H, depth, rows)
        if op == "render_packed":
            b = sc.to_rgba8(e["rgb"])
            ch = 4 if fmt == "rgba8" else 1 if scene_facts(scene)[3] else 3
            out = {"packed8": np.ascontiguousarray(b[..., :ch])}
        elif op == "render_host":
            out = {"rgb64f": e["rgb"]}
        else:
            out = _images(e["rgb"], e["rc"], OUTSETS[outs])
        out["grid_rc"] = e["rc"]
    elif op == "render_ss":
        e = _supersampled(scene, cam_key, W, H, depth, rows)
        out = _images(e["rgb"], e["rc2"], OUTSETS[outs])
        out["grid_rc"] = e["hi_rc"]
    elif op == "render_adaptive":
        base, ss = _plain(scene, cam_key, W, H, depth, None), _supersampled(scene, cam_key, W, H, depth, None)
        rgb, rc2, mask = ac.combine(base["rgb"], base["rc"], ss["rgb"], ss["rc2"], ADAPTIVE_T)
        out = _images(rgb, rc2, OUTSETS[outs])
        out["refined"] = mask.astype(np.uint8)
        out["grid_rc"] = base["rc"]
    else:
        d = mc.displacement(s, _MOVES[scene])
        L = LENS
        if op == "motion":
            e = mc.render(s, cam, W, H, depth, L["S"], L["A"], L["R"], L["F"], d)
        elif op == "jitter":
            e = jc.render(s, cam, W, H, depth, L["S"], L["J"], L["seed"], L["A"], 0.0, L["F"], d)
        elif op == "lens_adaptive":
            e = la.render(s, cam, W, H, depth, L["lo"], L["hi"], L["T"], L["A"], L["R"], L["F"], d)
        else:
            raise KeyError(op)
        out = _images(e["rgb"], e["rc2"])
        if op == "lens_adaptive":
            out["refined"] = e["mask"].astype(np.uint8)
    return _frozen(out)


def expected(step):
    """The oracle's outputs of a rendering step, memoised and read-only: the images the step asks for by name ("packed8":
    the packed byte image; "refined": the adaptive renders' mask), and for the calls with a view "grid_rc", the packed ray
    counters of the grid the view is keyed by (the sample grid's for a supersampled render)."""
    rows = tuple(step["rows"]) if step["rows"] else None
    return _expected(step["op"], step["scene"], (step["cam"],) + tuple(step["cam_size"]), step["size"][0], step["size"][1], step["depth"], rows,
                     step["outs"], step["fmt"] if step["op"] == "render_packed" else "")


def motion_of(scene):
    """The displacement the sampled calls' steps set before they render (rt_set_motion)."""
    return mc.displacement(scene_pair(scene)[0], _MOVES[scene])


# ---- the comparison --------------------------------------------------------------------------------------------------
def _pixels(a):
    """-> [rows, W, bytes per pixel] uint8 view of an image [rows, W] or [rows, W, C]."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], a.shape[1], -1)


def _first(bad):
    r, c = np.argwhere(bad)[0][:2]
    return f"first at row {int(r)}, column {int(c)}, {int(bad.sum())} in all"


def check_step(got, want, twin, what=""):
    """got, twin: {output name: array} of the context under test and of its twin (None: no twin); want: expected()'s
    dict.  The FP64 image and the counters bit for bit (NaNs by position), the float and byte images from the formulas,
    every output byte for byte against the twin, and no pixel left at the sentinel.  `what` names the step (its index and
    model branch); a failure adds the output and the first differing pixel."""
    for name, g in got.items():
        w = want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        gbytes = g.tobytes()
        if gbytes == w.tobytes() and (twin is None or gbytes == twin[name].tobytes()):
            continue                                 # (the same bytes: nothing below can object)
        gb, wb = _pixels(g), _pixels(w)
        left = (gb == SENTINEL).all(axis=2) & ~(wb == SENTINEL).all(axis=2)
        assert not left.any(), f"{what}: {name}: pixels no wave wrote (still the sentinel), {_first(left)}"
        if g.dtype.kind == "f":
            gn, wn = np.isnan(g), np.isnan(w)
            ib = np.uint64 if g.dtype == np.float64 else np.uint32
            bad = (gn != wn) | (~wn & (np.ascontiguousarray(g).view(ib) != np.ascontiguousarray(w).view(ib)))
        else:
            bad = g != w
        bad = bad.reshape(g.shape[0], g.shape[1], -1).any(axis=2)
        assert not bad.any(), f"{what}: {name} differs from the oracle, {_first(bad)}"
        if twin is not None:
            bad = (gb != _pixels(twin[name])).any(axis=2)
            assert not bad.any(), f"{what}: {name} differs from the twin's bytes, {_first(bad)}"


# ---- the censuses the floors of test_view_sequence.py are stated on ----------------------------------------------------
def trace(steps, **knobs):
    """The true model's verdict of every step."""
    m = Model(**knobs)
    return [m.step(s) for s in steps]


def branch_counts(steps, **knobs):
    out = dict.fromkeys(BRANCHES, 0)
    for r in trace(steps, **knobs):
        if r["branch"]:
            out[r["branch"]] += 1
    return out


def forgotten(steps, field, **knobs):
    """The steps a model that forgets `field` calls cached and the true model does not -> [(index, the stale view's
    plan, the new view's plan)]."""
    true, lax = Model(**knobs), Model(forget=(field,), **knobs)
    out = []
    for k, s in enumerate(steps):
        stale = lax.order_plan
        a, b = true.step(s), lax.step(s)
        if b["branch"] == "cached" and a["branch"] != "cached":
            out.append((k, stale, a["plan"]))
    return out


def discriminating(step, stale, new):
    """A stale verdict would show: the stale view's sky grid has the new view's shape and marks a tile in which the
    oracle's counters of the new view are not all the miss counter."""
    v = sky_verdict(stale)
    miss = sk.tiles_all_miss(expected(step)["grid_rc"])
    return v.shape == miss.shape and bool((v.astype(bool) & ~miss).any())
