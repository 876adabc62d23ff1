"""GPU tests of the view cache (rt_ctx::View, rt_plain.hip render_plan_view) along seeded call sequences and along one
named path per transition the hand-written cache tests do not take: a camera change that keeps the eye, a depth change,
a frame that grows the per-tile buffers and shrinks again, another width on the same tile grid, another row plan, the
entry points that share one view key, the sampled calls between two cached renders, scene swaps across the kernel
families, and a graph captured midway and replayed late.

One long-lived context per test executes the steps; beside it a twin created under RT_CONE_CACHE=0 RT_LEVEL_MASKS=0
RT_SKY_TILES=0 RT_TILE_CLASSES=0 and put in rt_diag_tile_order(.., 1) executes the same steps.  Every output buffer is
filled with 0xA5 on the step's stream first.  Every step is compared with the CPU oracle (view_sequence_common.expected)
bit for bit and with the twin byte for byte, and the host-side model of the cache is cross-checked against the library
after every step the device is drained behind: of the model's calibrated view (the last completed calibration, until
the next one starts or a tile_order step) rt_diag_sky_count reports the tiles and as many sky tiles as rt_diag_sky_tiles
proves when the calibration recorded cone masks, else none; rt_diag_tile_classes and rt_diag_flat_tiles report that tile
count exactly when the model says the calibration made classes and flat verdicts, else 0.  After a render the model
calls cached rt_diag_disp_count reports that view's tiles and no more positions than tiles; after any other step, what
it reported before the step.  A failure names the seed, the step and the model's branch.

A replay is not ordered against the context's other streams by the library (it rewrites the per-eye records on its own
stream), so the burst test drains the device around captures and replays, as a caller must."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402

from . import flat_tiles_common as ft  # noqa: E402
from . import tile_classes_common as tc  # noqa: E402
from . import view_sequence_common as vs  # noqa: E402

pytestmark = pytest.mark.gpu

TWIN_KNOBS = dict(RT_CONE_CACHE=0, RT_LEVEL_MASKS=0, RT_SKY_TILES=0, RT_TILE_CLASSES=0)
IMAGES = vs.OUTS + ("refined", "packed8")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Ctx:
    """A context, the graphs it captured and whether it is the twin."""

    def __init__(self, twin, **knobs):
        with _env(**knobs):
            self.t = Tracer(0)
        self.twin = twin
        self.graphs = {}
        if twin:
            abi.check(abi.lib().rt_diag_tile_order(self.t._ctx, 1), "rt_diag_tile_order")

    def close(self):
        self.graphs.clear()
        self.t.close()


@contextlib.contextmanager
def _pair(**knobs):
    """(the context under test, created under `knobs`; its twin; the streams of a step's `stream` field)."""
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    on, off = Ctx(False, **knobs), Ctx(True, **TWIN_KNOBS)
    streams = [torch.cuda.default_stream(), torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        yield on, off, streams
    finally:
        torch.cuda.synchronize()
        on.close()
        off.close()


def _fill(bufs):
    for k in IMAGES:
        if bufs.get(k) is not None:
            bufs[k].view(torch.uint8).fill_(vs.SENTINEL)
    return bufs


def _execute(c, step, streams):
    """One step on context c -> the buffers it renders into ({name: tensor or array}), or None when it renders nothing."""
    t, lib, op = c.t, abi.lib(), step["op"]
    if op == "set_scene":
        t.set_scene(vs.scene_pair(step["scene"])[1])
        return None
    if op == "tile_order":
        abi.check(lib.rt_diag_tile_order(t._ctx, 1), "rt_diag_tile_order")
        if not c.twin:
            abi.check(lib.rt_diag_tile_order(t._ctx, 0), "rt_diag_tile_order")
        return None
    if op == "replay":
        g, bufs, st = c.graphs[step["slot"]]
        with torch.cuda.stream(st):
            _fill(bufs)
            g.replay()
        return bufs
    W, H = step["size"]
    cam = vs.camera_named(step["cam"], *step["cam_size"])
    depth, rows = step["depth"], vs.rows_of(step["rows"])
    st = streams[step["stream"]]
    flags = dict(zip(vs.OUTS, (bool(v) for v in vs.OUTSETS[step["outs"]])))
    L = vs.LENS
    if op == "render_host":
        rgb = np.full((scenes.local_rows(H, rows), W, 3), np.nan)
        rgb.view(np.uint8)[...] = vs.SENTINEL
        stats = abi.rt_stats()
        abi.check(lib.rt_render(t._ctx, ctypes.byref(vs.scene_pair(step["scene"])[1]), ctypes.byref(cam), W, H, depth,
                                ctypes.byref(rows) if rows is not None else None, None, None,
                                ctypes.c_void_p(rgb.ctypes.data), ctypes.byref(stats)), "rt_render")
        assert stats.primary_rays == rgb.shape[0] * W
        return {"rgb64f": rgb}
    if op in vs.SAMPLED_OPS:
        t.set_motion(vs.motion_of(step["scene"]))
    with torch.cuda.stream(st):
        if op in ("render", "capture"):
            bufs = _fill(t.alloc(W, H, rows, **flags))
        elif op == "render_ss":
            bufs = _fill(t.alloc_ss(W, H, rows, **flags))
        elif op == "render_packed":
            ch = vs.expected(step)["packed8"].shape[2]
            bufs = _fill({"packed8": torch.empty((scenes.local_rows(H, rows), W, ch), dtype=torch.uint8, device="cuda")})
        elif op == "render_adaptive":
            bufs = _fill(t.alloc_adaptive(W, H, vs.SS, **flags))
        elif op == "lens_adaptive":
            bufs = _fill(t.alloc_lens_adaptive(W, H, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
        else:
            bufs = _fill(t.alloc_ss(W, H, None, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
    if op == "render":
        t.render_into(cam, W, H, depth, bufs, rows, st)
    elif op == "capture":
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            t.render_into(cam, W, H, depth, bufs, rows, st)
        c.graphs[step["slot"]] = (g, bufs, st)
        return None
    elif op == "render_ss":
        t.render_ss_into(cam, W, H, depth, vs.SS, bufs, rows, st)
    elif op == "render_packed":
        fmt = {1: abi.RT_PIXEL_GRAY8, 3: abi.RT_PIXEL_RGB8, 4: abi.RT_PIXEL_RGBA8}[bufs["packed8"].shape[2]]
        abi.check(lib.rt_render_dev_packed(t._ctx, ctypes.byref(cam), W, H, depth,
                                           ctypes.byref(rows) if rows is not None else None, abi.RT_PIXEL_RGBA32F, None,
                                           fmt, ctypes.c_void_p(bufs["packed8"].data_ptr()),
                                           ctypes.c_void_p(st.cuda_stream)), "rt_render_dev_packed")
    elif op == "render_adaptive":
        t.render_adaptive_into(cam, W, H, depth, vs.SS, vs.ADAPTIVE_T, bufs, st)
    elif op == "motion":
        t.render_motion_into(cam, W, H, depth, L["S"], L["A"], L["R"], L["F"], bufs, st)
    elif op == "jitter":
        t.render_jitter_into(cam, W, H, depth, L["S"], L["J"], L["seed"], L["A"], 0.0, L["F"], bufs, st)
    elif op == "lens_adaptive":
        t.render_lens_adaptive_into(cam, W, H, depth, L["lo"], L["hi"], L["T"], L["A"], L["R"], L["F"], bufs, st)
    else:
        raise KeyError(op)
    return bufs


def _host(bufs):
    out = {}
    for k in IMAGES:
        v = bufs.get(k)
        if v is not None:
            out[k] = v if isinstance(v, np.ndarray) else v.cpu().numpy()
    if "raycount" in out:
        out["raycount"] = out["raycount"].view(np.uint32)
    return out


def _disp_count(c):
    pos, tiles, run_max = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    abi.check(abi.lib().rt_diag_disp_count(c.t._ctx, ctypes.byref(pos), ctypes.byref(tiles), ctypes.byref(run_max)),
              "rt_diag_disp_count")
    return pos.value, tiles.value, run_max.value


def _sky_count(c):
    tiles, sky = ctypes.c_int(), ctypes.c_int()
    abi.check(abi.lib().rt_diag_sky_count(c.t._ctx, ctypes.byref(tiles), ctypes.byref(sky)), "rt_diag_sky_count")
    return tiles.value, sky.value


def _cross_check(c, verdict, what, before, drained=True):
    """The model's verdict of the step the context under test just executed, against the library's own account.
    before: rt_diag_disp_count ahead of the step."""
    p = verdict["plan"]
    if verdict["branch"] == "cached":
        pos, tiles, _ = _disp_count(c)
        assert tiles == p["tiles"] and 1 <= pos <= tiles, \
            f"{what}: the model calls this render cached, the library last rendered {pos} positions of {tiles} tiles " \
            f"from a cache (the view has {p['tiles']} tiles)"
    else:                                               # (the last cached render's account, whatever happened since)
        assert _disp_count(c) == before, \
            f"{what}: the model does not call this step a cached render, rt_diag_disp_count went from {before} to " \
            f"{_disp_count(c)}"
    if not drained:                                     # (the diagnostics below wait for the device)
        return
    # the calibrated view: the last completed calibration, until the next one starts or a tile_order step
    v = verdict["view"]
    cone = v is not None and v["cone"]
    n = v["plan"]["tiles"] if cone else 0
    want = (n, int(vs.sky_verdict(v["plan"]).sum())) if cone else (0, 0)
    assert _sky_count(c) == want, \
        f"{what}: of its calibrated view ({v and dict(v, plan=v['plan']['tiles'])}) the model expects (tiles, sky " \
        f"tiles) {want}, the library reports {_sky_count(c)}"
    got = tc.class_counts(c.t)[0], ft.flat_counts(c.t)[0]     # (the counts: the values are pinned by those modules' tests)
    want = (n if v["classes"] else 0, n if v["flat"] else 0) if cone else (0, 0)
    assert got == want, \
        f"{what}: of its calibrated view ({v and dict(v, plan=v['plan']['tiles'])}) the model expects (classified " \
        f"tiles, tiles with a flat verdict) {want}, the library reports {got}"


def _what(label, k, step, verdict):
    return f"{label} step {k} ({step['op']}, model branch {verdict['branch']}, prepare {verdict['prepare']})"


def _run(steps, label, burst=1, model_knobs=None, **knobs):
    """The steps on a context created under `knobs` and on its twin.  burst = 1: synchronised and checked after every
    step.  burst > 1: that many steps queued on rotating streams into separate buffers with no synchronisation between
    them (but around a capture or a replay), all checked after the last; the twin then executes them one by one."""
    model = vs.Model(**(model_knobs or {}))
    with _pair(**knobs) as (on, off, streams):
        for k0 in range(0, len(steps), burst):
            chunk = list(enumerate(steps[k0:k0 + burst], k0))
            if burst > 1:
                # the j-th step of a burst moves j streams on (a graph stays on its own), so that consecutive renders of
                # one view, a calibration among them, are in flight on different streams: the ordering rt_ctx::Sync owes
                chunk = [(k, s if s["op"] in ("capture", "replay", "set_scene", "tile_order")
                          else dict(s, stream=(s["stream"] + j) % 3)) for j, (k, s) in enumerate(chunk)]
            verdicts, got = {}, {}
            for k, step in chunk:
                verdicts[k] = model.step(step)
                if burst > 1 and step["op"] in ("capture", "replay"):
                    torch.cuda.synchronize()
                before = _disp_count(on)
                got[k] = _execute(on, step, streams)
                if burst > 1 and step["op"] in ("capture", "replay"):
                    torch.cuda.synchronize()
                last = k == chunk[-1][0]
                if last:
                    torch.cuda.synchronize()
                _cross_check(on, verdicts[k], _what(label, k, step, verdicts[k]), before, drained=last)
            for k, step in chunk:
                twin = _execute(off, step, streams)
                torch.cuda.synchronize()
                if got[k] is not None:
                    vs.check_step(_host(got[k]), vs.expected(step), _host(twin), _what(label, k, step, verdicts[k]))
        return model


# ---- the paths -------------------------------------------------------------------------------------------------------
def _view(**kv):
    v = {"op": "render", "scene": "c2", "size": [64, 40], "cam": "base", "depth": 1, "rows": None, "outs": "all",
         "fmt": "native", "stream": 0}
    v.update(kv)
    v.setdefault("cam_size", list(v["size"]))
    return v


def _there_and_back(a, *others, scene="c2"):
    """View A first, calibrated and cached twice; each other view three times; A again three times."""
    return [{"op": "set_scene", "scene": scene}] + [a] * 4 + [b for o in others for b in [o] * 3] + [a] * 3


def _branches(steps, **knobs):
    return [r["branch"] for r in vs.trace(steps, **knobs) if r["branch"]]


def _named_paths():
    """The steps of the named tests below, by test (and case)."""
    r, set_c2 = _view, {"op": "set_scene", "scene": "c2"}
    p = {("same_eye", cam): _there_and_back(r(), r(cam=cam)) for cam in vs.EYE_FIXED}
    p["moved_eye"] = _there_and_back(r(), r(cam="below"), r(cam="steep"))
    for scene, depths, size in DEPTH_CASES:
        p["depth", scene, tuple(size)] = _there_and_back(*(r(scene=scene, depth=d, size=size) for d in depths), scene=scene)
    p["grow"] = _there_and_back(r(), r(size=[160, 96]), r(size=[33, 17])) + \
        _there_and_back(r(scene="c5", depth=3), r(scene="c5", depth=3, size=[160, 96]), scene="c5")
    p["same_grid"] = _there_and_back(r(), r(size=[61, 37], cam_size=[64, 40]), r(size=[61, 37]))
    for size in ROW_SIZES:
        p["rows", tuple(size)] = _there_and_back(r(size=size), *(r(size=size, rows=list(k)) for k in vs.ROWS if k))
    p["entry_points"] = [set_c2] + [r()] * 3 + [r(op="render_adaptive")] * 3 + [r()] * 2 + \
        [r(op="render_adaptive", outs="bench"), r(outs="bench"), r(op="render_adaptive", outs="bench")] + \
        [r(op="render_ss")] * 3 + [r(op="render_packed", outs="bytes")] * 3 + \
        [r(op="render_packed", outs="bytes", fmt="rgba8"), r(outs="bytes"), r(op="render_packed", outs="bytes", fmt="rgba8")] + \
        [r(op="render_host", outs="parity"), r(outs="parity"), r(op="render_host", outs="parity")] + [r()] * 3
    sampled = [r(op=op) for op in vs.SAMPLED_OPS]
    p["sampled"] = [set_c2] + [r()] * 4 + sampled + [r()] + sampled[::-1] + [r()] * 2
    p["scenes"] = []
    for name in ("c2", "c5", "c1", "demo", "tree_demo", "rise", "c2"):
        p["scenes"] += [{"op": "set_scene", "scene": name}] + [r(scene=name, depth=2)] * 3
    p["scenes"] += [set_c2] + [r(depth=2)] * 2
    cap = r(op="capture", slot=0, stream=1)
    replay = dict(cap, op="replay")
    p["capture"] = [set_c2] + [r()] * 4 + [cap] + [r(cam="look_a")] * 3 + [r(cam="steep", stream=2)] * 3 + [replay] + \
        [r()] * 3 + [replay] + [r(cam="below")] * 2 + [replay]
    p["tile_order"] = [set_c2] + [r()] * 3 + [{"op": "tile_order"}] + [r()] * 3
    return p


DEPTH_CASES = [("c2", (0, 1, 2), [64, 40]), ("c2", (0, 2, 1), [160, 96]), ("c5", (3, 1, 5), [64, 40])]
ROW_SIZES = ([128, 80], [64, 40])
PATHS = _named_paths()


@pytest.fixture(scope="module", autouse=True)
def oracle_frames():
    """The oracle's frame of every step of every sequence and path, computed once ahead of the tests that share them
    (view_sequence_common.expected memoises them, read-only)."""
    for steps in [vs.generate(seed) for seeds in vs.SEEDS.values() for seed in seeds] + list(PATHS.values()):
        for s in steps:
            if "size" in s and s["op"] != "capture":
                vs.expected(s)


# ---- the seeded sequences ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", vs.SEEDS["sequence"])
def test_sequence(seed):
    _run(vs.generate(seed), f"seed {seed}")


@pytest.mark.parametrize("seed", vs.SEEDS["bursts"])
def test_sequence_bursts(seed):
    _run(vs.generate(seed), f"seed {seed} (bursts of 4)", burst=4)


@pytest.mark.parametrize("seed", vs.SEEDS["moving_order"])
def test_sequence_moving_order(seed):
    _run(vs.generate(seed), f"seed {seed} (RT_MOVING_ORDER=1 RT_RECALIBRATE=3)", model_knobs=vs.MOVING_KNOBS,
         RT_MOVING_ORDER=1, RT_RECALIBRATE=3)


def test_sequence_tile_order_policy():
    seed, = vs.SEEDS["tile_order_policy"]
    _run(vs.generate(seed), f"seed {seed} (RT_ORDER_POLICY=1)", RT_ORDER_POLICY=1)




# ---- one named path per transition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", vs.EYE_FIXED)
def test_same_eye_other_look_at_up_pitch_bottom(cam):
    """The one way a new view renders without rt_prepare_kernel: the eye stays, look_at, up, pitch or the bottom corner
    changes.  At 64 x 40 each of these views has hits in tiles the canonical view proves sky, or the other way round
    (test_view_sequence.py)."""
    steps = PATHS["same_eye", cam]
    verdicts = vs.trace(steps)
    assert [r["prepare"] for r in verdicts[1:]] == [True] + [False] * 9
    assert [r["branch"] for r in verdicts[1:]] == ["first", "calibration", "cached", "cached", "other", "calibration",
                                                   "cached", "other", "calibration", "cached"]
    _run(steps, f"same eye, {cam}")


def test_moved_eye_and_back():
    """The counterpart: the eye alone moves, to the two eyes whose views have hits where the canonical view proves sky,
    and every first render of an eye prepares it."""
    steps = PATHS["moved_eye"]
    assert [r["prepare"] for r in vs.trace(steps)[1:]] == [True, False, False, False] + [True, False, False] * 3
    _run(steps, "moved eye")


@pytest.mark.parametrize("scene,depths,size", DEPTH_CASES, ids=["c2-64x40", "c2-160x96", "c5-64x40"])
def test_depth_change_on_a_calibrated_view(scene, depths, size):
    """Another depth on a calibrated camera: other level-mask strides (the fast kernels' level-mask launch for c2, the
    culling kernels' own masks for c5) and, for c2, other tile classes — a tile that is sphere-free at depth 0 reflects a
    sphere at depth 1 — and a kernel instance that may not read the class bit."""
    _run(PATHS["depth", scene, tuple(size)], f"depth change, {scene}")


def test_grow_then_shrink():
    """160 x 96 (240 tiles) grows the per-tile buffers of a context calibrated at 64 x 40 (40 tiles); then 33 x 17 (15);
    then the same with c5, whose level masks grow too."""
    _run(PATHS["grow"], "grow then shrink")


def test_same_tile_grid_other_width():
    """64 x 40 and 61 x 37 are both 8 x 5 tiles: through the 64 x 40 camera (the size alone changes) and through its
    own."""
    _run(PATHS["same_grid"], "same tile grid")


@pytest.mark.parametrize("size", ROW_SIZES, ids=["128x80", "64x40"])
def test_row_plan_change(size):
    """Full frame, rank 0 and rank 1 of two ranks, a band height that is no multiple of 8, two frames in one call: at 128
    x 80 both ranks have 5 tile rows, at 64 x 40 rank 1 of (8, 2) and of (5, 3) both have 2."""
    _run(PATHS["rows", tuple(size)], f"row plans at {size}")


def test_entry_points_share_one_camera():
    """One camera through rt_render_dev, the adaptive render (whose base pass has rt_render_dev's key but for the sample
    count's tag when it writes counters, and rt_render_dev's own key when it does not), rt_render_ss_dev,
    rt_render_dev_packed (with RGBA8 the key of an rt_render_dev that writes the byte image alone) and the host-buffer
    rt_render (the key of an rt_render_dev that writes the FP64 image and the counters)."""
    steps = PATHS["entry_points"]
    b = _branches(steps)
    assert b[8:11] == b[17:20] == b[20:23] == ["first", "calibration", "cached"]     # the pairs that share a key
    _run(steps, "entry points")


def test_sampled_calls_leave_the_view_cached():
    """The lens family's calls, the jittered and the adaptive lens render between cached renders of a view: the view's
    dispatch count is unchanged and the next render of it is a cached one, and exact."""
    steps = PATHS["sampled"]
    assert _branches(steps) == ["first", "calibration"] + ["cached"] * 5
    with _pair() as (on, off, streams):
        before = None
        for k, step in enumerate(steps):
            got, twin = _execute(on, step, streams), _execute(off, step, streams)
            torch.cuda.synchronize()
            if got is not None:
                vs.check_step(_host(got), vs.expected(step), _host(twin), f"step {k} ({step['op']})")
            if k == 4:
                before = _disp_count(on)
                assert before[1] == 40 and 1 <= before[0] < 40           # (15 of the 40 tiles are sky: runs)
            if k > 4:
                assert _disp_count(on) == before, f"step {k} ({step['op']}) changed the view's dispatch count"


def test_scene_families_on_one_context():
    """c2 (fast kernels, tile classes), c5 (culling kernels), c1 (no masks), demo and tree_demo (never cone-calibrated),
    rise (c2 with one sphere moved against the sky), c2 again, and the same scene set once more, which keeps the view.
    One camera, size and depth throughout: the scene alone tells the views apart."""
    steps = PATHS["scenes"]
    assert _branches(steps) == ["first", "calibration", "cached"] * 7 + ["cached"] * 2
    _run(steps, "scene families")


def test_capture_midway_and_late_replay():
    """A render captured on a side stream after the context calibrated its view; other cameras, one with another eye,
    are calibrated; the graph is replayed; the first view is rendered again; the graph is replayed again.  Every render
    after the capture prepares its eye."""
    steps = PATHS["capture"]
    assert all(r["prepare"] for r in vs.trace(steps)[5:] if r["branch"])
    _run(steps, "capture midway")


def test_tile_order_forgets_the_calibrated_view():
    """rt_diag_tile_order(1), then (0), on a calibrated and cached view: the diagnostics describe no view until the view
    is calibrated afresh, which takes its first and its calibration render again."""
    steps = PATHS["tile_order"]
    verdicts = vs.trace(steps)
    assert [r["branch"] for r in verdicts] == [None, "first", "calibration", "cached", None, "first", "calibration", "cached"]
    assert [r["view"] is not None for r in verdicts] == [False, False, True, True, False, False, True, True]
    assert all(r["view"]["plan"]["tiles"] == 40 and r["view"]["cone"] and r["view"]["classes"] and r["view"]["flat"]
               for r in verdicts[2:4] + verdicts[6:])
    _run(steps, "tile order and back")
