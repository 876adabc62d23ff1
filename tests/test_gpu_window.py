"""GPU: windows of the accumulating and converging renders (rt_render_accum_window_dev, rt_render_converge_window_dev,
their host-buffer forms, Tracer.render_*_window*, the CLI's --window) against numpy slices of the expected FULL frames:
tests/accum_common.py and tests/converge_common.py on frames of the CPU oracle, and the fixtures made from the reference
build (tests/golden/accum.npz, converge.npz).  Expected values never come from the code under test.

Float images and the sums are compared bit for bit (NaNs by position), everything else exactly.  Every buffer a window
is rendered into is filled with a sentinel first, and every element outside the window must still hold it afterwards:
between the rows of a padded window, and everywhere else in a full frame whose window is rendered in place.  Frames are
19 x 11 at S = 2 unless said (a tile is 4 x 4 pixels); tests/test_window_oracle.py shows that the windows discriminate.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_tracer_fragment_shader_amd import abi, distributed, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402,F401

from . import accum_common as ac  # noqa: E402
from . import converge_common as cc  # noqa: E402
from . import lens_gpu_common as lg  # noqa: E402
from . import motion_common as mc  # noqa: E402
from . import shutter_common as hc  # noqa: E402
from . import soft_common as so  # noqa: E402
from . import ssaa_common as sc  # noqa: E402
from . import window_common as wc  # noqa: E402
from .lens_gpu_common import OUTS, _host, fresh, tr  # noqa: E402,F401
from .test_converge_oracle import INST_E, INST_K, MAIN  # noqa: E402
from .test_jitter_oracle import SHAPES  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, A, R, F, M = wc.W, wc.H, wc.A, wc.R, wc.F, wc.M
MOVES = mc.MOVES
LAYOUTS = ("dense", "padded", "inplace")
ACCUM_BUFS = ("accum",) + OUTS
CONVERGE_BUFS = ("accum", "accum2", "count") + OUTS
NAMES = ("rt_render_accum_window_dev", "rt_render_converge_window_dev", "rt_render_accum_window",
         "rt_render_converge_window")


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    for name in NAMES:
        assert name in abi.SIGNATURES and hasattr(abi.lib(), name), name


def _dev(t, a):
    return torch.from_numpy(np.array(a, copy=True)).to(torch.device("cuda", t.device))     # (a may be read-only)


class Frame:
    """Sentinel-filled device buffers `names` in one layout for the window `win` of a width x height frame."""

    def __init__(self, t, win, layout, names, width=W, height=H):
        (rows, cols), self.where = wc.layout_shape(layout, win, width, height)
        self.win, self.layout, self.t = win, layout, t
        self.full = {n: _dev(t, wc.sentinel(n, rows, cols)) for n in names}

    def view(self, n):
        """What the Tracer is given: the dense or full-frame tensor, or the window's columns of the padded rows."""
        if n not in self.full:
            return None
        return self.full[n][:, :self.win[2]] if self.layout == "padded" else self.full[n]

    def bufs(self):
        return {("raycount" if n == "raycount" else n): self.view(n) for n in OUTS}

    def state(self):
        return self.view("accum"), self.view("accum2"), self.view("count")

    def put(self, n, a):
        """Host values of the window's pixels into the window's place."""
        a = np.asarray(a)
        if n == "count":
            a = a.astype(np.int64).astype(np.uint32).view(np.int32)
        self.full[n][self.where] = _dev(self.t, a.astype(wc.BUFFERS[n][0]))

    def host(self):
        torch.cuda.synchronize()
        return {n: v.cpu().numpy() for n, v in self.full.items()}


def _want(e, win, converge):
    """The window's expected buffers from the full-frame expectation `e`."""
    m = wc.crop(e["mean"], win)
    out = {"accum": wc.crop(e["acc"], win), "rgb64f": m, "rgba32f": sc.to_rgba32f(m), "rgba8": sc.to_rgba8(m),
           "raycount": wc.crop(e["rc2"], win)}
    if converge:
        out["accum2"], out["count"] = wc.crop(e["sq"], win), wc.crop(e["n"], win)
    return out


def _active_of(e, win, Mp, E):
    return int(wc.crop(~cc.stopped(e["acc"], e["sq"], e["n"], Mp, E), win).sum())


def _same(name, got, want, what):
    if name in ("count", "raycount"):
        assert np.array_equal(got.view(np.uint32).astype(np.int64), np.asarray(want).astype(np.int64)), f"{what} {name}"
    elif name == "rgba8":
        assert np.array_equal(got, want), f"{what} {name}"
    else:
        sc.assert_same_bits(got, want, f"{what} {name}")


def _check(fr, want, what, names=None):
    """The window's pixels of every buffer against `want`, and every other element against the sentinel."""
    host = fr.host()
    for n in (names if names is not None else host):
        _same(n, host[n][fr.where], want[n], f"{what} {fr.win} {fr.layout}")
    for n, arr in host.items():
        assert wc.untouched_outside(n, arr, fr.where), f"{what} {fr.win} {fr.layout}: {n} written outside the window"
    return host


def _set(t, name, e):
    scene, depth = sc.scene_of(name)
    t.set_scene(scene)
    t.set_motion(e["d"])
    return depth


def _accum(t, e, depth, S, J, seed, n0, K, fr, width=W, height=H, bufs=None, arf=(A, R, F)):
    t.render_accum_window_into(e["cam"], hc.motion_abi(e["motion"]), width, height, fr.win, depth, S, J, seed, n0, K,
                               *arf, fr.view("accum"), fr.bufs() if bufs is None else bufs)


def _converge(t, e, depth, S, J, seed, K, Mp, E, fr, width=W, height=H, bufs=None, arf=(A, R, F), active=True):
    """-> the window's active count (None without `active`)."""
    act = torch.full((1,), 12345, dtype=torch.int32, device=torch.device("cuda", t.device)) if active else None
    t.render_converge_window_into(e["cam"], hc.motion_abi(e["motion"]), width, height, fr.win, depth, S, J, seed, K, Mp, E,
                                  *arf, fr.state(), fr.bufs() if bufs is None else bufs, act)
    torch.cuda.synchronize()
    return None if act is None else int(act.cpu().numpy().view(np.uint32)[0])


def _accum_e(name="c2", w=W, h=H, S=2, J=4, n0=0, K=wc.ACCUM_K):
    return ac.expected(name, "crane", w, h, S, J, 1, n0, K, A, R, F, MOVES[name])


def _converge_e(name="c2", w=W, h=H, case=MAIN):
    S, J, E, K = case
    return cc.expected(name, "crane", w, h, S, J, 1, K, M, E, A, R, F, MOVES[name])


# 1. every window of the list, three layouts ----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("win", wc.WINDOWS)
def test_accum_windows(tr, win, layout):
    e = _accum_e()
    depth = _set(tr, "c2", e)
    fr = Frame(tr, win, layout, ACCUM_BUFS)
    _accum(tr, e, depth, 2, 4, 1, 0, wc.ACCUM_K, fr)
    _check(fr, _want(e, win, False), "accum")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("win", wc.WINDOWS)
def test_converge_windows(tr, win, layout):
    S, J, E, K = MAIN
    e = _converge_e()
    depth = _set(tr, "c2", e)
    fr = Frame(tr, win, layout, CONVERGE_BUFS)
    fr.put("count", np.zeros((win[3], win[2]), np.int64))     # a new sum; the sums keep their sentinel and are not read
    active = _converge(tr, e, depth, S, J, 1, K, M, E, fr)
    _check(fr, _want(e, win, True), "converge")
    assert active == _active_of(e, win, M, E), (win, layout)


# 2. every instance on one unaligned window of every shape ---------------------------------------------------------------
@pytest.mark.parametrize("S,J,w,h", SHAPES)
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_variants(tr, name, S, J, w, h):
    """c2 depth 1 and c5 depth 3: the opaque instances; demo depth 5: the FULL one; tree_demo depth 5: the ray-tree one;
    both calls, in place in a full frame."""
    win = wc.SHAPE_WINDOWS[(S, J, w, h)]
    e = _accum_e(name, w, h, S, J)
    depth = _set(tr, name, e)
    fr = Frame(tr, win, "inplace", ACCUM_BUFS, w, h)
    _accum(tr, e, depth, S, J, 1, 0, wc.ACCUM_K, fr, w, h)
    _check(fr, _want(e, win, False), f"accum {name} S={S}")
    c = _converge_e(name, w, h, (S, J, INST_E, INST_K))
    fr = Frame(tr, win, "inplace", CONVERGE_BUFS, w, h)
    fr.put("count", np.zeros((win[3], win[2]), np.int64))
    active = _converge(tr, c, depth, S, J, 1, INST_K, M, INST_E, fr, w, h)
    _check(fr, _want(c, win, True), f"converge {name} S={S}")
    assert active == _active_of(c, win, M, INST_E)


# 3. the whole-frame window is the un-windowed call; one pass is the shutter render's rectangle ----------------------------
def test_whole_frame_window_is_the_unwindowed_call(tr):
    S, J, E, K = MAIN
    e = _converge_e()
    depth = _set(tr, "c2", e)
    m = hc.motion_abi(e["motion"])
    flags = dict(rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    whole = (0, 0, W, H)
    bufs, acc = tr.render_accum(e["cam"], m, W, H, depth, S, J, 1, 0, wc.ACCUM_K, A, R, F, **flags)
    wbufs, wacc = tr.render_accum_window(e["cam"], m, W, H, whole, depth, S, J, 1, 0, wc.ACCUM_K, A, R, F, **flags)
    a, b = _host(bufs), _host(wbufs)
    for k in OUTS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert acc.cpu().numpy().tobytes() == wacc.cpu().numpy().tobytes()
    bufs, st, act = tr.render_converge(e["cam"], m, W, H, depth, S, J, 1, K, M, E, A, R, F, **flags)
    wbufs, wst, wact = tr.render_converge_window(e["cam"], m, W, H, whole, depth, S, J, 1, K, M, E, A, R, F, **flags)
    a, b = _host(bufs), _host(wbufs)
    for k in OUTS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    for x, y in zip(st, wst):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert int(act.cpu()[0]) == int(wact.cpu()[0]) == e["active"]


def test_one_pass_from_pass_zero_is_the_shutter_renders_rectangle(tr):
    S, J, seed, win = 2, 4, 1, wc.UNALIGNED
    e = _converge_e()
    depth = _set(tr, "c2", e)
    m = hc.motion_abi(e["motion"])
    flags = dict(rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    sh = _host(tr.render_shutter(e["cam"], m, W, H, depth, S, J, seed, A, R, F, **flags))
    sc.assert_same_bits(sh["rgb64f"], hc.expected("c2", "crane", W, H, S, J, seed, A, R, F, MOVES["c2"])["rgb"], "shutter")
    bufs, acc = tr.render_accum_window(e["cam"], m, W, H, win, depth, S, J, seed, 0, 1, A, R, F, **flags)
    got = _host(bufs)
    for k in OUTS:
        assert got[k].tobytes() == np.ascontiguousarray(wc.crop(sh[k], win)).tobytes(), k
    assert acc.cpu().numpy().tobytes() == np.ascontiguousarray(wc.crop(sh["rgb64f"], win)).tobytes()
    bufs, st, act = tr.render_converge_window(e["cam"], m, W, H, win, depth, S, J, seed, 1, 2, 0.5, A, R, F, **flags)
    got = _host(bufs)
    for k in OUTS:
        assert got[k].tobytes() == np.ascontiguousarray(wc.crop(sh[k], win)).tobytes(), k
    assert st[0].cpu().numpy().tobytes() == np.ascontiguousarray(wc.crop(sh["rgb64f"], win)).tobytes()
    assert (st[2].cpu().numpy() == 1).all() and int(act.cpu()[0]) == win[2] * win[3]


# 4. tiling ---------------------------------------------------------------------------------------------------------------
def _plans():
    """The two partitions of the frame, each in a shuffled order."""
    out = []
    for order, plan in (((2, 0, 3, 1), wc.TILING), ((1, 2, 0), distributed.window_plan(W, H, 3))):
        assert wc.is_partition(plan, W, H) and sorted(order) == list(range(len(plan)))
        out.append([plan[k] for k in order])
    return out


def _tile(fr, win):
    """The full-frame buffers of `fr` addressed as the window `win` in place."""
    t = Frame.__new__(Frame)
    t.win, t.layout, t.t, t.full = win, "inplace", fr.t, fr.full
    _, t.where = wc.layout_shape("inplace", win, W, H)
    return t


@pytest.mark.parametrize("plan", _plans(), ids=["rectangles", "strips"])
def test_tiled_accum(tr, plan):
    """(0, 2) then (2, 1) per window, window after window into one set of full-frame buffers: the bytes of (0, 3), and
    the two calls' counters sum to its counters."""
    e = _accum_e()
    depth = _set(tr, "c2", e)
    fr = Frame(tr, (0, 0, W, H), "inplace", ACCUM_BUFS)
    first_rc = _dev(tr, wc.sentinel("raycount", H, W))
    for win in plan:
        t = _tile(fr, win)
        _accum(tr, e, depth, 2, 4, 1, 0, 2, t, bufs={**t.bufs(), "raycount": first_rc})
        _accum(tr, e, depth, 2, 4, 1, 2, 1, t)
    want = _want(e, (0, 0, W, H), False)
    want["raycount"] = _accum_e(n0=2, K=1)["rc2"]
    host = _check(fr, want, "tiled accum")
    total = first_rc.cpu().numpy().view(np.uint32) + host["raycount"].view(np.uint32)
    assert np.array_equal(total, e["rc2"])


def _tiled_converge(t, e, depth, fr, plan, K):
    """-> (the windows' active counts summed, the calls' counters in a full frame)."""
    rc = _dev(t, wc.sentinel("raycount", H, W))
    total = 0
    for win in plan:
        tile = _tile(fr, win)
        total += _converge(t, e, depth, 2, 4, 1, K, M, MAIN[2], tile, bufs={**tile.bufs(), "raycount": rc})
    torch.cuda.synchronize()
    return total, rc.cpu().numpy().view(np.uint32)


def _new_full_state(t):
    fr = Frame(t, (0, 0, W, H), "inplace", CONVERGE_BUFS)
    fr.put("count", np.zeros((H, W), np.int64))
    return fr


def _unwindowed_converge(t, e, depth, fr, K):
    act = torch.zeros((1,), dtype=torch.int32, device=torch.device("cuda", t.device))
    rc = torch.empty((H, W, 2), dtype=torch.int32, device=act.device)
    t.render_converge_into(e["cam"], hc.motion_abi(e["motion"]), W, H, depth, 2, 4, 1, K, M, MAIN[2], A, R, F, fr.state(),
                           {**fr.bufs(), "raycount": rc}, act)
    torch.cuda.synchronize()
    return int(act.cpu()[0]), rc.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("plan", _plans(), ids=["rectangles", "strips"])
def test_tiled_converge(tr, plan):
    """6 then 10 passes per window equal one call of 16; the windows' active counts sum to the call's."""
    S, J, E, K = MAIN
    assert K == 16
    e = _converge_e()
    depth = _set(tr, "c2", e)
    fr = _new_full_state(tr)
    _, rc6 = _tiled_converge(tr, e, depth, fr, plan, 6)
    active, rc10 = _tiled_converge(tr, e, depth, fr, plan[::-1], 10)
    want = _want(e, (0, 0, W, H), True)
    _check(fr, want, "tiled converge", names=[n for n in CONVERGE_BUFS if n != "raycount"])
    assert active == e["active"] and np.array_equal(rc6 + rc10, e["rc2"])


@pytest.mark.parametrize("windowed_first", [False, True])
def test_windowed_and_unwindowed_calls_continue_each_other(tr, windowed_first):
    e = _converge_e()
    depth = _set(tr, "c2", e)
    plan = _plans()[0]
    fr = _new_full_state(tr)
    if windowed_first:
        _, rc6 = _tiled_converge(tr, e, depth, fr, plan, 6)
        active, rc10 = _unwindowed_converge(tr, e, depth, fr, 10)
    else:
        _, rc6 = _unwindowed_converge(tr, e, depth, fr, 6)
        active, rc10 = _tiled_converge(tr, e, depth, fr, plan, 10)
    _check(fr, _want(e, (0, 0, W, H), True), "interop", names=[n for n in CONVERGE_BUFS if n != "raycount"])
    assert active == e["active"] and np.array_equal(rc6 + rc10, e["rc2"])


# 5. resume; the launch split ---------------------------------------------------------------------------------------------
def test_resume_on_a_window_under_a_smaller_tolerance(tr):
    S, J, win = 2, 4, wc.UNALIGNED
    fo = cc.frames("c2", "crane", W, H, S, J, 1, A, R, F, MOVES["c2"])
    a = cc.converge(fo, cc.zero_state(H, W), 6, M, 1.0 / 8.0)
    b = cc.converge(fo, cc.state_of(a), 10, M, 1.0 / 32.0)
    assert (wc.crop(b["received"], win) > 0).any() and (wc.crop(a["n"], win) < 6).any()
    e = _converge_e()
    depth = _set(tr, "c2", e)
    fr = Frame(tr, win, "padded", CONVERGE_BUFS)
    fr.put("count", np.zeros((win[3], win[2]), np.int64))
    active = _converge(tr, e, depth, S, J, 1, 6, M, 1.0 / 8.0, fr)
    _check(fr, _want(a, win, True), "loose")
    assert active == _active_of(a, win, M, 1.0 / 8.0)
    active = _converge(tr, e, depth, S, J, 1, 10, M, 1.0 / 32.0, fr)
    _check(fr, _want(b, win, True), "resumed")
    assert active == _active_of(b, win, M, 1.0 / 32.0)


def test_launch_split_is_invisible_in_a_fresh_process(tmp_path):
    """A process of its own under RT_ACCUM_MAX_PASSES=2 (tests/window_common.py as a module): three accumulated passes as
    two launches and a budget of 16 as eight, on an unaligned window."""
    win = wc.UNALIGNED
    out = tmp_path / "child.npz"
    env = dict(os.environ, RT_ACCUM_MAX_PASSES="2")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.window_common", str(out)], cwd=root, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(np.load(out))
    for prefix, want in (("a_", _want(_accum_e(), win, False)), ("c_", _want(_converge_e(), win, True))):
        for n, v in want.items():
            _same(n, got[prefix + n], v, "RT_ACCUM_MAX_PASSES=2 " + prefix)
    assert int(got["c_active"].view(np.uint32)[0]) == _active_of(_converge_e(), win, M, MAIN[2])


# 6. the fixtures ---------------------------------------------------------------------------------------------------------
def _fixture_scene(t, base):
    name, S, J, Ff, Af, Rf, lights, moves, motion = ac.shutter_fixture(base)
    scene, depth = sc.scene_of(name)
    t.set_scene(scene if lights is None else so.scene_abi(scene, lights))
    t.set_motion(mc.displacement(scene, moves))
    e = {"cam": scenes.make_camera(ac.FIX_W, ac.FIX_H, 500.0 / ac.FIX_W), "motion": hc.MOTIONS[motion]}
    return e, depth, S, J, (Af, Rf, Ff)


def test_fixture_windows(tr):
    win = wc.FIXTURE_WINDOW
    key, base, seed, K = ac.FIXTURES[0]
    assert key == "c2_pan_k3"
    e, depth, S, J, arf = _fixture_scene(tr, base)
    fr = Frame(tr, win, "inplace", ("accum", "rgb64f"), ac.FIX_W, ac.FIX_H)
    _accum(tr, e, depth, S, J, seed, 0, K, fr, ac.FIX_W, ac.FIX_H, bufs={"rgb64f": fr.view("rgb64f")}, arf=arf)
    fx = ac.fixtures()
    _check(fr, {"accum": wc.crop(fx[key + "_acc"], win), "rgb64f": wc.crop(fx[key + "_mean"], win)}, key)
    key, base, seed, K, Mf, E = cc.FIXTURE
    e, depth, S, J, arf = _fixture_scene(tr, base)
    fr = Frame(tr, win, "inplace", ("accum", "accum2", "count", "rgb64f"), cc.FIX_W, cc.FIX_H)
    fr.put("count", np.zeros((win[3], win[2]), np.int64))
    _converge(tr, e, depth, S, J, seed, K, Mf, E, fr, cc.FIX_W, cc.FIX_H, bufs={"rgb64f": fr.view("rgb64f")}, arf=arf)
    fx = cc.fixtures()
    _check(fr, {"accum": wc.crop(fx[key + "_acc"], win), "accum2": wc.crop(fx[key + "_sq"], win),
                "count": wc.crop(fx[key + "_count"], win), "rgb64f": wc.crop(fx[key + "_mean"], win)}, key)


# 7. each output alone, none, no active -----------------------------------------------------------------------------------
@pytest.mark.parametrize("only", OUTS + (None,))
def test_nullable_outputs(tr, only):
    S, J, E, K = MAIN
    win = wc.UNALIGNED
    a, c = _accum_e(), _converge_e()
    depth = _set(tr, "c2", c)
    names = ("accum",) + ((only,) if only else ())
    fr = Frame(tr, win, "inplace", names)
    _accum(tr, a, depth, S, J, 1, 0, wc.ACCUM_K, fr, bufs={only: fr.view(only)} if only else {})
    _check(fr, _want(a, win, False), f"accum with {only}")
    fr = Frame(tr, win, "inplace", ("accum2", "count") + names)
    fr.put("count", np.zeros((win[3], win[2]), np.int64))
    _converge(tr, c, depth, S, J, 1, K, M, E, fr, bufs={only: fr.view(only)} if only else {}, active=False)
    _check(fr, _want(c, win, True), f"converge with {only}")


# 8. graph capture ---------------------------------------------------------------------------------------------------
def test_graph_capture_of_a_windowed_converge_call(fresh):
    """A capture of ten passes on a window, in place, continuing a state of six; three replays, each from the restored
    state, sentinel images and a spoilt active word (its reset is a memset node of the call)."""
    S, J, win = 2, 4, wc.UNALIGNED
    fo = cc.frames("c2", "crane", W, H, S, J, 1, A, R, F, MOVES["c2"])
    a = cc.converge(fo, cc.zero_state(H, W), 6, M, 1.0 / 8.0)
    e = cc.converge(fo, cc.state_of(a), 10, M, 1.0 / 32.0)
    x = _converge_e()
    depth = _set(fresh, "c2", x)
    m = hc.motion_abi(x["motion"])
    fr = Frame(fresh, win, "inplace", CONVERGE_BUFS)
    active = torch.zeros((1,), dtype=torch.int32, device=fr.full["count"].device)
    pristine = {n: v.clone() for n, v in fr.full.items()}
    render_into = lambda s: fresh.render_converge_window_into(x["cam"], m, W, H, win, depth, S, J, 1, 10, M, 1.0 / 32.0,  # noqa: E731
                                                              A, R, F, fr.state(), fr.bufs(), active, stream=s)

    def restore():
        for n, v in fr.full.items():
            v.copy_(pristine[n])
        for n, key in (("accum", "acc"), ("accum2", "sq"), ("count", "n")):
            fr.put(n, wc.crop(a[key], win))
        active.fill_(12345)
        torch.cuda.synchronize()

    def check(what):
        _check(fr, _want(e, win, True), what)
        assert int(active.cpu().numpy()[0]) == _active_of(e, win, M, 1.0 / 32.0), what

    s = torch.cuda.Stream()
    restore()
    with torch.cuda.stream(s):
        render_into(s)                                                           # warm-up outside the capture
    s.synchronize()
    check("direct")
    g = torch.cuda.CUDAGraph()
    restore()
    with torch.cuda.graph(g, stream=s):
        render_into(s)
    for k in range(3):
        restore()
        g.replay()
        check(f"replay {k} of 3")


# 9. host buffers with a stride; the CLI ----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["padded", "inplace"])
def test_host_buffers_with_a_stride(tr, layout):
    S, J, seed, win = 2, 4, 1, wc.UNALIGNED
    x0, y0, w, h = win
    (rows, cols), where = wc.layout_shape(layout, win, W, H)
    a2, a3 = _accum_e(K=2), _accum_e(n0=2, K=1)
    fo = cc.frames("c2", "crane", W, H, S, J, seed, A, R, F, MOVES["c2"])
    c6 = cc.converge(fo, cc.zero_state(H, W), 6, M, 1.0 / 8.0)
    c16 = cc.converge(fo, cc.state_of(c6), 10, M, 1.0 / 32.0)
    scene, depth = sc.scene_of("c2")
    s_abi = scene.to_abi()
    d = np.ascontiguousarray(a2["d"])
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    m = hc.motion_abi(a2["motion"])
    wabi = abi.rt_window(x0, y0, w, h, cols)
    L = abi.lib()

    def ptr(arr):                                            # window pixel (0, 0) of a host array
        return ctypes.c_void_p(arr[where].ctypes.data)

    def check(host, want, what):
        for n, arr in host.items():
            _same(n, arr[where], want[n], what)
            assert wc.untouched_outside(n, arr, where), f"{what}: {n} written outside the window"

    host = {n: wc.sentinel(n, rows, cols) for n in ("accum", "rgba32f", "rgba8", "rgb64f")}
    for n0, K, e in ((0, 2, a2), (2, 1, a3)):
        st = abi.rt_stats()
        abi.check(L.rt_render_accum_window(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(a2["cam"]), ctypes.byref(m), W, H,
                                           ctypes.byref(wabi), depth, S, J, seed, n0, K, A, R, F, ptr(host["accum"]),
                                           ptr(host["rgba32f"]), ptr(host["rgba8"]), ptr(host["rgb64f"]), ctypes.byref(st)),
                  "rt_render_accum_window")
        check(host, _want(e, win, False), f"host accum ({n0}, {K})")
        rc = wc.crop(e["rc2"], win)
        prim = w * h * S * S * K
        assert st.primary_rays == prim and st.reflect_rays == int(rc[..., 0].sum(dtype=np.uint64)) - prim
        assert st.shadow_rays == int(rc[..., 1].sum(dtype=np.uint64))
    host = {n: wc.sentinel(n, rows, cols) for n in ("accum", "accum2", "count", "rgba32f", "rgba8", "rgb64f")}
    host["count"][where] = 0
    for K, E, e in ((6, 1.0 / 8.0, c6), (10, 1.0 / 32.0, c16)):
        st, n_active = abi.rt_stats(), ctypes.c_uint64(99)
        abi.check(L.rt_render_converge_window(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(a2["cam"]), ctypes.byref(m), W,
                                              H, ctypes.byref(wabi), depth, S, J, seed, K, M, E, A, R, F,
                                              ptr(host["accum"]), ptr(host["accum2"]), ptr(host["count"]),
                                              ptr(host["rgba32f"]), ptr(host["rgba8"]), ptr(host["rgb64f"]),
                                              ctypes.byref(st), ctypes.byref(n_active)), "rt_render_converge_window")
        check(host, _want(e, win, True), f"host converge K={K}")
        assert n_active.value == _active_of(e, win, M, E)
        rc = wc.crop(e["rc2"], win)
        prim = int(wc.crop(e["received"], win).sum()) * S * S
        assert st.primary_rays == prim and st.reflect_rays == int(rc[..., 0].sum(dtype=np.uint64)) - prim
        assert st.shadow_rays == int(rc[..., 1].sum(dtype=np.uint64))


def _read_ppm(path, w, h):
    hdr, body = open(path, "rb").read().split(b"\n", 1)
    assert hdr.split() == [b"P6", str(w).encode(), str(h).encode(), b"255"]
    return np.frombuffer(body, np.uint8).reshape(h, w, 3)


def test_cli_writes_the_windows_image(tmp_path):
    motion = ((12.0, 30.0, -16.0), (50.0, 20.0, 0.0))
    win = wc.FIXTURE_WINDOW
    assert win[0] + win[2] <= lg.W and win[1] + win[3] <= lg.H
    c = cc.expected("c2", motion, lg.W, lg.H, 2, 4, 7, 8, 4, 0.03125, 8.0, 0.0, 0.5, MOVES["c2"])
    a = ac.expected("c2", motion, lg.W, lg.H, 2, 4, 7, 0, 3, 8.0, 0.0, 0.5, MOVES["c2"])
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c2_window.ppm"
    base = [exe, "--config", "c2", "--width", str(lg.W), "--height", str(lg.H), "--samples", "2", "--shutter", "0.5",
            "--move", "4:50,0,0", "--move", "0:0,12,-30", "--aperture", "8", "--eye-move", "12,30,-16", "--look-move",
            "50,20,0", "--jitter", "4", "--seed", "7", "--out", str(out), "--window", ",".join(str(v) for v in win)]
    r = subprocess.run(base + ["--passes", "8", "--tolerance", "0.03125"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    npx = win[2] * win[3]
    active, traced = _active_of(c, win, 4, 0.03125), int(wc.crop(c["n"], win).sum())
    assert f"{active} of {npx} pixels still active" in r.stdout, r.stdout
    assert f"{traced} of {8 * npx} pixel-passes traced" in r.stdout and f"{4 * traced} primary rays" in r.stdout, r.stdout
    want = sc.to_rgba8(wc.crop(c["mean"], win))[::-1, :, :3]                    # PPM rows run top to bottom
    assert np.array_equal(_read_ppm(out, win[2], win[3]), want)
    r = subprocess.run(base + ["--passes", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "accumulated, 3 passes" in r.stdout and f"{npx * 4 * 3} primary rays" in r.stdout, r.stdout
    assert np.array_equal(_read_ppm(out, win[2], win[3]), sc.to_rgba8(wc.crop(a["mean"], win))[::-1, :, :3])


# 10. argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(tr):
    from .test_window_oracle import BAD_WINDOWS
    S, J, E, K = MAIN
    e = _converge_e()
    depth = _set(tr, "c2", e)
    cam, m = e["cam"], hc.motion_abi(e["motion"])
    fr = Frame(tr, (0, 0, W, H), "inplace", CONVERGE_BUFS)
    active = torch.full((1,), -7, dtype=torch.int32, device=fr.full["count"].device)
    L = abi.lib()
    p = lambda n: None if n is None else ctypes.c_void_p(fr.full[n].data_ptr())  # noqa: E731
    good = (3, 2, 7, 5, W)

    def accum(win=good, w=W, h=H, S=2, J=4, n0=0, K=3, acc="accum"):
        wp = None if win is None else ctypes.byref(abi.rt_window(*win))
        return L.rt_render_accum_window_dev(tr._ctx, ctypes.byref(cam), ctypes.byref(m), w, h, wp, depth, S, J, 1, n0, K,
                                            A, R, F, p(acc), p("rgba32f"), p("rgba8"), p("rgb64f"), p("raycount"),
                                            lg.stream_ptr())

    def converge(win=good, w=W, h=H, S=2, J=4, K=K, Mp=M, E=E, acc="accum", acc2="accum2", count="count"):
        wp = None if win is None else ctypes.byref(abi.rt_window(*win))
        return L.rt_render_converge_window_dev(tr._ctx, ctypes.byref(cam), ctypes.byref(m), w, h, wp, depth, S, J, 1, K,
                                               Mp, E, A, R, F, p(acc), p(acc2), p(count), p("rgba32f"), p("rgba8"),
                                               p("rgb64f"), p("raycount"), ctypes.c_void_p(active.data_ptr()),
                                               lg.stream_ptr())

    for call in (accum, converge):
        for bad in [None] + BAD_WINDOWS:
            assert call(win=bad) == abi.RT_EINVAL and "window" in abi.last_error(), (call.__name__, bad)
        # the un-windowed call's own checks, one of each family
        assert call(acc=None) == abi.RT_EINVAL and "accum" in abi.last_error()
        assert call(K=0) == abi.RT_EINVAL and "passes" in abi.last_error()
        assert call(K=65537) == abi.RT_EINVAL and "passes" in abi.last_error()
        assert call(J=3) == abi.RT_EINVAL and "jitter" in abi.last_error()
        assert call(S=3) == abi.RT_EINVAL and "samples" in abi.last_error()
        assert call(win=(0, 0, 1, 1, 1), w=0) == abi.RT_EINVAL
        assert call(win=(3, 2, 7, 5, 7), w=9, h=11) == abi.RT_EINVAL and "window" in abi.last_error()   # leaves a smaller frame
    assert accum(n0=2 ** 31 - 1, K=2) == abi.RT_EINVAL and "first_pass" in abi.last_error()
    assert converge(acc2=None) == abi.RT_EINVAL and "accum2" in abi.last_error()
    assert converge(count=None) == abi.RT_EINVAL and "count" in abi.last_error()
    assert converge(Mp=1) == abi.RT_EINVAL and "min_passes" in abi.last_error()
    assert converge(E=-1.0) == abi.RT_EINVAL and "tolerance" in abi.last_error()
    dev = torch.device("cuda", tr.device)
    with pytest.raises(ValueError):                          # neither the frame's nor the window's shape
        tr.render_accum_window_into(cam, m, W, H, wc.UNALIGNED, depth, 2, 4, 1, 0, 3, A, R, F,
                                    torch.empty((5, 8, 3), dtype=torch.float64, device=dev), {})
    with pytest.raises(ValueError):                          # two buffers with different row strides
        tr.render_accum_window_into(cam, m, W, H, wc.UNALIGNED, depth, 2, 4, 1, 0, 3, A, R, F,
                                    torch.empty((5, 7, 3), dtype=torch.float64, device=dev),
                                    {"rgb64f": torch.empty((H, W, 3), dtype=torch.float64, device=dev)})
    with pytest.raises(ValueError):                          # the wrong type
        tr.render_accum_window_into(cam, m, W, H, wc.UNALIGNED, depth, 2, 4, 1, 0, 3, A, R, F,
                                    torch.empty((5, 7, 3), dtype=torch.float32, device=dev), {})
    with pytest.raises(ValueError):
        tr.render_accum_window_into(cam, m, W, H, (13, 2, 7, 5), depth, 2, 4, 1, 0, 3, A, R, F,
                                    torch.empty((5, 7, 3), dtype=torch.float64, device=dev), {})
    torch.cuda.synchronize()
    for n, arr in fr.host().items():
        assert (arr == wc.BUFFERS[n][2]).all(), f"a rejected call wrote {n}"
    assert int(active.cpu()[0]) == -7
    t = _tile(fr, good[:4])                                   # the same buffers, good arguments
    t.put("count", np.zeros((5, 7), np.int64))
    assert _converge(tr, e, depth, S, J, 1, K, M, E, t) == _active_of(e, good[:4], M, E)
    _check(t, _want(e, good[:4], True), "after the errors")


# 11. the context's other state --------------------------------------------------------------------------------------------
def test_no_side_effect(fresh):
    """A view's first, calibration and cached renders; then windowed calls of both kinds with other cameras and windows;
    then the view again and a plain render: the per-view state is what it was."""
    w, h = lg.W, lg.H
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    fresh.set_motion(mc.displacement(scene, MOVES["c2"]))
    cam = scenes.make_camera(w, h, 500.0 / w)
    frames = lg.view_frames(fresh, scene, cam, depth)
    flags = dict(rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    before = _host(fresh.render_soft(cam, w, h, depth, 2, A, R, **flags))
    e = _converge_e()
    for win in (wc.UNALIGNED, (12, 6, 7, 5)):
        fresh.render_accum_window(e["cam"], hc.motion_abi(e["motion"]), W, H, win, depth, 2, 4, 1, 0, 3, A, R, F, **flags)
        bufs, st, act = fresh.render_converge_window(e["cam"], hc.motion_abi(e["motion"]), W, H, win, depth, 2, 4, 1, 16, M,
                                                     MAIN[2], A, R, F, **flags)
    sc.assert_same_bits(_host(bufs)["rgb64f"], wc.crop(e["mean"], win), "the last window")
    assert int(act.cpu()[0]) == _active_of(e, win, M, MAIN[2])
    lg.check_view_unchanged(frames, _host(fresh.render(cam, w, h, depth, **flags)))
    after = _host(fresh.render_soft(cam, w, h, depth, 2, A, R, **flags))
    for key in OUTS:
        assert after[key].tobytes() == before[key].tobytes(), key
