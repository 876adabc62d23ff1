"""GPU: lists of windows of the accumulating and converging renders (rt_set_windows, rt_render_accum_windows_dev,
rt_render_converge_windows_dev, their host-buffer forms, Tracer.render_*_windows*, the CLI's --windows) against numpy
slices and concatenations of the expected FULL frames (tests/accum_common.py, tests/converge_common.py on frames of the
CPU oracle; tests/window_list_common.py pack() and scatter()).  Expected values never come from the code under test.

Every buffer of a call is filled with sentinels first and compared WHOLE: in place, the windows' pixels of the expected
frame and the sentinel everywhere else; packed, the windows' pixels one window after the other and the sentinel in the
spare elements behind them.  Floats bit for bit (NaNs by position), everything else exactly.  Frames are 19 x 11 at
S = 2, J = 4 unless said (a tile is 4 x 4 pixels).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402

from . import accum_common as ac  # noqa: E402
from . import converge_common as cc  # noqa: E402
from . import lens_gpu_common as lg  # noqa: E402
from . import motion_common as mc  # noqa: E402
from . import shutter_common as hc  # noqa: E402
from . import ssaa_common as sc  # noqa: E402
from . import window_common as wc  # noqa: E402
from . import window_list_common as wl  # noqa: E402
from .lens_gpu_common import OUTS, _host, fresh, tr  # noqa: E402,F401
from .test_converge_oracle import INST_E, INST_K, MAIN  # noqa: E402
from .test_jitter_oracle import SHAPES  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, A, R, F, M = wc.W, wc.H, wc.A, wc.R, wc.F, wc.M
MOVES = mc.MOVES
LAYOUTS = ("inplace", "packed")
ACCUM_BUFS = ("accum",) + OUTS
CONVERGE_BUFS = ("accum", "accum2", "count") + OUTS
SPARE = 5                                    # elements behind a packed buffer's last window
NAMES = ("rt_window_list_plan", "rt_set_windows", "rt_render_accum_windows_dev", "rt_render_converge_windows_dev",
         "rt_render_accum_windows", "rt_render_converge_windows")
LISTS = {k: v for k, v in wl.lists().items() if k != "ONE"}
WHOLE = (0, 0, W, H)


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    for name in NAMES:
        assert name in abi.SIGNATURES and hasattr(abi.lib(), name), name


def _dev(t, a):
    return torch.from_numpy(np.array(a, copy=True)).to(torch.device("cuda", t.device))     # (a may be read-only)


def _typed(name, a):
    """Host values of buffer `name` in the buffer's own type (the counters are uint32 held in int32 tensors)."""
    a = np.asarray(a)
    if name in ("count", "raycount"):
        return a.astype(np.int64).astype(np.uint32).view(np.int32)
    return a.astype(wc.BUFFERS[name][0])


def _layout_of(name, full, wins, layout):
    """The whole buffer `name` of a list call: the windows' pixels of the full-frame values `full` where the layout puts
    them, the sentinel everywhere else."""
    a, fill = _typed(name, full), wc.BUFFERS[name][2]
    if layout == "inplace":
        return wl.scatter(a, wins, fill)
    return np.concatenate([wl.pack(a, wins), np.full((SPARE,) + a.shape[2:], fill, a.dtype)])


def _blank(name, wins, layout, shape):
    """A sentinel-filled host buffer `name` of the list: the full frame in place; the windows' elements and SPARE packed."""
    dtype, c, fill = wc.BUFFERS[name]
    lead = tuple(shape) if layout == "inplace" else (sum(w * h for _, _, w, h in wins) + SPARE,)
    return np.full(lead + (() if name == "count" else (c,)), fill, dtype)


class Bufs:
    """Sentinel-filled device buffers `names` of the list `wins` of a width x height frame in one layout."""

    def __init__(self, t, wins, layout, names, width=W, height=H):
        self.t, self.wins, self.layout, self.shape = t, wins, layout, (height, width)
        self.full = {n: _dev(t, self.blank(n)) for n in names}

    def blank(self, n):
        return _blank(n, self.wins, self.layout, self.shape)

    def put(self, n, full):
        """Full-frame host values into the windows' places (the sentinel stays everywhere else)."""
        self.full[n].copy_(_dev(self.t, _layout_of(n, full, self.wins, self.layout)))

    def new_sum(self):
        self.put("count", np.zeros(self.shape, np.int64))    # the sums keep their sentinel and are not read
        return self

    def bufs(self):
        return {n: self.full.get(n) for n in OUTS}

    def state(self):
        return self.full["accum"], self.full["accum2"], self.full["count"]

    def host(self):
        torch.cuda.synchronize()
        return {n: v.cpu().numpy() for n, v in self.full.items()}

    def check(self, want, what, names=None):
        """Every buffer, whole, against the layout of the full-frame expectation `want`."""
        host = self.host()
        for n in (names if names is not None else host):
            _same(n, host[n], _layout_of(n, want[n], self.wins, self.layout), f"{what} {self.layout}")
        return host


def _same(name, got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what} {name}: {got.shape} {got.dtype}"
    if name in ("count", "raycount", "rgba8"):
        assert np.array_equal(got, want), f"{what} {name}"
    else:
        sc.assert_same_bits(got, want, f"{what} {name}")


def _want(e, converge):
    """The full-frame expectation of every buffer from accum_common / converge_common's `e`."""
    m = e["mean"]
    out = {"accum": e["acc"], "rgb64f": m, "rgba32f": sc.to_rgba32f(m), "rgba8": sc.to_rgba8(m), "raycount": e["rc2"]}
    if converge:
        out["accum2"], out["count"] = e["sq"], e["n"]
    return out


def _active_of(e, wins, Mp, E):
    return int((~cc.stopped(e["acc"], e["sq"], e["n"], Mp, E) & wl.mask(wins, *e["n"].shape[::-1])).sum())


def _set(t, name, e, wins, layout, width=W, height=H):
    scene, depth = sc.scene_of(name)
    t.set_scene(scene)
    t.set_motion(e["d"])
    want = sum(w * h for _, _, w, h in wins) if layout == "packed" else width * height
    assert t.set_windows(width, height, wins, layout) == want
    return depth


def _accum(t, e, depth, S, J, seed, n0, K, b, width=W, height=H, bufs=None):
    t.render_accum_windows_into(e["cam"], hc.motion_abi(e["motion"]), width, height, depth, S, J, seed, n0, K, A, R, F,
                                b.full["accum"], b.bufs() if bufs is None else bufs)


def _converge(t, e, depth, S, J, seed, K, Mp, E, b, width=W, height=H, bufs=None, active=True):
    """-> the list's active count (None without `active`)."""
    act = torch.full((1,), 12345, dtype=torch.int32, device=torch.device("cuda", t.device)) if active else None
    t.render_converge_windows_into(e["cam"], hc.motion_abi(e["motion"]), width, height, depth, S, J, seed, K, Mp, E,
                                   A, R, F, b.state(), b.bufs() if bufs is None else bufs, act)
    torch.cuda.synchronize()
    return None if act is None else int(act.cpu().numpy().view(np.uint32)[0])


def _accum_e(name="c2", w=W, h=H, S=2, J=4, n0=0, K=wc.ACCUM_K):
    return ac.expected(name, "crane", w, h, S, J, 1, n0, K, A, R, F, MOVES[name])


def _converge_e(name="c2", w=W, h=H, case=MAIN):
    S, J, E, K = case
    return cc.expected(name, "crane", w, h, S, J, 1, K, M, E, A, R, F, MOVES[name])


# 1. every list, both layouts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(LISTS))
def test_lists(tr, name, layout):
    """accum (0, ACCUM_K) and converge MAIN: every window pixel holds the expected frame's pixel in every buffer, every
    other element its sentinel (in place: the rest of the frame; packed: the spare elements), and `active` counts the
    list's pixels."""
    S, J, E, K = MAIN
    wins = LISTS[name]
    a, c = _accum_e(), _converge_e()
    depth = _set(tr, "c2", c, wins, layout)
    b = Bufs(tr, wins, layout, ACCUM_BUFS)
    _accum(tr, a, depth, S, J, 1, 0, wc.ACCUM_K, b)
    b.check(_want(a, False), f"accum {name}")
    b = Bufs(tr, wins, layout, CONVERGE_BUFS).new_sum()
    active = _converge(tr, c, depth, S, J, 1, K, M, E, b)
    b.check(_want(c, True), f"converge {name}")
    assert active == _active_of(c, wins, M, E), name
    if name == "SCATTER":                                   # the list holds stopped and running pixels
        assert 0 < active < int(wl.mask(wins).sum())


# 2. a partition is the un-windowed call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["TILING", "BANDS"])
def test_a_partition_is_the_unwindowed_call(tr, plan):
    """One call on TILING, and the three ranks' BANDS one after the other, into one set of full-frame buffers: the bytes
    of one un-windowed call, and the `active` values sum to its `active`."""
    S, J, E, K = MAIN
    a, c = _accum_e(), _converge_e()
    calls = [wl.TILING] if plan == "TILING" else wl.BANDS
    scene, depth = sc.scene_of("c2")
    tr.set_scene(scene)
    tr.set_motion(c["d"])
    m = hc.motion_abi(c["motion"])
    flags = dict(rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    ba = Bufs(tr, [WHOLE], "inplace", ACCUM_BUFS)
    bc = Bufs(tr, [WHOLE], "inplace", CONVERGE_BUFS).new_sum()
    total = 0
    for wins in calls:
        tr.set_windows(W, H, wins, "inplace")
        _accum(tr, a, depth, S, J, 1, 0, wc.ACCUM_K, ba)
        total += _converge(tr, c, depth, S, J, 1, K, M, E, bc)
    ha, hcv = ba.check(_want(a, False), plan), bc.check(_want(c, True), plan)
    assert total == c["active"]
    bufs, acc = tr.render_accum(c["cam"], m, W, H, depth, S, J, 1, 0, wc.ACCUM_K, A, R, F, **flags)
    torch.cuda.synchronize()
    assert acc.cpu().numpy().tobytes() == ha["accum"].tobytes()
    for k in OUTS:
        assert bufs[k].cpu().numpy().tobytes() == ha[k].tobytes(), k
    bufs, st, act = tr.render_converge(c["cam"], m, W, H, depth, S, J, 1, K, M, E, A, R, F, **flags)
    torch.cuda.synchronize()
    for k, x in zip(("accum", "accum2", "count"), st):
        assert x.cpu().numpy().tobytes() == hcv[k].tobytes(), k
    for k in OUTS:
        assert bufs[k].cpu().numpy().tobytes() == hcv[k].tobytes(), k
    assert int(act.cpu()[0]) == total


# 3. the order of the list ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_order_changes_nothing_but_packed_offsets(tr, layout):
    S, J, E, K = MAIN
    c = _converge_e()
    base = wl.SCATTER + [(0, 8, 2, 3)]
    shuffled = [base[k] for k in (3, 0, 4, 2, 1)]
    seen = []
    for wins in (base, base[::-1], shuffled):
        depth = _set(tr, "c2", c, wins, layout)
        b = Bufs(tr, wins, layout, CONVERGE_BUFS).new_sum()
        assert _converge(tr, c, depth, S, J, 1, K, M, E, b) == _active_of(c, base, M, E)
        seen.append(b.check(_want(c, True), f"order {wins}"))     # packed: against the new offsets
    if layout == "inplace":
        for other in seen[1:]:
            for n in CONVERGE_BUFS:
                assert other[n].tobytes() == seen[0][n].tobytes(), n


# 4. ONE is the single-window call on the whole frame and the un-windowed call -----------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_equals_the_window_call_and_the_unwindowed_call(tr, layout):
    S, J, E, K = MAIN
    c = _converge_e()
    depth = _set(tr, "c2", c, wl.ONE, layout)
    m = hc.motion_abi(c["motion"])
    flags = dict(rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    lb, lacc = tr.render_accum_windows(c["cam"], m, W, H, depth, S, J, 1, 0, wc.ACCUM_K, A, R, F, **flags)
    wb, wacc = tr.render_accum_window(c["cam"], m, W, H, WHOLE, depth, S, J, 1, 0, wc.ACCUM_K, A, R, F, **flags)
    ub, uacc = tr.render_accum(c["cam"], m, W, H, depth, S, J, 1, 0, wc.ACCUM_K, A, R, F, **flags)
    torch.cuda.synchronize()
    for other, oacc in ((wb, wacc), (ub, uacc)):
        assert lacc.cpu().numpy().tobytes() == oacc.cpu().numpy().tobytes()
        for k in OUTS:
            assert lb[k].cpu().numpy().tobytes() == other[k].cpu().numpy().tobytes(), k
    assert tuple(lacc.shape) == ((W * H, 3) if layout == "packed" else (H, W, 3))
    lb, lst, lact = tr.render_converge_windows(c["cam"], m, W, H, depth, S, J, 1, K, M, E, A, R, F, **flags)
    wb, wst, wact = tr.render_converge_window(c["cam"], m, W, H, WHOLE, depth, S, J, 1, K, M, E, A, R, F, **flags)
    ub, ust, uact = tr.render_converge(c["cam"], m, W, H, depth, S, J, 1, K, M, E, A, R, F, **flags)
    torch.cuda.synchronize()
    for other, ost in ((wb, wst), (ub, ust)):
        for x, y in zip(lst, ost):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        for k in OUTS:
            assert lb[k].cpu().numpy().tobytes() == other[k].cpu().numpy().tobytes(), k
    assert int(lact.cpu()[0]) == int(wact.cpu()[0]) == int(uact.cpu()[0]) == c["active"]


# 5. every instance at every shape ----------------------------------------------------------------------------------------
def _free_pixel(win, w, h):
    """A one-pixel window of the w x h frame outside `win`."""
    x0, y0, ww, hh = win
    for x, y in ((w - 1, h - 1), (0, h - 1), (w - 1, 0), (0, 0)):
        if not (x0 <= x < x0 + ww and y0 <= y < y0 + hh):
            return (x, y, 1, 1)
    raise AssertionError(win)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("S,J,w,h", SHAPES)
@pytest.mark.parametrize("name", ["c2", "tree_demo"])
def test_variants(tr, name, S, J, w, h, layout):
    """c2 depth 1: the opaque instances; tree_demo depth 5: the ray-tree ones; S = 1, 2, 4, 8; a two-window list."""
    win = wc.SHAPE_WINDOWS[(S, J, w, h)]
    wins = [win, _free_pixel(win, w, h)]
    a = _accum_e(name, w, h, S, J)
    depth = _set(tr, name, a, wins, layout, w, h)
    b = Bufs(tr, wins, layout, ACCUM_BUFS, w, h)
    _accum(tr, a, depth, S, J, 1, 0, wc.ACCUM_K, b, w, h)
    b.check(_want(a, False), f"accum {name} S={S}")
    c = _converge_e(name, w, h, (S, J, INST_E, INST_K))
    b = Bufs(tr, wins, layout, CONVERGE_BUFS, w, h).new_sum()
    active = _converge(tr, c, depth, S, J, 1, INST_K, M, INST_E, b, w, h)
    b.check(_want(c, True), f"converge {name} S={S}")
    assert active == _active_of(c, wins, M, INST_E)


# 6. continuation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_split_calls(tr, layout):
    """(0, 2) then (2, 1) equals (0, 3); 6 then 10 converging passes equal 16; the calls' counters sum."""
    S, J, E, K = MAIN
    a, c = _accum_e(), _converge_e()
    depth = _set(tr, "c2", c, wl.SCATTER, layout)
    b = Bufs(tr, wl.SCATTER, layout, ACCUM_BUFS)
    first_rc = _dev(tr, b.blank("raycount"))
    _accum(tr, a, depth, S, J, 1, 0, 2, b, bufs={**b.bufs(), "raycount": first_rc})
    _accum(tr, a, depth, S, J, 1, 2, 1, b)
    want = dict(_want(a, False), raycount=_accum_e(n0=2, K=1)["rc2"])
    host = b.check(want, "accum (0, 2) + (2, 1)")
    # each call's counters are its own passes' (the oracle's sum over both calls is a["rc2"])
    _same("raycount", first_rc.cpu().numpy(), _layout_of("raycount", _accum_e(K=2)["rc2"], wl.SCATTER, layout), "(0, 2)")
    assert np.array_equal(np.asarray(_accum_e(K=2)["rc2"]) + want["raycount"], a["rc2"]) and host is not None
    b = Bufs(tr, wl.SCATTER, layout, CONVERGE_BUFS).new_sum()
    _converge(tr, c, depth, S, J, 1, 6, M, E, b)
    active = _converge(tr, c, depth, S, J, 1, 10, M, E, b)
    b.check(_want(c, True), "converge 6 + 10", names=[n for n in CONVERGE_BUFS if n != "raycount"])
    assert active == _active_of(c, wl.SCATTER, M, E)


@pytest.mark.parametrize("first", ["unwindowed", "window", "list"])
def test_list_calls_and_the_other_calls_continue_each_other(tr, first):
    """Six passes by one kind of call, ten more by another, in place in one set of full-frame buffers.  The pixels of
    SCATTER get both calls and hold the state of sixteen passes; every other pixel holds what the one call that owned it
    left (the un-windowed call's six or ten passes) or was never touched (the single-window calls)."""
    S, J, E, K = MAIN
    fo = cc.frames("c2", "crane", W, H, S, J, 1, A, R, F, MOVES["c2"])
    six = cc.converge(fo, cc.zero_state(H, W), 6, M, E)
    c = _converge_e()
    depth = _set(tr, "c2", c, wl.SCATTER, "inplace")
    m = hc.motion_abi(c["motion"])
    b = Bufs(tr, [WHOLE], "inplace", CONVERGE_BUFS).new_sum()
    names = [n for n in CONVERGE_BUFS if n != "raycount"]
    act = torch.zeros((1,), dtype=torch.int32, device=torch.device("cuda", tr.device))

    def unwindowed(K):
        tr.render_converge_into(c["cam"], m, W, H, depth, S, J, 1, K, M, E, A, R, F, b.state(), b.bufs(), act)

    def windows(K):
        for win in wl.SCATTER:
            tr.render_converge_window_into(c["cam"], m, W, H, win, depth, S, J, 1, K, M, E, A, R, F, b.state(), b.bufs(),
                                           act)

    def lst(K):
        tr.render_converge_windows_into(c["cam"], m, W, H, depth, S, J, 1, K, M, E, A, R, F, b.state(), b.bufs(), act)

    inside = wl.mask(wl.SCATTER)
    want16, want6 = _want(c, True), _want(six, True)
    if first == "list":
        # the list first: its pixels hold six passes, the others nothing; then the whole frame gets ten more
        lst(6)
        rest = cc.converge(fo, cc.zero_state(H, W), 10, M, E)
        unwindowed(10)
        mixed = {n: np.where(inside if np.ndim(want16[n]) == 2 else inside[..., None], want16[n], _want(rest, True)[n])
                 for n in names}
        b.check(mixed, "list then un-windowed", names=names)
        assert int(act.cpu()[0]) == int((~cc.stopped(*[mixed[k] for k in ("accum", "accum2", "count")], M, E)).sum())
        return
    (unwindowed if first == "unwindowed" else windows)(6)
    lst(10)
    outside = want6 if first == "unwindowed" else {n: np.full(np.shape(want16[n]), wc.BUFFERS[n][2]) for n in names}
    if first == "window":
        outside["count"] = np.zeros((H, W), np.int64)         # new_sum() zeroed the whole frame's counts
    mixed = {n: np.where(inside if np.ndim(want16[n]) == 2 else inside[..., None], want16[n], outside[n]) for n in names}
    host = b.host()
    for n in names:
        _same(n, host[n], _typed(n, mixed[n]), f"{first} then list")
    assert int(act.cpu()[0]) == _active_of(c, wl.SCATTER, M, E)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_resume_under_a_smaller_tolerance(tr, layout):
    S, J = 2, 4
    fo = cc.frames("c2", "crane", W, H, S, J, 1, A, R, F, MOVES["c2"])
    a = cc.converge(fo, cc.zero_state(H, W), 6, M, 1.0 / 8.0)
    e = cc.converge(fo, cc.state_of(a), 10, M, 1.0 / 32.0)
    inside = wl.mask(wl.SCATTER)
    assert (e["received"][inside] > 0).any() and (a["n"][inside] < 6).any()
    x = _converge_e()
    depth = _set(tr, "c2", x, wl.SCATTER, layout)
    b = Bufs(tr, wl.SCATTER, layout, CONVERGE_BUFS).new_sum()
    assert _converge(tr, x, depth, S, J, 1, 6, M, 1.0 / 8.0, b) == _active_of(a, wl.SCATTER, M, 1.0 / 8.0)
    b.check(_want(a, True), "loose")
    assert _converge(tr, x, depth, S, J, 1, 10, M, 1.0 / 32.0, b) == _active_of(e, wl.SCATTER, M, 1.0 / 32.0)
    b.check(_want(e, True), "resumed")


# 7. the launch split and the grid's fold ------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"RT_ACCUM_MAX_PASSES": "1"}, {"RT_ACCUM_MAX_PASSES": "3", "RT_WINDOW_GRID_X": "4"}],
                         ids=["1", "3-folded"])
def test_launch_split_is_invisible_in_a_fresh_process(tmp_path, env):
    """A process of its own (tests/window_list_common.py as a module) under RT_ACCUM_MAX_PASSES = 1 and = 3 — the second
    with the ten tiles of SCATTER folded into rows of four, two padding waves behind them: the default's bytes."""
    out = tmp_path / "child.npz"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.window_list_common", str(out)], cwd=root,
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(np.load(out))
    for prefix, want in (("a_", _want(_accum_e(), False)), ("c_", _want(_converge_e(), True))):
        for n, v in want.items():
            _same(n, got[prefix + n], wl.pack(_typed(n, v), wl.SCATTER), f"{env} {prefix}")
    assert int(got["c_active"].view(np.uint32)[0]) == _active_of(_converge_e(), wl.SCATTER, M, MAIN[2])


def test_a_folded_grid_gives_the_same_bytes(monkeypatch):
    """PIXELS under RT_WINDOW_GRID_X = 8 (read when the context is created): 209 tiles as 27 rows of the grid, seven
    padding waves."""
    S, J, E, K = MAIN
    monkeypatch.setenv("RT_WINDOW_GRID_X", "8")
    t = Tracer(0)
    try:
        c = _converge_e()
        depth = _set(t, "c2", c, wl.PIXELS, "packed")
        b = Bufs(t, wl.PIXELS, "packed", CONVERGE_BUFS).new_sum()
        assert _converge(t, c, depth, S, J, 1, K, M, E, b) == c["active"]
        b.check(_want(c, True), "folded")
    finally:
        t.close()


# 8. each output alone, none, no active -----------------------------------------------------------------------------------
@pytest.mark.parametrize("only", OUTS + (None,))
def test_nullable_outputs(tr, only):
    S, J, E, K = MAIN
    a, c = _accum_e(), _converge_e()
    depth = _set(tr, "c2", c, wl.SCATTER, "packed")
    names = ("accum",) + ((only,) if only else ())
    b = Bufs(tr, wl.SCATTER, "packed", names)
    _accum(tr, a, depth, S, J, 1, 0, wc.ACCUM_K, b, bufs={only: b.full[only]} if only else {})
    b.check(_want(a, False), f"accum with {only}")
    b = Bufs(tr, wl.SCATTER, "packed", ("accum2", "count") + names).new_sum()
    _converge(tr, c, depth, S, J, 1, K, M, E, b, bufs={only: b.full[only]} if only else {}, active=False)
    b.check(_want(c, True), f"converge with {only}")


# 9. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_of_a_converging_list_call(fresh):
    """A capture of ten passes on SCATTER, in place, continuing a state of six; two replays, each from the restored
    state, sentinel images and a spoilt active word (its reset is a memset node of the call)."""
    S, J = 2, 4
    fo = cc.frames("c2", "crane", W, H, S, J, 1, A, R, F, MOVES["c2"])
    a = cc.converge(fo, cc.zero_state(H, W), 6, M, 1.0 / 8.0)
    e = cc.converge(fo, cc.state_of(a), 10, M, 1.0 / 32.0)
    x = _converge_e()
    depth = _set(fresh, "c2", x, wl.SCATTER, "inplace")
    m = hc.motion_abi(x["motion"])
    b = Bufs(fresh, wl.SCATTER, "inplace", CONVERGE_BUFS)
    active = torch.zeros((1,), dtype=torch.int32, device=b.full["count"].device)
    render_into = lambda s: fresh.render_converge_windows_into(x["cam"], m, W, H, depth, S, J, 1, 10, M, 1.0 / 32.0,  # noqa: E731
                                                               A, R, F, b.state(), b.bufs(), active, stream=s)

    def restore():
        for n in b.full:
            b.full[n].copy_(_dev(fresh, b.blank(n)))
        for n, key in (("accum", "acc"), ("accum2", "sq"), ("count", "n")):
            b.put(n, a[key])
        active.fill_(12345)
        torch.cuda.synchronize()

    def check(what):
        b.check(_want(e, True), what)
        assert int(active.cpu().numpy()[0]) == _active_of(e, wl.SCATTER, M, 1.0 / 32.0), what

    s = torch.cuda.Stream()
    restore()
    with torch.cuda.stream(s):
        render_into(s)                                                           # the eager call
    s.synchronize()
    check("eager")
    g = torch.cuda.CUDAGraph()
    restore()
    with torch.cuda.graph(g, stream=s):
        render_into(s)
    for k in range(2):
        restore()
        g.replay()
        check(f"replay {k} of 2")


# 10. errors write nothing --------------------------------------------------------------------------------------------------
def test_errors_write_nothing(fresh):
    S, J, E, K = MAIN
    t = fresh
    e = _converge_e()
    scene, depth = sc.scene_of("c2")
    t.set_scene(scene)
    t.set_motion(e["d"])
    cam, m = e["cam"], hc.motion_abi(e["motion"])
    b = Bufs(t, wl.SCATTER, "inplace", CONVERGE_BUFS)
    active = torch.full((1,), -7, dtype=torch.int32, device=b.full["count"].device)
    L = abi.lib()
    p = lambda n: None if n is None else ctypes.c_void_p(b.full[n].data_ptr())  # noqa: E731

    def accum(w=W, h=H, S=2, J=4, n0=0, K=3, acc="accum"):
        return L.rt_render_accum_windows_dev(t._ctx, ctypes.byref(cam), ctypes.byref(m), w, h, depth, S, J, 1, n0, K, A, R,
                                             F, p(acc), p("rgba32f"), p("rgba8"), p("rgb64f"), p("raycount"),
                                             lg.stream_ptr())

    def converge(w=W, h=H, S=2, J=4, K=K, Mp=M, E=E, acc="accum", acc2="accum2", count="count"):
        return L.rt_render_converge_windows_dev(t._ctx, ctypes.byref(cam), ctypes.byref(m), w, h, depth, S, J, 1, K, Mp, E,
                                                A, R, F, p(acc), p(acc2), p(count), p("rgba32f"), p("rgba8"),
                                                p("rgb64f"), p("raycount"), ctypes.c_void_p(active.data_ptr()),
                                                lg.stream_ptr())

    def untouched(what):
        torch.cuda.synchronize()
        for n, arr in b.host().items():
            assert (arr == wc.BUFFERS[n][2]).all(), f"{what}: a rejected call wrote {n}"
        assert int(active.cpu()[0]) == -7, what

    for call in (accum, converge):                          # no list set
        assert call() == abi.RT_EINVAL and "window" in abi.last_error(), call.__name__
    untouched("no list")
    t.set_windows(W, H, wl.SCATTER, "inplace")
    for call in (accum, converge):
        # another frame than the list's
        assert call(w=W + 1) == abi.RT_EINVAL and "window" in abi.last_error()
        assert call(h=H - 1) == abi.RT_EINVAL and "window" in abi.last_error()
        # the un-windowed call's own checks, one of each family
        assert call(acc=None) == abi.RT_EINVAL and "accum" in abi.last_error()
        assert call(K=0) == abi.RT_EINVAL and "passes" in abi.last_error()
        assert call(K=65537) == abi.RT_EINVAL and "passes" in abi.last_error()
        assert call(J=3) == abi.RT_EINVAL and "jitter" in abi.last_error()
        assert call(S=3) == abi.RT_EINVAL and "samples" in abi.last_error()
        assert call(w=0) == abi.RT_EINVAL
    assert accum(n0=2 ** 31 - 1, K=2) == abi.RT_EINVAL and "first_pass" in abi.last_error()
    assert converge(acc2=None) == abi.RT_EINVAL and "accum2" in abi.last_error()
    assert converge(count=None) == abi.RT_EINVAL and "count" in abi.last_error()
    assert converge(Mp=1) == abi.RT_EINVAL and "min_passes" in abi.last_error()
    assert converge(E=-1.0) == abi.RT_EINVAL and "tolerance" in abi.last_error()
    untouched("bad arguments")
    # a failed rt_set_windows leaves the list in force.  The entry point itself, on this context: two windows sharing
    # one pixel, a window listed twice, a window off the frame, an empty one, n = 0 with a non-null array, n = 4097,
    # an unknown layout, a null array with n > 0, another frame's bad size
    def set_windows(wins, n=None, layout=abi.RT_WINDOWS_IN_PLACE, w=W, h=H, null=False):
        arr = (abi.rt_window * max(len(wins), 1))(*[abi.rt_window(x0, y0, ww, hh, 0) for x0, y0, ww, hh in wins])
        return L.rt_set_windows(t._ctx, w, h, None if null else arr, len(wins) if n is None else n, layout)

    for kw, names in ((dict(wins=[(3, 2, 7, 5), (9, 6, 4, 4)]), "window"),
                      (dict(wins=wl.SCATTER + [wl.SCATTER[0]]), "window"),
                      (dict(wins=[(3, 2, 7, 5), (16, 0, 4, 4)]), "window"),
                      (dict(wins=[(3, 2, 7, 5), (0, 0, 0, 4)]), "window"),
                      (dict(wins=[(0, 0, 1, 1)], n=0), "n "),
                      (dict(wins=[(k, 0, 1, 1) for k in range(4097)], w=4097, h=1), "n "),
                      (dict(wins=wl.SCATTER, layout=2), "layout"),
                      (dict(wins=wl.SCATTER, null=True), "wins"),
                      (dict(wins=wl.SCATTER, w=0), "width")):
        assert set_windows(**kw) == abi.RT_EINVAL and names in abi.last_error(), (kw, abi.last_error())
    # and through the Tracer, which remembers the list in force too
    for bad in ([(3, 2, 7, 5), (9, 6, 4, 4)], [(16, 0, 4, 4)], []):
        with pytest.raises(abi.RtError):
            t.set_windows(W, H, bad, "inplace")
    with pytest.raises(ValueError):
        t.set_windows(W, H, wl.SCATTER, "dense")
    assert t._windows == (W, H, "inplace", W * H)
    untouched("failed set_windows")
    t.set_scene(scene)                                      # rt_set_scene keeps the list, and so does another scene
    other, _ = sc.scene_of("c5")
    t.set_scene(other)
    t.set_scene(scene)
    t.set_motion(e["d"])
    b.new_sum()
    assert converge() == abi.RT_OK, abi.last_error()
    torch.cuda.synchronize()
    assert int(active.cpu().numpy().view(np.uint32)[0]) == _active_of(e, wl.SCATTER, M, E)
    b.check(_want(e, True), "the old list, after the errors")
    # a cleared list
    t.set_windows(W, H, None)
    b = Bufs(t, wl.SCATTER, "inplace", CONVERGE_BUFS)
    active.fill_(-7)
    for call in (accum, converge):
        assert call() == abi.RT_EINVAL and "window" in abi.last_error(), call.__name__
    untouched("cleared list")
    with pytest.raises(ValueError):
        t.render_accum_windows_into(cam, m, W, H, depth, 2, 4, 1, 0, 3, A, R, F, b.full["accum"], {})
    t.set_windows(W, H, wl.SCATTER, "packed")
    dev = torch.device("cuda", t.device)
    with pytest.raises(ValueError):                          # too few elements
        t.render_accum_windows_into(cam, m, W, H, depth, 2, 4, 1, 0, 3, A, R, F,
                                    torch.empty((71, 3), dtype=torch.float64, device=dev), {})
    with pytest.raises(ValueError):                          # the wrong type
        t.render_accum_windows_into(cam, m, W, H, depth, 2, 4, 1, 0, 3, A, R, F,
                                    torch.empty((72, 3), dtype=torch.float32, device=dev), {})
    with pytest.raises(ValueError):                          # another frame
        t.render_accum_windows_into(cam, m, W + 1, H, depth, 2, 4, 1, 0, 3, A, R, F,
                                    torch.empty((72, 3), dtype=torch.float64, device=dev), {})


# 11. the context's other state ---------------------------------------------------------------------------------------------
def test_no_side_effect(fresh):
    """A view's first, calibration and cached renders, a shutter render and a single-window call; then list calls of both
    kinds; then the three again: equal bytes."""
    w, h = lg.W, lg.H
    scene, depth = sc.scene_of("c2")
    fresh.set_scene(scene)
    fresh.set_motion(mc.displacement(scene, MOVES["c2"]))
    cam = scenes.make_camera(w, h, 500.0 / w)
    frames = lg.view_frames(fresh, scene, cam, depth)
    flags = dict(rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    e = _converge_e()
    m = hc.motion_abi(e["motion"])

    def others():
        sh = _host(fresh.render_shutter(e["cam"], m, W, H, depth, 2, 4, 1, A, R, F, **flags))
        wb, wacc = fresh.render_accum_window(e["cam"], m, W, H, wc.UNALIGNED, depth, 2, 4, 1, 0, 3, A, R, F, **flags)
        return [sh, dict(_host(wb), accum=wacc.cpu().numpy())]

    before = others()
    for layout in LAYOUTS:
        fresh.set_windows(W, H, wl.SCATTER, layout)
        fresh.render_accum_windows(e["cam"], m, W, H, depth, 2, 4, 1, 0, 3, A, R, F, **flags)
        bufs, st, act = fresh.render_converge_windows(e["cam"], m, W, H, depth, 2, 4, 1, 16, M, MAIN[2], A, R, F, **flags)
    sc.assert_same_bits(_host(bufs)["rgb64f"], wl.pack(e["mean"], wl.SCATTER), "the last list call")
    assert int(act.cpu()[0]) == _active_of(e, wl.SCATTER, M, MAIN[2])
    lg.check_view_unchanged(frames, _host(fresh.render(cam, w, h, depth, **flags)))
    for x, y in zip(before, others()):
        for key in x:
            assert x[key].tobytes() == y[key].tobytes(), key


# 12. host buffers; the CLI -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_conveniences(tr, layout):
    S, J, seed, wins = 2, 4, 1, wl.SCATTER
    a2, a3 = _accum_e(K=2), _accum_e(n0=2, K=1)
    fo = cc.frames("c2", "crane", W, H, S, J, seed, A, R, F, MOVES["c2"])
    c6 = cc.converge(fo, cc.zero_state(H, W), 6, M, 1.0 / 8.0)
    c16 = cc.converge(fo, cc.state_of(c6), 10, M, 1.0 / 32.0)
    scene, depth = sc.scene_of("c2")
    s_abi = scene.to_abi()
    d = np.ascontiguousarray(a2["d"])
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    m = hc.motion_abi(a2["motion"])
    arr = (abi.rt_window * len(wins))(*[abi.rt_window(x0, y0, w, h, 0) for x0, y0, w, h in wins])
    code = wl.LAYOUTS[layout]
    L = abi.lib()
    inside = wl.mask(wins)
    blank = lambda n: _blank(n, wins, layout, (H, W))  # noqa: E731
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731

    def check(host, want, what):
        for n, x in host.items():
            _same(n, x, _layout_of(n, want[n], wins, layout), what)

    def stats_of(st, rc, prim):
        assert st.primary_rays == prim and st.reflect_rays == int(rc[..., 0][inside].sum(dtype=np.uint64)) - prim
        assert st.shadow_rays == int(rc[..., 1][inside].sum(dtype=np.uint64))

    host = {n: blank(n) for n in ("accum", "rgba32f", "rgba8", "rgb64f")}
    for n0, K, e in ((0, 2, a2), (2, 1, a3)):
        st = abi.rt_stats()
        abi.check(L.rt_render_accum_windows(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(a2["cam"]), ctypes.byref(m), W,
                                            H, depth, S, J, seed, n0, K, A, R, F, ptr(host["accum"]),
                                            ptr(host["rgba32f"]), ptr(host["rgba8"]), ptr(host["rgb64f"]),
                                            ctypes.byref(st), arr, len(wins), code), "rt_render_accum_windows")
        check(host, _want(e, False), f"host accum ({n0}, {K})")
        stats_of(st, e["rc2"], int(inside.sum()) * S * S * K)
    host = {n: blank(n) for n in ("accum", "accum2", "count", "rgba32f", "rgba8", "rgb64f")}
    host["count"] = _layout_of("count", np.zeros((H, W), np.int64), wins, layout)
    for K, E, e in ((6, 1.0 / 8.0, c6), (10, 1.0 / 32.0, c16)):
        st, n_active = abi.rt_stats(), ctypes.c_uint64(99)
        abi.check(L.rt_render_converge_windows(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(a2["cam"]), ctypes.byref(m),
                                               W, H, depth, S, J, seed, K, M, E, A, R, F, ptr(host["accum"]),
                                               ptr(host["accum2"]), ptr(host["count"]), ptr(host["rgba32f"]),
                                               ptr(host["rgba8"]), ptr(host["rgb64f"]), ctypes.byref(st),
                                               ctypes.byref(n_active), arr, len(wins), code),
                  "rt_render_converge_windows")
        check(host, _want(e, True), f"host converge K={K}")
        assert n_active.value == _active_of(e, wins, M, E)
        stats_of(st, e["rc2"], int(e["received"][inside].sum()) * S * S)
    # a bad list is rejected before anything is written or set
    bad = (abi.rt_window * 2)(abi.rt_window(3, 2, 7, 5, 0), abi.rt_window(9, 6, 4, 4, 0))
    before = {n: x.copy() for n, x in host.items()}
    assert L.rt_render_accum_windows(tr._ctx, ctypes.byref(s_abi), dp, ctypes.byref(a2["cam"]), ctypes.byref(m), W, H,
                                     depth, S, J, seed, 0, 2, A, R, F, ptr(host["accum"]), ptr(host["rgba32f"]),
                                     ptr(host["rgba8"]), ptr(host["rgb64f"]), None, bad, 2, code) == abi.RT_EINVAL
    assert "window" in abi.last_error()
    for n in host:
        assert host[n].tobytes() == before[n].tobytes(), n


def _read_ppm(path, w, h):
    hdr, body = open(path, "rb").read().split(b"\n", 1)
    assert hdr.split() == [b"P6", str(w).encode(), str(h).encode(), b"255"]
    return np.frombuffer(body, np.uint8).reshape(h, w, 3)


def test_cli_writes_the_scattered_frame(tmp_path):
    motion = ((12.0, 30.0, -16.0), (50.0, 20.0, 0.0))
    wins = wl.SCATTER
    inside = wl.mask(wins, lg.W, lg.H)
    c = cc.expected("c2", motion, lg.W, lg.H, 2, 4, 7, 8, 4, 0.03125, 8.0, 0.0, 0.5, MOVES["c2"])
    a = ac.expected("c2", motion, lg.W, lg.H, 2, 4, 7, 0, 3, 8.0, 0.0, 0.5, MOVES["c2"])
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c2_windows.ppm"
    base = [exe, "--config", "c2", "--width", str(lg.W), "--height", str(lg.H), "--samples", "2", "--shutter", "0.5",
            "--move", "4:50,0,0", "--move", "0:0,12,-30", "--aperture", "8", "--eye-move", "12,30,-16", "--look-move",
            "50,20,0", "--jitter", "4", "--seed", "7", "--out", str(out), "--windows",
            ":".join(",".join(str(v) for v in w) for w in wins)]
    r = subprocess.run(base + ["--passes", "8", "--tolerance", "0.03125"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    npx = int(inside.sum())
    active, traced = _active_of(c, wins, 4, 0.03125), int(c["n"][inside].sum())
    assert f"{active} of {npx} pixels still active" in r.stdout, r.stdout
    assert f"{traced} of {8 * npx} pixel-passes traced" in r.stdout and f"{4 * traced} primary rays" in r.stdout, r.stdout
    want = wl.scatter(sc.to_rgba8(c["mean"]), wins, 0)[::-1, :, :3]             # PPM rows run top to bottom
    assert np.array_equal(_read_ppm(out, lg.W, lg.H), want)
    r = subprocess.run(base + ["--passes", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "accumulated, 3 passes" in r.stdout and f"{npx * 4 * 3} primary rays" in r.stdout, r.stdout
    assert np.array_equal(_read_ppm(out, lg.W, lg.H), wl.scatter(sc.to_rgba8(a["mean"]), wins, 0)[::-1, :, :3])
    r = subprocess.run(base + ["--passes", "3", "--windows", "3,2,7,5:9,6,4,4"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "window" in r.stderr
    r = subprocess.run(base[:-2] + ["--windows", "3,2,7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--windows" in r.stderr
