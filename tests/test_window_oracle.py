"""CPU: windows of the accumulating and converging renders (include/rt_api.h: windows of the accumulating and converging
renders).  The symbols; the rejection of every bad window before any device work; distributed.window_plan; the CLI's
usage errors; and the two conditions that make the cases of tests/test_gpu_window.py discriminating — a window is the
shifted camera's frame at J = 1 and is not at J = 4 (so a kernel keyed by window-local coordinates, or by the window's
width, shows), and every window of the list holds stopped and running pixels of the converging MAIN case.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ray_tracer_fragment_shader_amd import abi, distributed, scenes
from ray_tracer_fragment_shader_amd.tracer import Tracer

from . import converge_common as cc
from . import motion_common as mc
from . import shutter_common as hc
from . import ssaa_common as sc
from . import window_common as wc
from .test_converge_oracle import MAIN
from .test_jitter_oracle import SHAPES

W, H, A, R, F, M = wc.W, wc.H, wc.A, wc.R, wc.F, wc.M
MOVES = mc.MOVES
NAMES = ("rt_render_accum_window_dev", "rt_render_converge_window_dev", "rt_render_accum_window",
         "rt_render_converge_window")
# every way a window of the 19 x 11 frame can be wrong: (x0, y0, w, h, stride)
BAD_WINDOWS = [(-1, 0, 4, 4, 4), (0, -1, 4, 4, 4), (0, 0, 0, 4, 4), (0, 0, 4, 0, 4), (0, 0, -3, 4, 4), (0, 0, 4, -3, 4),
               (16, 0, 4, 4, 4), (0, 8, 4, 4, 4), (0, 0, 20, 11, 20), (0, 0, 19, 12, 19), (19, 0, 1, 1, 1),
               (0, 11, 1, 1, 1), (2 ** 31 - 1, 0, 2, 1, 2), (0, 2 ** 31 - 1, 1, 2, 1), (3, 2, 7, 5, 6), (3, 2, 7, 5, 0),
               (3, 2, 7, 5, -7)]


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    for name in NAMES:
        assert name in abi.SIGNATURES and hasattr(abi.lib(), name), name


def test_symbols_and_signatures():
    for name, n in zip(NAMES, (21, 25, 22, 26)):
        assert len(abi.SIGNATURES[name][1]) == n, name
    # one more argument than the un-windowed call, the window, right after the frame's size
    for name in NAMES:
        parent = abi.SIGNATURES[name.replace("_window", "")][1]
        args = abi.SIGNATURES[name][1]
        k = args.index(ctypes.POINTER(abi.rt_window))
        assert args[:k] + args[k + 1:] == parent and args[k - 2:k] == [ctypes.c_int, ctypes.c_int], name
    assert [f[0] for f in abi.rt_window._fields_] == ["x0", "y0", "width", "height", "stride"]
    assert ctypes.sizeof(abi.rt_window) == 20
    assert abi.lib().rt_abi_version() == 10
    for method in ("render_accum_window_into", "render_accum_window", "render_converge_window_into",
                   "render_converge_window"):
        assert callable(getattr(Tracer, method))
    assert callable(distributed.window_plan)


def _calls(win):
    """The four entry points with `win` (an abi.rt_window or None) on a null context and null buffers: a window is
    checked before anything that needs a device."""
    L = abi.lib()
    cam = scenes.make_camera(W, H, 1.0)
    wp = None if win is None else ctypes.byref(win)
    return [
        lambda: L.rt_render_accum_window_dev(None, ctypes.byref(cam), None, W, H, wp, 1, 2, 4, 1, 0, 3, A, R, F, None, None, None,
                                     None, None, None),
        lambda: L.rt_render_converge_window_dev(None, ctypes.byref(cam), None, W, H, wp, 1, 2, 4, 1, 3, 3, 0.01, A, R, F, None,
                                        None, None, None, None, None, None, None, None),
        lambda: L.rt_render_accum_window(None, None, None, ctypes.byref(cam), None, W, H, wp, 1, 2, 4, 1, 0, 3, A, R, F, None,
                                 None, None, None, None),
        lambda: L.rt_render_converge_window(None, None, None, ctypes.byref(cam), None, W, H, wp, 1, 2, 4, 1, 3, 3, 0.01, A, R, F,
                                    None, None, None, None, None, None, None, None),
    ]


@pytest.mark.parametrize("bad", [None] + BAD_WINDOWS)
def test_bad_windows_are_rejected_before_any_device_work(bad):
    win = None if bad is None else abi.rt_window(*[v if v < 2 ** 31 else v - 2 ** 32 for v in bad])
    L = abi.lib()
    for k, name in enumerate(NAMES):
        rc = _calls(win)[k]()
        assert rc == abi.RT_EINVAL and "window" in abi.last_error() and name in abi.last_error(), (name, bad, abi.last_error())
    assert L.rt_abi_version() == 10


def test_a_good_window_reaches_the_context_check():
    for win in wc.WINDOWS:
        x0, y0, w, h = win
        for stride in (w, w + wc.PAD, W):
            for call in _calls(abi.rt_window(x0, y0, w, h, stride)):
                assert call() == abi.RT_EINVAL and "context" in abi.last_error(), (win, stride, abi.last_error())


def test_tracer_rejects_bad_windows_and_tensors():
    for bad in BAD_WINDOWS[:12] + [(1, 2, 3), "window", None]:
        with pytest.raises(ValueError):
            Tracer._window(None, W, H, bad[:4] if isinstance(bad, tuple) and len(bad) == 5 else bad, {})
    win, ptrs = Tracer._window(None, W, H, wc.UNALIGNED, {"accum": None})
    assert (win.x0, win.y0, win.width, win.height, win.stride) == wc.UNALIGNED + (wc.UNALIGNED[2],) and ptrs == {"accum": None}


# ---- window_plan ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(W, H), (1, 1), (7, 64), (1920, 1080)])
def test_window_plan_partitions_exactly(width, height):
    for parts in list(range(1, min(height, 70) + 1)) + [height, height + 1, 3 * height + 5]:
        plan = distributed.window_plan(width, height, parts)
        assert len(plan) == min(parts, height)
        assert wc.is_partition(plan, width, height), (width, height, parts)
        heights = [h for _, _, _, h in plan]
        assert max(heights) - min(heights) <= 1 and min(heights) >= 1
        assert all(x0 == 0 and w == width for x0, _, w, _ in plan)                # whole rows
        assert [y0 for _, y0, _, _ in plan] == [sum(heights[:k]) for k in range(len(plan))]   # contiguous, bottom up
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, -1)):
        with pytest.raises(ValueError):
            distributed.window_plan(*bad)


def test_the_tests_tiling_is_a_partition():
    assert wc.is_partition(wc.TILING, W, H)
    assert not wc.is_partition(wc.TILING[:-1], W, H) and not wc.is_partition(wc.TILING + [(0, 0, 1, 1)], W, H)
    for (S, J, w, h), win in wc.SHAPE_WINDOWS.items():
        assert (S, J, w, h) in SHAPES
        x0, y0, ww, hh = win
        assert 0 < x0 and x0 + ww <= w and y0 + hh <= h and (ww, hh) != (w, h)
        if S < 8:                                              # (at S = 8 a tile is one pixel: every origin is on the grid)
            assert (S * x0) % 8 != 0 or (S * y0) % 8 != 0      # the origin is off the full frame's tile grid


# ---- the CLI ------------------------------------------------------------------------------------------------------------
def test_cli_usage_errors(tmp_path):
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    size = ["--width", str(W), "--height", str(H)]
    base = size + ["--samples", "2", "--jitter", "4", "--passes", "3"]
    for args, word in ((size + ["--samples", "2", "--jitter", "4", "--window", "3,2,7,5"], "--passes"),
                       (base + ["--window", "3,2,7"], "X,Y,W,H"),
                       (base + ["--window", "3,2,7,5,1"], "X,Y,W,H"),
                       (base + ["--window", "3;2;7;5"], "X,Y,W,H"),
                       (base + ["--window", "a,2,7,5"], "X,Y,W,H"),
                       (base + ["--window", "3,2,7,5x"], "X,Y,W,H"),
                       (base + ["--window", "3.5,2,7,5"], "X,Y,W,H"),
                       (base + ["--window", "13,2,7,5"], "leaves"),
                       (base + ["--window", "3,7,7,5"], "leaves"),
                       (base + ["--window", "-1,2,7,5"], "leaves"),
                       (base + ["--window", "3,2,0,5"], "leaves"),
                       (base + ["--tolerance", "0.03125", "--window", "3,2,7,12"], "leaves")):
        r = subprocess.run([exe, "--config", "c2", "--out", str(tmp_path / "x.ppm")] + args, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert "--window" in r.stderr and word in r.stderr, (args, r.stderr)
        assert not (tmp_path / "x.ppm").exists()


# ---- the cases discriminate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [wc.UNALIGNED, (12, 6, 7, 5)])
def test_the_crop_is_the_shifted_cameras_frame_at_one_sub_position_only(win):
    """A w x h frame of the camera with bottom_x + x0, bottom_y + y0 through the oracle route.  At J = 1 nothing reads the
    sample key, and the frame equals the crop of the full frame bit for bit: the window's geometry by a second route.
    At J = 4 the key is Jr (S w) + I of the SMALL frame: at least a tenth of the window's pixels must differ (the floor
    test_seeds_differ uses for a frame), so a kernel keyed by window-local coordinates or by the window's width shows."""
    x0, y0, w, h = win
    S, seed = 2, 1
    scene, depth = sc.scene_of("c2")
    for J, same in ((1, True), (4, False)):
        full = hc.expected("c2", "crane", W, H, S, J, seed, A, R, F, MOVES["c2"])
        cam = scenes.make_camera(W, H, 500.0 / W)
        cam.bottom_x += x0
        cam.bottom_y += y0
        small = hc.render(scene, cam, full["motion"], w, h, depth, S, J, seed, A, R, F, full["d"])
        want = wc.crop(full["rgb"], win)
        if same:
            sc.assert_same_bits(small["rgb"], want, f"J = 1 {win}")
            assert np.array_equal(small["rc2"], wc.crop(full["rc2"], win))
        else:
            differ = (small["rgb"] != want).any(axis=2).sum()
            assert differ * 10 >= w * h, (win, int(differ), w * h)


def test_every_window_holds_stopped_and_running_pixels():
    S, J, E, K = MAIN
    e = cc.expected("c2", "crane", W, H, S, J, 1, K, M, E, A, R, F, MOVES["c2"])
    open_ = ~cc.stopped(e["acc"], e["sq"], e["n"], M, E)
    assert int(open_.sum()) == e["active"]
    for win in wc.WINDOWS + wc.TILING:
        o = wc.crop(open_, win)
        if o.size == 1:
            continue
        assert o.any() and not o.all(), win
    assert not wc.crop(open_, wc.STOPPED_PIXEL).any() and wc.crop(open_, wc.RUNNING_PIXEL).all()
    assert wc.STOPPED_PIXEL in wc.WINDOWS and wc.RUNNING_PIXEL in wc.WINDOWS
    # a window's active count is the number of its running pixels; the tiles' counts sum to the frame's
    assert sum(int(wc.crop(open_, t).sum()) for t in wc.TILING) == e["active"]
    for parts in (3,):
        assert sum(int(wc.crop(open_, t).sum()) for t in distributed.window_plan(W, H, parts)) == e["active"]
