"""Shared by the flat-tile tests (test_flat_tiles.py on the CPU, test_gpu_flat_tiles.py on the GPU): what a context's
last calibration decided (rt_diag_flat_tiles, rt_diag_flat_tile_grid), the record word (rt_diag_disp_sky_word) and the
oracle's per-tile truth.

A tile here is the kernel's: 8 x 8 lanes, the lanes past the frame's right edge or its last local row clamped to the last
pixel (render_body traces such a lane on the clamped pixel and stores nothing).  The truth comes from po.intersect
(oracle_intersect) alone: the primary ray of every lane, and for the lanes that hit the board one ray to every light and
the reflected ray."""
import ctypes
import functools

import numpy as np

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes

from . import sky_common as sk

SPHERE_FREE_BIT, FLAT_BIT, RUN_MAX = 0x80000000, 0x40000000, 65535

# (config, W, H) -> (tiles flat in the oracle, tiles with any primary hit), from oracle_truth below
ORACLE_COUNTS = {("c2", 321, 203): (116, 406), ("c2", 320, 184): (113, 396), ("c3", 321, 203): (82, 406),
                 ("c2", 64, 40): (0, 22)}


def flat_counts(tracer):
    """rt_diag_flat_tiles -> (tiles, flat) of the context's last calibrated view."""
    t, f = ctypes.c_int(), ctypes.c_int()
    abi.check(abi.lib().rt_diag_flat_tiles(tracer._ctx, ctypes.byref(t), ctypes.byref(f)), "rt_diag_flat_tiles")
    return t.value, f.value


def flat_grid(tracer, tiles_y, tiles_x):
    """rt_diag_flat_tile_grid -> bool [tile rows, tiles_x]."""
    out = np.full((tiles_y, tiles_x), 7, np.uint8)
    abi.check(abi.lib().rt_diag_flat_tile_grid(tracer._ctx, out.ctypes.data, out.size), "rt_diag_flat_tile_grid")
    assert ((out == 0) | (out == 1)).all()
    return out != 0


def sky_word(run, sphere_free, flat):
    """rt_diag_disp_sky_word -> the record's word, or the error code."""
    w = ctypes.c_uint32(0xDEADBEEF)
    rc = abi.lib().rt_diag_disp_sky_word(run, int(sphere_free), int(flat), ctypes.byref(w))
    return w.value if rc == abi.RT_OK else rc


def flat_gates(name, eye):
    """rt_diag_flat_gates -> (gates, hits_ok, board_skip_y) of scene `name` (sky_common.scene_named) seen from `eye`."""
    sc = sk.scene_named(name).to_abi()
    e = (ctypes.c_double * 3)(*[float(x) for x in eye])
    g, h, y = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_double(0.0)
    abi.check(abi.lib().rt_diag_flat_gates(ctypes.byref(sc), e, ctypes.byref(g), ctypes.byref(h), ctypes.byref(y)),
              "rt_diag_flat_gates")
    return g.value, h.value, y.value


def tiles_all_clamped(px):
    """bool [rows, W] -> bool [tile rows, tiles_x]: all 64 lanes of the tile, clamped lanes included, are set."""
    h, w = px.shape
    ty, tx = (h + 7) // 8, (w + 7) // 8
    full = np.pad(px, ((0, ty * 8 - h), (0, tx * 8 - w)), mode="edge")
    return full.reshape(ty, 8, tx, 8).all(axis=(1, 3))


def tiles_any(px):
    """bool [rows, W] -> bool [tile rows, tiles_x]: some lane of the tile is set (clamped lanes repeat a valid one)."""
    return ~tiles_all_clamped(~px)


@functools.lru_cache(maxsize=None)
def oracle_truth(name, W, H, eye=None, rows_key=None):
    """-> dict of bool [tile rows, tiles_x] grids, from po.intersect on the rays of every lane:
    any_hit   some primary ray of the tile hits something;
    board     all 64 primary rays hit the board (material 0 or 1: a checker square);
    lit       ... and no ray from such a hit point to a light hits anything;
    no_refl   ... and no reflected ray Line(p, reflected_end) hits anything;
    flat      board & lit & no_refl."""
    sc = sk.scene_named(name)
    full = sc.to_abi()
    rows = scenes.rows(*rows_key) if rows_key else None
    cam = sk.camera(W, H, eye)
    sp = po.screen_points(cam, W, H, rows)
    nl = sp.shape[0]
    ends = sp.reshape(-1, 3)
    starts = np.broadcast_to(np.array(cam.eye[:], np.float64), ends.shape).copy()
    h = po.intersect(full, starts, ends)
    hit = h["hit"] != 0
    board = hit & ((h["material"] == 0) | (h["material"] == 1))
    idx = np.flatnonzero(board)
    p, re = h["point"][idx], h["reflected_end"][idx]
    lit = np.zeros(hit.shape, bool)
    no_refl = np.zeros(hit.shape, bool)
    if idx.size:
        blocked = np.zeros(idx.size, bool)
        for lt in sc.lights:
            L = np.broadcast_to(np.array(lt.position(), np.float64), p.shape).copy()
            blocked |= po.intersect(full, p, L)["hit"] != 0
        lit[idx] = ~blocked
        no_refl[idx] = po.intersect(full, p, re)["hit"] == 0
    g = lambda a: tiles_all_clamped(a.reshape(nl, W))
    out = {"any_hit": tiles_any(hit.reshape(nl, W)), "board": g(board), "lit": g(board & lit),
           "no_refl": g(board & no_refl)}
    out["flat"] = out["board"] & out["lit"] & out["no_refl"]
    return out
