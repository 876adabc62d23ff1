"""Shared by the tile-class tests (test_tile_classes.py on the CPU, test_gpu_tile_classes.py on the GPU): the host's
class decision (rt_diag_tile_class_plan), what a context's last calibration decided (rt_diag_tile_classes,
rt_diag_tile_class_grid) and the oracle's per-tile truth."""
import ctypes

import numpy as np

from ray_tracer_fragment_shader_amd import abi

TRACE, SKY, SPHERE_FREE = 0, 1, 2      # rt_diag_tile_class_grid


def class_plan(cone, sky, masks, n_spheres):
    """rt_diag_tile_class_plan -> uint8 [tiles]: 1 sphere-free.  cone uint64 [tiles]; sky uint8 [tiles] or None; masks
    uint64 [tiles, slots] or None (no slots)."""
    cone = np.ascontiguousarray(cone, np.uint64)
    tiles = cone.size
    slots = 0 if masks is None else masks.shape[1]
    if masks is not None:
        masks = np.ascontiguousarray(masks, np.uint64)
    if sky is not None:
        sky = np.ascontiguousarray(sky, np.uint8)
    out = np.full(tiles, 7, np.uint8)
    abi.check(abi.lib().rt_diag_tile_class_plan(cone.ctypes.data, sky.ctypes.data if sky is not None else None,
                                                masks.ctypes.data if masks is not None and slots else None, tiles,
                                                slots, n_spheres, out.ctypes.data), "rt_diag_tile_class_plan")
    return out


def class_counts(tracer):
    """rt_diag_tile_classes -> (tiles, sky, sphere_free) of the context's last calibrated view."""
    t, s, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    abi.check(abi.lib().rt_diag_tile_classes(tracer._ctx, ctypes.byref(t), ctypes.byref(s), ctypes.byref(f)),
              "rt_diag_tile_classes")
    return t.value, s.value, f.value


def class_grid(tracer, tiles_y, tiles_x):
    """rt_diag_tile_class_grid -> uint8 [tile rows, tiles_x]: TRACE, SKY or SPHERE_FREE."""
    out = np.full((tiles_y, tiles_x), 7, np.uint8)
    abi.check(abi.lib().rt_diag_tile_class_grid(tracer._ctx, out.ctypes.data, out.size), "rt_diag_tile_class_grid")
    return out


def tiles_any(px):
    """bool [rows, W] -> bool [tile rows, tiles_x]: some valid pixel of the 8 x 8 tile is set."""
    h, w = px.shape
    ty, tx = (h + 7) // 8, (w + 7) // 8
    full = np.zeros((ty * 8, tx * 8), bool)
    full[:h, :w] = px
    return full.reshape(ty, 8, tx, 8).any(axis=(1, 3))
