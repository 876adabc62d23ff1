"""Shared by the sky-tile tests (test_sky_tiles.py on the CPU, test_gpu_sky_tiles.py on the GPU): the scenes and eyes
the verdict is checked on, the host verdict (rt_diag_sky_tiles) and the oracle's per-tile truth."""
import ctypes

import numpy as np

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes

MISS = 1          # a pixel's packed ray counter when its primary ray misses: one segment, no shadow ray


def scene_named(name):
    """c2 / c3 / c5: the benchmark scenes; noboard: c2's spheres without the board; rise: c2's spheres with the far
    corner's sphere replaced by one that stands above the far board edge, against the sky."""
    if name in ("c2", "c3", "c5"):
        return scenes.CONFIGS[name].scene()
    sc = scenes.CONFIGS["c2"].scene()
    if name == "noboard":
        sc.has_board = False
    elif name == "rise":
        sc.spheres[3] = scenes.SphereSpec("d8", 30.0, 80.0)
    else:
        raise KeyError(name)
    return sc


def board_y(scene_abi):
    """Height of the board plane (rt_host.cpp: g_scene position + board position)."""
    return scene_abi.position[1] + scene_abi.board_position[1]


def camera(W, H, eye=None):
    cam = scenes.make_camera(W, H, 500.0 / W)
    if eye is not None:
        cam.eye = abi.vec3(eye)
    return cam


def orbit_eyes():
    """bench.py's moving-camera leg: 16 eyes on an orbit."""
    return [(60.0 * np.sin(2.0 * np.pi * v / 16), 100.0 + 10.0 * np.cos(2.0 * np.pi * v / 16), 200.0)
            for v in range(16)]


def host_verdict(scene_abi, cam, W, H, rows=None):
    """rt_diag_sky_tiles -> uint8 [tile rows, tiles_x]."""
    nl = scenes.local_rows(H, rows)
    tx, ty = (W + 7) // 8, (nl + 7) // 8
    out = np.zeros((ty, tx), np.uint8)
    abi.check(abi.lib().rt_diag_sky_tiles(ctypes.byref(scene_abi), ctypes.byref(cam), W, H,
                                          ctypes.byref(rows) if rows is not None else None, out.ctypes.data,
                                          out.size), "rt_diag_sky_tiles")
    return out


def tiles_all_miss(rc):
    """rc: the oracle's (or the kernel's) ray counters [rows, W] -> bool [tile rows, tiles_x]: every valid pixel of
    the 8 x 8 tile has the miss counter."""
    h, w = rc.shape
    ty, tx = (h + 7) // 8, (w + 7) // 8
    miss = np.ones((ty * 8, tx * 8), bool)
    miss[:h, :w] = rc == MISS
    return miss.reshape(ty, 8, tx, 8).all(axis=(1, 3))


def oracle_rc(scene_abi, cam, W, H, depth=1, rows=None):
    return po.render(scene_abi, cam, W, H, depth, rows)[1]
