"""Lists of windows of the accumulating and converging renders (rt_window_list_plan, rt_set_windows,
rt_render_accum_windows_dev, rt_render_converge_windows_dev): the lists, a numpy restatement of the plan and the
builders of expected buffers shared by tests/test_window_list_plan.py and tests/test_gpu_window_list.py.

The expected value of a list is made of numpy slices of the expected FULL frame (tests/accum_common.py,
tests/converge_common.py): pack() concatenates the windows' pixels in list order (the PACKED layout), scatter() puts them
into a sentinel-filled full frame (IN_PLACE).  No new oracle, and nothing from the code under test.  Run as a module
(python -m tests.window_list_common OUT.npz) it renders SCATTER with each call, packed, in a process of its own and
stores the outputs: the launch-split test starts it under RT_ACCUM_MAX_PASSES and RT_WINDOW_GRID_X.
"""
import sys

import numpy as np

from ray_tracer_fragment_shader_amd import distributed

from . import window_common as wc

W, H = wc.W, wc.H                            # 19 x 11; at S = 2 a tile is 4 x 4 output pixels
IN_PLACE, PACKED = 0, 1
LAYOUTS = {"inplace": IN_PLACE, "packed": PACKED}

TILING = list(wc.TILING)                     # partitions the frame
# disjoint: an unaligned window, one touching two frame edges, one running pixel and one stopped pixel of the MAIN case
SCATTER = [(3, 2, 7, 5), (12, 6, 7, 5), wc.RUNNING_PIXEL, wc.STOPPED_PIXEL]
# all 209 one-pixel windows in a seeded shuffled order: one tile each, search depth 8, every padding lane outside
_order = np.random.default_rng(20260921).permutation(W * H)
PIXELS = [(int(k % W), int(k // W), 1, 1) for k in _order]
ROWS = distributed.window_plan(W, H, 11)
BANDS = [distributed.band_windows(W, H, 3, r, 2) for r in range(3)]   # their union partitions the frame
ONE = [(0, 0, W, H)]


def lists():
    """{name: list} of every list above (each rank's BANDS under its own name)."""
    out = {"TILING": TILING, "SCATTER": SCATTER, "PIXELS": PIXELS, "ROWS": ROWS, "ONE": ONE}
    out.update({f"BANDS{r}": b for r, b in enumerate(BANDS)})
    return out


def plan(width, height, samples, wins, layout):
    """rt_window_list_plan restated: -> (first_tile [n + 1] uint32, offset [n] int64, elements)."""
    first, off, tiles, area = [], [], 0, 0
    for x0, y0, w, h in wins:
        first.append(tiles)
        off.append(area if layout == PACKED else y0 * width + x0)
        tiles += -(-samples * w // 8) * -(-samples * h // 8)
        area += w * h
    return (np.array(first + [tiles], np.uint32), np.array(off, np.int64),
            area if layout == PACKED else width * height)


def pack(frame, wins):
    """The PACKED buffer of a full-frame array [H, W(, C)]: every window's pixels dense, one after the other."""
    frame = np.asarray(frame)
    return np.concatenate([wc.crop(frame, w).reshape((w[2] * w[3],) + frame.shape[2:]) for w in wins])


def scatter(frame, wins, sentinel):
    """The IN_PLACE buffer: the windows' pixels of `frame` in a full frame that holds `sentinel` everywhere else."""
    frame = np.asarray(frame)
    out = np.full(frame.shape, sentinel, frame.dtype)
    for x0, y0, w, h in wins:
        out[y0:y0 + h, x0:x0 + w] = frame[y0:y0 + h, x0:x0 + w]
    return out


def mask(wins, width=W, height=H):
    """[H, W] bool: the pixels of the list."""
    m = np.zeros((height, width), bool)
    for x0, y0, w, h in wins:
        m[y0:y0 + h, x0:x0 + w] = True
    return m


def _child(out_path):
    """SCATTER, packed, by one accumulating and one converging list call of the MAIN case in a context created in this
    process."""
    import torch

    from ray_tracer_fragment_shader_amd.tracer import Tracer

    from . import converge_common as cc
    from . import motion_common as mc
    from . import shutter_common as hc
    from . import ssaa_common as sc

    S, J, E, K = 2, 4, 1.0 / 32.0, 16
    e = cc.expected("c2", "crane", W, H, S, J, 1, 1, 2, 0.0, wc.A, wc.R, wc.F, mc.MOVES["c2"])
    scene, depth = sc.scene_of("c2")
    t = Tracer(0)
    t.set_scene(scene)
    t.set_motion(e["d"])
    t.set_windows(W, H, SCATTER, "packed")
    m = hc.motion_abi(e["motion"])
    flags = dict(rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    out = {}
    bufs, acc = t.render_accum_windows(e["cam"], m, W, H, depth, S, J, 1, 0, wc.ACCUM_K, wc.A, wc.R, wc.F, **flags)
    torch.cuda.synchronize()
    out.update({"a_" + k: v.cpu().numpy() for k, v in bufs.items()}, a_accum=acc.cpu().numpy())
    bufs, state, active = t.render_converge_windows(e["cam"], m, W, H, depth, S, J, 1, K, wc.M, E, wc.A, wc.R, wc.F,
                                                    **flags)
    torch.cuda.synchronize()
    out.update({"c_" + k: v.cpu().numpy() for k, v in bufs.items()}, c_accum=state[0].cpu().numpy(),
               c_accum2=state[1].cpu().numpy(), c_count=state[2].cpu().numpy(), c_active=active.cpu().numpy())
    t.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    _child(sys.argv[1])
