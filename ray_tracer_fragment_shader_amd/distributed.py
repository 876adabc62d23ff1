"""Image-space data parallelism across the GPUs of one node.

One process per GPU.  A frame's rows are cut into bands of `band_height` rows dealt round-robin to the
ranks (rt_rows); contiguous stripes would be badly imbalanced (sky rows are cheap, board rows are not).
The scene (< 40 KB) is built on every rank from the same descriptor, so the only data-path collective is
the exchange of finished rows, over RCCL (torch.distributed "nccl" backend = RCCL over xGMI):

* frame streams (weak scaling, the bench default): each step renders N frames, one per rank as its
  display; every frame is banded over all N ranks, each rank renders its bands of all N frames in ONE
  launch (rt_rows.frames = N, frame-major), and one all-to-all sends frame f's rows to rank f, which puts
  them in image order with rt_unshuffle_dev.  Link traffic is balanced: every rank sends and receives
  (N-1)/N of one frame per step.
* one frame split N ways (strong scaling, the c4 design): bands of a single frame, gathered to rank 0.

The reference has no distribution at all (single thread).
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.distributed as dist

from . import abi, scenes


def auto_band_height(height: int, world: int, preferred: int = 8, equal_rows: bool = False) -> int:
    """The render's tile height, 8 rows (rt_band_plan's choice: tile-aligned bands keep the per-wave cone culling;
    ranks differ by at most one band); with `equal_rows` (frame streams: the all-to-all needs every rank's rows equal)
    the largest band height <= 16 that gives every rank the same number of rows per frame, falling back to
    `preferred` (e.g. 15 rows for 1080 rows over 8 ranks)."""
    if not equal_rows:
        return 8
    for hb in range(16, 0, -1):
        if height % (hb * world) == 0:
            return hb
    return preferred


class BandPlan:
    """Row-band partition of `frames` stacked height-row frames over `world` ranks.  equal_rows (default: frames > 1,
    the frame streams' all-to-all) asks the automatic band height for the same rows on every rank."""

    def __init__(self, height: int, world: int, band_height: Optional[int] = None, frames: int = 1,
                 equal_rows: Optional[bool] = None):
        self.height = height
        self.world = world
        self.frames = frames
        eq = frames > 1 if equal_rows is None else equal_rows
        self.band_height = band_height or auto_band_height(height, world, equal_rows=eq)
        self.frame_local = [scenes.local_rows(height, self.rows(r, 1)) for r in range(world)]
        self.local = [n * frames for n in self.frame_local]
        self.slab_rows = max(self.frame_local) if world > 0 else 0     # rows per frame, padded
        self.balanced = len(set(self.frame_local)) == 1

    def rows(self, rank: int, frames: Optional[int] = None) -> abi.rt_rows:
        return scenes.rows(self.band_height, self.world, rank, self.frames if frames is None else frames)


def window_plan(width: int, height: int, parts: int) -> List[tuple]:
    """The frame as `parts` windows (x0, y0, w, h) for Tracer.render_accum_window_into / render_converge_window_into:
    horizontal strips of whole rows, bottom to top, whose heights differ by at most one (the taller ones first) — the
    contiguous split a rank per GPU, or a tile loop over a frame whose state does not fit at once, would use.  The
    strips partition the frame exactly; a window's bytes do not depend on the split.  More parts than rows give one
    strip per row (never an empty window).  A pure function: moving the strips between processes is the caller's."""
    if width < 1 or height < 1 or parts < 1:
        raise ValueError("width, height and parts must be at least 1")
    n = min(parts, height)
    base, extra = divmod(height, n)
    plan, y = [], 0
    for k in range(n):
        h = base + (1 if k < extra else 0)
        plan.append((0, y, width, h))
        y += h
    return plan


def band_windows(width: int, height: int, n_ranks: int, rank: int, band_height: int) -> List[tuple]:
    """The windows (0, y, width, h) of `rank` in a round-robin band split, in ascending y, for Tracer.set_windows: the
    frame is cut into bands of `band_height` rows, bottom to top (the last one may be shorter), and band b goes to rank
    b mod n_ranks — the split that balances where contiguous strips (window_plan) do not, and which one list call
    renders in one launch per launch group.  A rank with no band gets an empty list (set no list of it).  The ranks'
    lists partition the frame.

    This is the row ownership of the plain render's multi-GPU path: with rt_rows {band_height, n_ranks, rank}
    rt_global_row maps a rank's local row lr to image row ((lr // hb) * n_ranks + rank) * hb + lr % hb, i.e. to the
    rows of exactly these windows, in this order.  rt_band_plan (csrc/rt_host.cpp; rt_group_plan.cpp's rt_group_plan_frame
    calls it) chooses that path's band height — 8, the tile height, when asked for 0 — and the rows of the largest
    slab; it leaves what it is given above 0 unchanged, so band_windows(..., band_height=hb) with the hb it returns is
    the same split.  band_windows has no default height and calls nothing: a pure function."""
    if width < 1 or height < 1 or n_ranks < 1 or band_height < 1:
        raise ValueError("width, height, n_ranks and band_height must be at least 1")
    if rank < 0 or rank >= n_ranks:
        raise ValueError("rank must lie in 0 .. n_ranks - 1")
    return [(0, y, width, min(band_height, height - y))
            for y in range(rank * band_height, height, n_ranks * band_height)]


def _host_staged(group=None) -> bool:
    """gloo over device tensors: the rehearsal of the RCCL path on one GPU (bench.py --backend gloo) stages
    the exchange through host memory; RCCL moves device memory directly."""
    return dist.get_backend(group) == "gloo"


def gather_slabs(slab: torch.Tensor, world: int, root: int = 0, group=None) -> Optional[List[torch.Tensor]]:
    """Gather every rank's padded slab to `root` (one collective).  Returns the list on root, None elsewhere."""
    if world == 1:
        return [slab]
    rank = dist.get_rank(group)
    if slab.is_cuda and _host_staged(group):
        h = slab.cpu()
        hb = [torch.empty_like(h) for _ in range(world)] if rank == root else None
        dist.gather(h, gather_list=hb, dst=root, group=group)
        return [b.to(slab.device) for b in hb] if rank == root else None
    bufs = [torch.empty_like(slab) for _ in range(world)] if rank == root else None
    dist.gather(slab, gather_list=bufs, dst=root, group=group)
    return bufs


def exchange_frames(local: torch.Tensor, recv: torch.Tensor, world: int, async_op: bool = False, group=None):
    """Frame streams: `local` = [world frames, rows, ...] of this rank's bands (frame-major, equal rows per
    frame); after the all-to-all `recv` = [world ranks, rows, ...] holds every rank's bands of the frame this
    rank displays."""
    if world == 1:
        recv.copy_(local)
        return None
    if local.is_cuda and _host_staged(group):
        h = torch.empty(recv.shape, dtype=recv.dtype)
        dist.all_to_all_single(h, local.cpu(), group=group)
        recv.copy_(h)
        return None
    return dist.all_to_all_single(recv, local, group=group, async_op=async_op)


def assemble_on_device(slabs: torch.Tensor, plan: BandPlan, width: int, out: torch.Tensor, stream=None):
    """[world, slab_rows, W, C] (one frame's bands from every rank) -> [H, W, C] (rt_unshuffle_dev)."""
    from .tracer import unshuffle
    return unshuffle(slabs, out, width, plan.height, plan.band_height, plan.world, plan.slab_rows, stream)


def assemble_on_host(slabs, plan: BandPlan):
    """One frame from every rank's bands, on the host through the C ABI's row map (rt_global_row): used
    where no GPU is present (gloo rehearsal) and to cross-check rt_unshuffle_dev."""
    import ctypes
    import numpy as np
    L = abi.lib()
    first = np.asarray(slabs[0])
    out = np.zeros((plan.height,) + first.shape[1:], first.dtype)
    g = ctypes.c_int()
    for r in range(plan.world):
        rr = plan.rows(r, 1)
        s = np.asarray(slabs[r])
        for lr in range(plan.frame_local[r]):
            abi.check(L.rt_global_row(plan.height, ctypes.byref(rr), lr, ctypes.byref(g)), "rt_global_row")
            out[g.value] = s[lr]
    return out
