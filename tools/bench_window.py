#!/usr/bin/env python3
"""What a window costs: bench_accum.py's c2 frames (1920 x 1080 output, depth 1), square light panels of half-width
R = 40, the sphere on c4 moving by |d| = 40 along x, shutter F = 1, pinhole (A = 0), the eye moving by |move| = 40 along
y, J = 16 sub-positions; per S in {1, 2} two calls — accum: rt_render_accum_dev (0, 16); converge: rt_render_converge_dev
with K = 64, M = 4, E = 1 / 255 from a zeroed count (the zeroing is part of the leg) — each writing RGBA32F + RGBA8, and
per call these legs, timed in one process, alternating in blocks:

  full        the un-windowed call
  whole       the window call with the window (0, 0, width, height), in place: the price of the window arithmetic and of
              the five more kernel arguments
  strips2, strips4, strips8
              the frame as distributed.window_plan(width, height, parts) strips, one window call per strip into the same
              full-frame buffers: the per-launch ramp and drain tiling costs, the number a split over GPUs has to beat
  grid4x4     the frame as 4 x 4 tiles of 480 x 270 pixels, likewise
  aligned     one 960 x 540 window at (8, 8), on the tile grid at S = 1 and S = 2, dense buffers
  unaligned   one 960 x 540 window at (3, 5), dense buffers: rows and columns that start off the tile grid

Before timing, every full-frame leg's sums (for converge also the sums of squares and counts), both images and the
active count must be the `full` leg's bytes, and the two 960 x 540 legs' must be the bytes of their rectangle of it.
Every leg has its own context and is warmed through two calls; a timed block is at least --block-ms of GPU work between
two events.  Reports median (min - max) per frame of the leg; a leg is called slower or faster than another only where
the gap exceeds the two legs' spreads added.  Writes one JSON document (default profiles/window/bench_window.json) and
prints it.

  python tools/bench_window.py [--rounds 7] [--block-ms 20] [--seed 1] [--frames N [--legs full,whole]] [--case N]
                               [--out FILE]

--frames N (> 0) only runs N frames of each leg of --legs per case after the warm-up and writes nothing: the workload
for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_window.py --frames 5 --case 3).
"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.distributed import window_plan  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402
from tools.bench_accum import J, MOVER, stats, verdict  # noqa: E402
from tools.sampled_bench import block_ms, parse_args  # noqa: E402

M, E = 4, 1.0 / 255.0
PASSES = {"accum": 16, "converge": 64}
SUB_W, SUB_H = 960, 540
ALIGNED, UNALIGNED = (8, 8, SUB_W, SUB_H), (3, 5, SUB_W, SUB_H)


def grid_plan(width, height, nx, ny):
    xs = [width * k // nx for k in range(nx + 1)]
    ys = [height * k // ny for k in range(ny + 1)]
    return [(xs[i], ys[j], xs[i + 1] - xs[i], ys[j + 1] - ys[j]) for j in range(ny) for i in range(nx)]


class Leg:
    """One frame of the call `kind` per frame(): the un-windowed call (windows None) or one window call per window of
    `windows` into buffers of the frame's size (dense False) or of the one window's own size (dense True)."""

    def __init__(self, kind, windows, dense, scene, cam, W, H, depth, S, R, F, disp, seed, camera):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.tr.set_motion(disp)
        self.kind, self.windows, self.seed, self.K = kind, windows, seed, PASSES[kind]
        self.cam, self.camera, self.frame_size, self.size, self.tail = cam, camera, (W, H), (depth, S, J), (0.0, R, F)
        bw, bh = (windows[0][2], windows[0][3]) if dense else (W, H)
        self.bufs = self.tr.alloc(bw, bh, rgba32f=True, rgba8=True)
        self.state = self.tr.alloc_converge(bw, bh)
        self.active = torch.zeros((1,), dtype=torch.int32, device=self.state[0].device)
        self.active_sum = 0

    def frame(self, count_active=False):
        t, acc = self.tr, self.state[0]
        if self.kind == "converge":
            self.state[2].zero_()
        self.active_sum = 0
        if self.windows is None:
            if self.kind == "accum":
                t.render_accum_into(self.cam, self.camera, *self.frame_size, *self.size, self.seed, 0, self.K, *self.tail,
                                    acc, self.bufs)
            else:
                t.render_converge_into(self.cam, self.camera, *self.frame_size, *self.size, self.seed, self.K, M, E,
                                       *self.tail, self.state, self.bufs, self.active)
            if count_active:
                self.active_sum = int(self.active[0])
            return
        for win in self.windows:
            if self.kind == "accum":
                t.render_accum_window_into(self.cam, self.camera, *self.frame_size, win, *self.size, self.seed, 0, self.K,
                                           *self.tail, acc, self.bufs)
            else:
                t.render_converge_window_into(self.cam, self.camera, *self.frame_size, win, *self.size, self.seed, self.K,
                                              M, E, *self.tail, self.state, self.bufs, self.active)
                if count_active:
                    self.active_sum += int(self.active[0])

    def tensors(self):
        """What must agree between legs, by name."""
        out = {"accum": self.state[0], "rgba32f": self.bufs["rgba32f"], "rgba8": self.bufs["rgba8"]}
        if self.kind == "converge":
            out["accum2"], out["count"] = self.state[1], self.state[2]
        return out

    def close(self):
        self.tr.close()


def same(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def main():
    def options(ap):
        ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
        ap.add_argument("--eye-move", type=float, default=40.0, help="|move| of the eye, along y")
        ap.add_argument("--light-size", type=float, default=40.0)
        ap.add_argument("--shutter", type=float, default=1.0)
        ap.add_argument("--seed", type=int, default=1)
        ap.add_argument("--case", type=int, default=-1, help="only case N of the four (S, call) cases (for a kernel trace)")
        ap.add_argument("--legs", default="full,whole", help="the legs --frames runs, in this order")

    a = parse_args("bench_window", __doc__, options)
    cfg = scenes.CONFIGS["c2"]
    disp = [[0.0, 0.0, 0.0] for _ in cfg.scene().spheres]
    disp[MOVER][0] = a.move
    eye_move = [0.0, a.eye_move, 0.0]
    W, H = cfg.width, cfg.height
    plans = {"full": (None, False), "whole": ([(0, 0, W, H)], False),
             "strips2": (window_plan(W, H, 2), False), "strips4": (window_plan(W, H, 4), False),
             "strips8": (window_plan(W, H, 8), False), "grid4x4": (grid_plan(W, H, 4, 4), False),
             "aligned": ([ALIGNED], True), "unaligned": ([UNALIGNED], True)}
    doc = {"config": "c2", "view": "static", "width": W, "height": H, "depth": cfg.depth, "moving_sphere": MOVER,
           "displacement": disp[MOVER], "eye_move": eye_move, "look_at_move": [0.0, 0.0, 0.0], "shutter": a.shutter,
           "light_size": a.light_size, "aperture": 0.0, "jitter": J, "seed": a.seed, "passes": PASSES, "min_passes": M,
           "tolerance": E, "windows": {k: v[0] for k, v in plans.items()}, "rounds": a.rounds,
           "unit": "ms per frame of the leg (device events around a block of frames)",
           "device": torch.cuda.get_device_name(0), "not_measured": "other scenes, depths and motions", "cases": []}
    if a.frames > 0:                                        # a trace holds the kernels of the legs asked for alone
        plans = {k: v for k, v in plans.items() if k == "full" or k in a.legs.split(",")}
    cases = [(S, kind) for S in (1, 2) for kind in ("accum", "converge")]
    for S, kind in cases if a.case < 0 else cases[a.case:a.case + 1]:
        view = (cfg.camera(), W, H, cfg.depth)
        legs = {k: Leg(kind, wins, dense, cfg.scene(), *view, S, a.light_size, a.shutter, disp, a.seed,
                       scenes.camera_motion(eye=eye_move)) for k, (wins, dense) in plans.items()}
        for leg in legs.values():
            leg.frame()
            leg.frame(count_active=True)
        torch.cuda.synchronize()
        full, active_full = legs["full"].tensors(), legs["full"].active_sum
        for k, leg in legs.items():
            for name, t in leg.tensors().items():
                if plans[k][1]:
                    x0, y0, w, h = plans[k][0][0]
                    want = full[name][y0:y0 + h, x0:x0 + w]
                else:
                    want = full[name]
                if not same(t, want):
                    sys.exit(f"bench_window: S={S} {kind}: {name} of the leg {k} differs from the un-windowed call's")
            if kind == "converge":
                if plans[k][1]:
                    x0, y0, w, h = plans[k][0][0]
                    # (the un-windowed call has no count of a rectangle: the window's own second call must repeat it)
                    first = leg.active_sum
                    leg.frame(count_active=True)
                    ok = leg.active_sum == first
                else:
                    ok = leg.active_sum == active_full
                if not ok:
                    sys.exit(f"bench_window: S={S} {kind}: the active count of the leg {k} is off")
        if a.frames > 0:
            for k in a.legs.split(","):
                for _ in range(a.frames):
                    legs[k].frame()
            torch.cuda.synchronize()
            print(f"bench_window: S={S} {kind}: {a.frames} frames of each of the legs {a.legs}")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 2), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            L = {k: stats(v) for k, v in times.items()}
            case = {"samples": S, "call": kind, "identical_bytes": True, "frames_per_block": n, "legs": L,
                    "launches_per_frame": {k: (1 if wins is None else len(wins)) * math.ceil(PASSES[kind] / 4)
                                           for k, (wins, _) in plans.items()}}
            if kind == "converge":
                case["active"] = active_full
            for k in ("whole", "strips2", "strips4", "strips8", "grid4x4"):
                case[f"{k}_over_full"] = round(L[k]["median_ms"] / L["full"]["median_ms"], 4)
                case[f"{k}_vs_full"] = verdict(L[k], L["full"])
            case["unaligned_over_aligned"] = round(L["unaligned"]["median_ms"] / L["aligned"]["median_ms"], 4)
            case["unaligned_vs_aligned"] = verdict(L["unaligned"], L["aligned"])
            doc["cases"].append(case)
        for leg in legs.values():
            leg.close()
        del legs, full
        torch.cuda.empty_cache()
    if a.frames > 0:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
