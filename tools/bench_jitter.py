#!/usr/bin/env python3
"""What jitter costs: c2 frames (1920 x 1080 output, depth 1, static view) at S = 2 and S = 4 samples per axis, square
light panels of half-width R = 40, the sphere on c4 moving by |d| = 40 along x, shutter F = 1, pinhole (A = 0); the legs
are timed in one process, alternating in blocks:

  motion     rt_render_motion_dev writing RGBA32F + RGBA8: the regular grid, light point and time shared by the lanes
             of equal (a, b)
  jitter_1   rt_render_jitter_dev with J = 1: the same frame through rt_jitter_kernel (the hash and the level shifts run,
             every level is 0)
  jitter_16  rt_render_jitter_dev with J = 16: every lane its own sub-pixel, lens, light and time position

Before timing, the jitter_1 frame must equal the motion frame byte for byte, the jitter_16 frame must differ from it,
and a second jitter_16 frame must equal the first.  Every leg has its own context and is warmed through four frames; a
timed block is at least --block-ms of GPU work between two events.  Reports median (min - max) per frame and the ratio
of each jitter leg to the motion leg; a leg is called slower or faster only where the gap exceeds the two legs' spreads
added.  Writes one JSON document (default profiles/jitter/bench_jitter.json) and prints it.

  python tools/bench_jitter.py [--rounds 7] [--block-ms 20] [--move 40] [--light-size 40] [--seed 1] [--frames N]
                               [--out FILE]

--frames N (> 0) only runs N frames of each leg per S after the warm-up and writes nothing: the workload for a kernel
trace (rocprofv3 --kernel-trace --stats -- python tools/bench_jitter.py --frames 20).
"""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402
from tools.sampled_bench import block_ms, parse_args, same_bytes  # noqa: E402

MOVER = 4                                      # c2's sphere on c4


class Leg:
    """One frame per call into fixed buffers: rt_render_motion_dev (jitter 0) or rt_render_jitter_dev."""

    def __init__(self, scene, cam, W, H, depth, S, R, F, disp, jitter, seed):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.tr.set_motion(disp)
        self.args, self.S, self.R, self.F, self.jitter, self.seed = (cam, W, H, depth), S, R, F, jitter, seed
        self.bufs = self.tr.alloc(W, H, rgba32f=True, rgba8=True)

    def frame(self):
        if self.jitter:
            self.tr.render_jitter_into(*self.args, self.S, self.jitter, self.seed, 0.0, self.R, self.F, self.bufs)
        else:
            self.tr.render_motion_into(*self.args, self.S, 0.0, self.R, self.F, self.bufs)

    def close(self):
        self.tr.close()


def main():
    def options(ap):
        ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
        ap.add_argument("--light-size", type=float, default=40.0)
        ap.add_argument("--shutter", type=float, default=1.0)
        ap.add_argument("--seed", type=int, default=1)

    a = parse_args("bench_jitter", __doc__, options)
    cfg = scenes.CONFIGS["c2"]
    disp = [[0.0, 0.0, 0.0] for _ in cfg.scene().spheres]
    disp[MOVER][0] = a.move
    doc = {"config": "c2", "view": "static", "width": cfg.width, "height": cfg.height, "depth": cfg.depth,
           "moving_sphere": MOVER, "displacement": disp[MOVER], "shutter": a.shutter, "light_size": a.light_size,
           "aperture": 0.0, "seed": a.seed, "rounds": a.rounds,
           "unit": "ms per frame (device events around a block of frames)", "device": torch.cuda.get_device_name(0),
           "cases": []}
    for S in (2, 4):
        view = (cfg.camera(), cfg.width, cfg.height, cfg.depth)
        legs = {k: Leg(cfg.scene(), *view, S, a.light_size, a.shutter, disp, J, a.seed)
                for k, J in (("motion", 0), ("jitter_1", 1), ("jitter_16", 16))}
        for leg in legs.values():
            for _ in range(4):
                leg.frame()
        torch.cuda.synchronize()
        if not same_bytes(legs["motion"], legs["jitter_1"]):
            sys.exit(f"bench_jitter: S={S}: the J = 1 frame differs from the motion frame")
        first = {k: v.clone() for k, v in legs["jitter_16"].bufs.items() if v is not None}
        legs["jitter_16"].frame()
        torch.cuda.synchronize()
        if not all(torch.equal(first[k].view(torch.uint8), legs["jitter_16"].bufs[k].view(torch.uint8)) for k in first):
            sys.exit(f"bench_jitter: S={S}: two J = 16 frames of equal arguments differ")
        changed = float((legs["jitter_16"].bufs["rgba8"] != legs["motion"].bufs["rgba8"]).any(dim=2).double().mean())
        if changed == 0.0:
            sys.exit(f"bench_jitter: S={S}: the J = 16 frame equals the motion frame")
        if a.frames > 0:
            for leg in legs.values():
                for _ in range(a.frames):
                    leg.frame()
            torch.cuda.synchronize()
            print(f"bench_jitter: S={S}: {a.frames} frames of each leg")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 3), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            case = {"samples": S, "identical_bytes_motion_and_jitter_1": True,
                    "rgba8_pixels_changed_by_jitter_16": round(changed, 5), "frames_per_block": n, "legs": {}}
            for k, v in times.items():
                case["legs"][k] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                                   "max_ms": round(max(v), 5)}
            M = case["legs"]["motion"]
            case["motion_spread_over_median"] = round((M["max_ms"] - M["min_ms"]) / M["median_ms"], 4)
            for k in ("jitter_1", "jitter_16"):
                X = case["legs"][k]
                case[f"{k}_over_motion"] = round(X["median_ms"] / M["median_ms"], 4)
                spread = (X["max_ms"] - X["min_ms"]) + (M["max_ms"] - M["min_ms"])
                gap = X["median_ms"] - M["median_ms"]
                case[f"{k}_vs_motion"] = "slower" if gap > spread else "faster" if -gap > spread else "no difference"
            doc["cases"].append(case)
        for leg in legs.values():
            leg.close()
        del legs, first
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
