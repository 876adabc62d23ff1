#!/usr/bin/env python3
"""What a moving camera costs: c2 frames (1920 x 1080 output, depth 1) at S = 2 and S = 4 samples per axis and J = 1 and
J = 16 sub-positions, square light panels of half-width R = 40, the sphere on c4 moving by |d| = 40 along x, shutter
F = 1, pinhole (A = 0); per (S, J) three legs are timed in one process, alternating in blocks:

  jitter     rt_render_jitter_dev writing RGBA32F + RGBA8: the frozen camera, its basis formed by the host
  frozen     rt_render_shutter_dev with a zero camera motion: the same frame through rt_shutter_kernel (every lane
             forms its camera and basis; all come out the frozen one)
  crane      rt_render_shutter_dev with the eye moving by |move| = 40 along y: every lane its own eye and basis

Before timing, the frozen frame must equal the jitter frame byte for byte, the crane frame must differ from it, and a
second crane frame must equal the first.  Every leg has its own context and is warmed through four frames; a timed
block is at least --block-ms of GPU work between two events.  Reports median (min - max) per frame, the ratio of each
shutter leg to the jitter leg and every leg's ray counts per frame; a leg is called slower or faster only where the gap
exceeds the two legs' spreads added.  Writes one JSON document (default profiles/shutter/bench_shutter.json) and prints
it.

  python tools/bench_shutter.py [--rounds 7] [--block-ms 20] [--move 40] [--eye-move 40] [--light-size 40] [--seed 1]
                                [--frames N] [--out FILE]

--frames N (> 0) only runs N frames of each leg per (S, J) after the warm-up and writes nothing: the workload for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_shutter.py --frames 20).
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
    """One frame per call into fixed buffers: rt_render_jitter_dev (camera None) or rt_render_shutter_dev."""

    def __init__(self, scene, cam, W, H, depth, S, J, R, F, disp, seed, camera):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.tr.set_motion(disp)
        self.args, self.rest, self.camera = (W, H, depth, S, J, seed, 0.0, R, F), cam, camera
        self.bufs = self.tr.alloc(W, H, rgba32f=True, rgba8=True)

    def frame(self):
        if self.camera is None:
            self.tr.render_jitter_into(self.rest, *self.args, self.bufs)
        else:
            self.tr.render_shutter_into(self.rest, self.camera, *self.args, self.bufs)

    def rays(self):
        """The primary, reflected and shadow rays of one frame, from the two-word counters."""
        W, H, depth, S = self.args[:4]
        flags = dict(rgba32f=False, raycount=True)
        bufs = (self.tr.render_jitter(self.rest, *self.args, **flags) if self.camera is None
                else self.tr.render_shutter(self.rest, self.camera, *self.args, **flags))
        torch.cuda.synchronize()
        rc = bufs["raycount"].to(torch.int64).reshape(-1, 2).sum(dim=0).tolist()
        return {"primary": W * H * S * S, "reflect": rc[0] - W * H * S * S, "shadow": rc[1]}

    def close(self):
        self.tr.close()


def main():
    def options(ap):
        ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
        ap.add_argument("--eye-move", type=float, default=40.0, help="|move| of the eye, along y")
        ap.add_argument("--light-size", type=float, default=40.0)
        ap.add_argument("--shutter", type=float, default=1.0)
        ap.add_argument("--seed", type=int, default=1)

    a = parse_args("bench_shutter", __doc__, options)
    cfg = scenes.CONFIGS["c2"]
    disp = [[0.0, 0.0, 0.0] for _ in cfg.scene().spheres]
    disp[MOVER][0] = a.move
    eye_move = [0.0, a.eye_move, 0.0]
    doc = {"config": "c2", "view": "static", "width": cfg.width, "height": cfg.height, "depth": cfg.depth,
           "moving_sphere": MOVER, "displacement": disp[MOVER], "eye_move": eye_move, "look_at_move": [0.0, 0.0, 0.0],
           "shutter": a.shutter, "light_size": a.light_size, "aperture": 0.0, "seed": a.seed, "rounds": a.rounds,
           "unit": "ms per frame (device events around a block of frames)", "device": torch.cuda.get_device_name(0),
           "not_measured": "other scenes, depths, apertures and motions", "cases": []}
    for S in (2, 4):
        for J in (1, 16):
            view = (cfg.camera(), cfg.width, cfg.height, cfg.depth)
            legs = {k: Leg(cfg.scene(), *view, S, J, a.light_size, a.shutter, disp, a.seed, cam)
                    for k, cam in (("jitter", None), ("frozen", scenes.camera_motion()),
                                   ("crane", scenes.camera_motion(eye=eye_move)))}
            for leg in legs.values():
                for _ in range(4):
                    leg.frame()
            torch.cuda.synchronize()
            if not same_bytes(legs["jitter"], legs["frozen"]):
                sys.exit(f"bench_shutter: S={S} J={J}: the zero-motion frame differs from the jittered frame")
            first = {k: v.clone() for k, v in legs["crane"].bufs.items() if v is not None}
            legs["crane"].frame()
            torch.cuda.synchronize()
            if not all(torch.equal(first[k].view(torch.uint8), legs["crane"].bufs[k].view(torch.uint8)) for k in first):
                sys.exit(f"bench_shutter: S={S} J={J}: two crane frames of equal arguments differ")
            changed = float((legs["crane"].bufs["rgba8"] != legs["jitter"].bufs["rgba8"]).any(dim=2).double().mean())
            if changed == 0.0:
                sys.exit(f"bench_shutter: S={S} J={J}: the crane frame equals the jittered frame")
            if a.frames > 0:
                for leg in legs.values():
                    for _ in range(a.frames):
                        leg.frame()
                torch.cuda.synchronize()
                print(f"bench_shutter: S={S} J={J}: {a.frames} frames of each leg")
            else:
                n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 3), 1e-3))) for k, leg in legs.items()}
                times = {k: [] for k in legs}
                for _ in range(a.rounds):
                    for k, leg in legs.items():
                        times[k].append(block_ms(leg, n[k]))
                case = {"samples": S, "jitter": J, "identical_bytes_jitter_and_frozen": True,
                        "rgba8_pixels_changed_by_crane": round(changed, 5), "frames_per_block": n,
                        "rays_per_frame": {k: leg.rays() for k, leg in legs.items()}, "legs": {}}
                for k, v in times.items():
                    case["legs"][k] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                                       "max_ms": round(max(v), 5)}
                M = case["legs"]["jitter"]
                case["jitter_spread_over_median"] = round((M["max_ms"] - M["min_ms"]) / M["median_ms"], 4)
                for k in ("frozen", "crane"):
                    X = case["legs"][k]
                    case[f"{k}_over_jitter"] = round(X["median_ms"] / M["median_ms"], 4)
                    spread = (X["max_ms"] - X["min_ms"]) + (M["max_ms"] - M["min_ms"])
                    gap = X["median_ms"] - M["median_ms"]
                    case[f"{k}_vs_jitter"] = "slower" if gap > spread else "faster" if -gap > spread else "no difference"
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
