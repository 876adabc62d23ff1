#!/usr/bin/env python3
"""What summing K jittered passes in the kernel saves: c2 frames (1920 x 1080 output, depth 1), square light panels of
half-width R = 40, the sphere on c4 moving by |d| = 40 along x, shutter F = 1, pinhole (A = 0), the eye moving by
|move| = 40 along y, J = 16 sub-positions; per (S, K) four legs are timed in one process, alternating in blocks:

  fused      one rt_render_accum_dev call of K passes from pass 0, writing RGBA32F + RGBA8 of the mean
  calls      K rt_render_accum_dev calls of one pass each on the same accumulator, every call writing both images (a
             preview that sharpens call after call)
  composed   what there was before: K rt_render_shutter_dev calls writing RGB64F, a torch FP64 accumulation per pass
             (copy for pass 0, add_ after), one division and the two conversions at the end
  shutter    one rt_render_shutter_dev frame writing RGBA32F + RGBA8: the cost of a single pass

Before timing, the three accumulators must be the same bytes, a second fused call must repeat the first, and the
K-pass mean must differ from the shutter frame.  Every leg has its own context and is warmed through three calls; a timed
block is at least --block-ms of GPU work between two events.  Reports median (min - max) per call, fused / K against
shutter, fused against composed and calls; a leg is called slower or faster only where the gap exceeds the two legs'
spreads added.  A last case, S = 4 and K = 4 (fused and shutter only), gives the per-pass time the launch split
(kAccumMaxPasses, rt_ctx.hpp) is chosen from.  Writes one JSON document (default profiles/accum/bench_accum.json) and
prints it.

  python tools/bench_accum.py [--rounds 7] [--block-ms 20] [--move 40] [--eye-move 40] [--light-size 40] [--seed 1]
                              [--frames N] [--case N] [--out FILE]

--frames N (> 0) only runs N calls of the fused and the shutter leg per case after the warm-up and writes nothing: the
workload for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_accum.py --frames 10 --case 3).
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
from tools.sampled_bench import block_ms, convert, parse_args, unfused_bufs  # noqa: E402

MOVER = 4                                      # c2's sphere on c4
J = 16


class Leg:
    """One call of the leg `kind` per frame() into fixed buffers."""

    def __init__(self, kind, scene, cam, W, H, depth, S, K, R, F, disp, seed, camera):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.tr.set_motion(disp)
        self.kind, self.K, self.seed = kind, K, seed
        self.cam, self.camera, self.size, self.tail = cam, camera, (W, H, depth, S, J), (0.0, R, F)
        dev = torch.device("cuda", 0)
        self.acc = self.tr.alloc_accum(W, H)
        if kind == "composed":
            self.pass_bufs = self.tr.alloc(W, H, rgba32f=False, rgb64f=True)
            self.bufs = unfused_bufs(W, H, dev)
            self.count = torch.tensor(float(K), dtype=torch.float64, device=dev)    # a tensor divisor: an IEEE division
        else:
            self.bufs = self.tr.alloc(W, H, rgba32f=True, rgba8=True)

    def frame(self):
        t = self.tr
        if self.kind == "fused":
            t.render_accum_into(self.cam, self.camera, *self.size, self.seed, 0, self.K, *self.tail, self.acc, self.bufs)
        elif self.kind == "calls":
            for p in range(self.K):
                t.render_accum_into(self.cam, self.camera, *self.size, self.seed, p, 1, *self.tail, self.acc, self.bufs)
        elif self.kind == "composed":
            for p in range(self.K):
                t.render_shutter_into(self.cam, self.camera, *self.size, (self.seed + p) & 0xFFFFFFFF, *self.tail,
                                      self.pass_bufs)
                if p == 0:
                    self.acc.copy_(self.pass_bufs["rgb64f"])
                else:
                    self.acc.add_(self.pass_bufs["rgb64f"])
            convert(torch.div(self.acc, self.count), self.bufs)
        else:
            t.render_shutter_into(self.cam, self.camera, *self.size, self.seed, *self.tail, self.bufs)

    def close(self):
        self.tr.close()


def stats(v):
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def verdict(x, y):
    """x against y: slower or faster only where the gap exceeds the two legs' spreads added."""
    spread = (x["max_ms"] - x["min_ms"]) + (y["max_ms"] - y["min_ms"])
    gap = x["median_ms"] - y["median_ms"]
    return "slower" if gap > spread else "faster" if -gap > spread else "no difference"


def main():
    def options(ap):
        ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
        ap.add_argument("--eye-move", type=float, default=40.0, help="|move| of the eye, along y")
        ap.add_argument("--light-size", type=float, default=40.0)
        ap.add_argument("--shutter", type=float, default=1.0)
        ap.add_argument("--seed", type=int, default=1)
        ap.add_argument("--case", type=int, default=-1, help="only case N of the five (S, K) cases (for a kernel trace)")

    a = parse_args("bench_accum", __doc__, options)
    cfg = scenes.CONFIGS["c2"]
    disp = [[0.0, 0.0, 0.0] for _ in cfg.scene().spheres]
    disp[MOVER][0] = a.move
    eye_move = [0.0, a.eye_move, 0.0]
    doc = {"config": "c2", "view": "static", "width": cfg.width, "height": cfg.height, "depth": cfg.depth,
           "moving_sphere": MOVER, "displacement": disp[MOVER], "eye_move": eye_move, "look_at_move": [0.0, 0.0, 0.0],
           "shutter": a.shutter, "light_size": a.light_size, "aperture": 0.0, "jitter": J, "seed": a.seed,
           "rounds": a.rounds, "unit": "ms per call (device events around a block of calls)",
           "device": torch.cuda.get_device_name(0), "not_measured": "other scenes, depths and motions", "cases": []}
    cases = ((1, 4, None), (1, 16, None), (2, 4, None), (2, 16, None), (4, 4, ("fused", "shutter")))
    for S, K, kinds in cases if a.case < 0 else cases[a.case:a.case + 1]:
        kinds = kinds or ("fused", "calls", "composed", "shutter")
        view = (cfg.camera(), cfg.width, cfg.height, cfg.depth)
        legs = {k: Leg(k, cfg.scene(), *view, S, K, a.light_size, a.shutter, disp, a.seed,
                       scenes.camera_motion(eye=eye_move)) for k in kinds}
        for leg in legs.values():
            for _ in range(3):
                leg.frame()
        torch.cuda.synchronize()
        fu = legs["fused"]
        for k in kinds:
            if k != "shutter" and not torch.equal(fu.acc.view(torch.int64), legs[k].acc.view(torch.int64)):
                sys.exit(f"bench_accum: S={S} K={K}: the accumulator of the leg {k} differs from the fused call's")
        same_images = {k: bool(torch.equal(fu.bufs["rgba8"], legs[k].bufs["rgba8"]) and
                               torch.equal(fu.bufs["rgba32f"].view(torch.int32), legs[k].bufs["rgba32f"].view(torch.int32)))
                       for k in kinds if k not in ("fused", "shutter")}
        first = {k: v.clone() for k, v in fu.bufs.items() if v is not None}
        first["acc"] = fu.acc.clone()
        fu.frame()
        torch.cuda.synchronize()
        now = dict(fu.bufs, acc=fu.acc)
        if not all(torch.equal(first[k].view(torch.uint8), now[k].view(torch.uint8)) for k in first):
            sys.exit(f"bench_accum: S={S} K={K}: two fused calls of equal arguments differ")
        changed = float((fu.bufs["rgba8"] != legs["shutter"].bufs["rgba8"]).any(dim=2).double().mean())
        if changed == 0.0:
            sys.exit(f"bench_accum: S={S} K={K}: the mean of {K} passes equals pass 0")
        if a.frames > 0:
            for k in ("fused", "shutter"):
                for _ in range(a.frames):
                    legs[k].frame()
            torch.cuda.synchronize()
            print(f"bench_accum: S={S} K={K}: {a.frames} calls of the fused and the shutter leg")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 3), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            L = {k: stats(v) for k, v in times.items()}
            case = {"samples": S, "passes": K, "identical_accumulators": True, "identical_images": same_images,
                    "rgba8_pixels_changed_by_the_mean": round(changed, 5), "calls_per_block": n, "legs": L,
                    "fused_per_pass_ms": round(L["fused"]["median_ms"] / K, 5),
                    "fused_per_pass_over_shutter": round(L["fused"]["median_ms"] / K / L["shutter"]["median_ms"], 4),
                    "shutter_spread_over_median": round((L["shutter"]["max_ms"] - L["shutter"]["min_ms"]) /
                                                        L["shutter"]["median_ms"], 4)}
            for other in (k for k in kinds if k in ("calls", "composed")):
                case[f"fused_over_{other}"] = round(L["fused"]["median_ms"] / L[other]["median_ms"], 4)
                case[f"fused_vs_{other}"] = verdict(L["fused"], L[other])
            doc["cases"].append(case)
        for leg in legs.values():
            leg.close()
        del legs, fu, first, now
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
