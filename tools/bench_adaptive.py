#!/usr/bin/env python3
"""What refining only the high-contrast pixels buys: c2 frames (1920 x 1080 output, depth 1, static view) at S = 2
and S = 4 samples per axis and threshold T = 8, three legs timed in one process, alternating in blocks:

  adaptive  rt_render_adaptive_dev writing RGBA32F + RGBA8 (+ refined): the base render, the classification and
            compaction pass, the refine pass over the work list
  full      rt_render_ss_dev of the same S writing RGBA32F + RGBA8 (S x S samples for every pixel)
  plain     the one-sample c2 frame (RGBA32F + RGBA8)

Before timing, the adaptive frame must equal, byte for byte, the cross-route `full where refined else plain` (no
oracle involved).  Every leg has its own context and is warmed through its first, calibration and cached renders;
a timed block is a few milliseconds of GPU work between two events.  Reports median (min - max) per frame, the
refined share and the ratio of the adaptive frame to the model plain + share x full.
Writes one JSON document (default profiles/adaptive/bench_adaptive.json) and prints it.

  python tools/bench_adaptive.py [--rounds 7] [--block-ms 20] [--threshold 8] [--frames N] [--out FILE]

--frames N (> 0) only runs N adaptive frames per S after the warm-up and writes nothing: the workload for a kernel
trace (rocprofv3 --kernel-trace --stats -- python tools/bench_adaptive.py --frames 20).
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402
from tools.sampled_bench import block_ms  # noqa: E402


class Leg:
    """One render call per frame into fixed buffers: adaptive (threshold given), full (samples > 0) or plain."""

    def __init__(self, scene, cam, W, H, depth, samples=0, threshold=None):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.args = (cam, W, H, depth)
        self.samples, self.threshold = samples, threshold
        if threshold is not None:
            self.bufs = self.tr.alloc_adaptive(W, H, samples, rgba32f=True, rgba8=True)
        else:
            self.bufs = self.tr.alloc(W, H, rgba32f=True, rgba8=True)

    def frame(self):
        if self.threshold is not None:
            self.tr.render_adaptive_into(*self.args, self.samples, self.threshold, self.bufs)
        elif self.samples:
            self.tr.render_ss_into(*self.args, self.samples, self.bufs)
        else:
            self.tr.render_into(*self.args, self.bufs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=20.0, help="GPU work per timed block")
    ap.add_argument("--threshold", type=int, default=8)
    ap.add_argument("--frames", type=int, default=0, help="> 0: only this many adaptive frames per S (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "bench_adaptive.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_adaptive: needs a HIP GPU")
    cfg = scenes.CONFIGS["c2"]
    W, H, depth = cfg.width, cfg.height, cfg.depth
    scene, cam = cfg.scene(), cfg.camera()
    doc = {"config": "c2", "view": "static", "width": W, "height": H, "depth": depth, "threshold": a.threshold,
           "rounds": a.rounds, "unit": "ms per frame (device events around a block of frames)",
           "device": torch.cuda.get_device_name(0), "cases": []}
    for S in (2, 4):
        legs = {"adaptive": Leg(scene, cam, W, H, depth, samples=S, threshold=a.threshold),
                "full": Leg(scene, cam, W, H, depth, samples=S),
                "plain": Leg(scene, cam, W, H, depth)}
        for leg in legs.values():                       # first, calibration and cached renders
            for _ in range(4):
                leg.frame()
        torch.cuda.synchronize()
        ad, fu, pl = legs["adaptive"], legs["full"], legs["plain"]
        ref = ad.bufs["refined"].bool().unsqueeze(-1)
        same = torch.equal(ad.bufs["rgba8"], torch.where(ref, fu.bufs["rgba8"], pl.bufs["rgba8"])) and \
            torch.equal(ad.bufs["rgba32f"].view(torch.int32),
                        torch.where(ref, fu.bufs["rgba32f"].view(torch.int32), pl.bufs["rgba32f"].view(torch.int32)))
        if not same:
            sys.exit(f"bench_adaptive: S={S}: the adaptive frame differs from `full where refined else plain`")
        n_ref = int(ad.bufs["refined"].sum(dtype=torch.int64))
        listed = int(ad.bufs["workspace"][:4].cpu().numpy().view("uint32")[0])
        if listed != n_ref:
            sys.exit(f"bench_adaptive: S={S}: the work list holds {listed} pixels, `refined` {n_ref}")
        share = n_ref / (W * H)
        if a.frames > 0:
            for _ in range(a.frames):
                ad.frame()
            torch.cuda.synchronize()
            print(f"bench_adaptive: S={S}: {a.frames} adaptive frames, refined share {share:.4f}")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 3), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            case = {"samples": S, "identical_bytes_to_cross_route": True, "refined_pixels": n_ref,
                    "refined_share": round(share, 5), "frames_per_block": n, "legs": {}}
            for k, v in times.items():
                case["legs"][k] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                                   "max_ms": round(max(v), 5)}
            A, F, P = case["legs"]["adaptive"], case["legs"]["full"], case["legs"]["plain"]
            model = P["median_ms"] + share * F["median_ms"]
            case["model_ms_plain_plus_share_times_full"] = round(model, 5)
            case["adaptive_over_model"] = round(A["median_ms"] / model, 4)
            case["full_over_adaptive"] = round(F["median_ms"] / A["median_ms"], 4)
            case["adaptive_over_plain"] = round(A["median_ms"] / P["median_ms"], 4)
            spread = (A["max_ms"] - A["min_ms"]) + (F["max_ms"] - F["min_ms"])
            case["adaptive_faster_than_full_by_more_than_both_spreads"] = bool(F["median_ms"] - A["median_ms"] > spread)
            doc["cases"].append(case)
        for leg in legs.values():
            leg.tr.close()
        del legs, ad, fu, pl
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
