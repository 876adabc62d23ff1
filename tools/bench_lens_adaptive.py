#!/usr/bin/env python3
"""What refining only the pixels whose samples disagree buys the lens family's renders: c2 frames (1920 x 1080 output,
depth 1, static view), the sphere on c4 moving by |d| = 40 along x with the shutter open for F = 1, area lights of
half-width R = 40, pinhole (A = 0), threshold T = 8; the sample pairs (2, 4) and (2, 8), and (2, 4) with the scene
frozen (F = 0: soft shadows alone).  Four legs are timed in one process, alternating in blocks:

  adaptive  rt_render_lens_adaptive_dev writing RGBA32F + RGBA8 (+ refined): the coarse render with the spread bytes,
            the classification and compaction pass, the refine pass over the work list
  full      rt_render_motion_dev at S_hi writing RGBA32F + RGBA8 (S_hi x S_hi samples for every pixel)
  coarse    rt_render_motion_dev at S_lo
  plain     the one-sample c2 frame

Before timing, the adaptive frame must equal, byte for byte, the cross-route `full where refined else coarse` (no
oracle involved).  Every leg has its own context and is warmed; a timed block is --block-ms of GPU work between two
events.  Reports median (min - max) per frame, the refined share, the ratio to the full frame and the ratio of the
adaptive frame to the model coarse + share x full.
Writes one JSON document (default profiles/lens_adaptive/bench_lens_adaptive.json) and prints it.

  python tools/bench_lens_adaptive.py [--rounds 7] [--block-ms 20] [--threshold 8] [--frames N] [--case K] [--out FILE]

--frames N (> 0) only runs N adaptive frames per case after the warm-up and writes nothing: the workload for a kernel
trace, one case (--case 0, 1 or 2, in the order above) per trace so that the passes' times are that case's
(rocprofv3 --kernel-trace --stats -- python tools/bench_lens_adaptive.py --frames 20 --case 0).
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
from tools.sampled_bench import Leg, block_ms  # noqa: E402

MOVER = 4                                      # c2's sphere on c4
CASES = [(2, 4, 1.0), (2, 8, 1.0), (2, 4, 0.0)]   # (S_lo, S_hi, shutter)


class AdaptiveLeg:
    """One rt_render_lens_adaptive_dev per frame into fixed buffers."""

    def __init__(self, scene, cam, W, H, depth, S_lo, S_hi, T, A, R, F, disp):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.tr.set_motion(disp)
        self.args = (cam, W, H, depth, S_lo, S_hi, T, A, R, F)
        self.bufs = self.tr.alloc_lens_adaptive(W, H, rgba32f=True, rgba8=True)

    def frame(self):
        self.tr.render_lens_adaptive_into(*self.args, self.bufs)

    def close(self):
        self.tr.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=20.0, help="GPU work per timed block")
    ap.add_argument("--threshold", type=int, default=8)
    ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
    ap.add_argument("--light-size", type=float, default=40.0)
    ap.add_argument("--frames", type=int, default=0, help="> 0: only this many adaptive frames per case (kernel traces)")
    ap.add_argument("--case", type=int, default=-1, help=">= 0: only this case (with --frames: one trace per case)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_adaptive", "bench_lens_adaptive.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_lens_adaptive: needs a HIP GPU")
    cfg = scenes.CONFIGS["c2"]
    W, H, depth = cfg.width, cfg.height, cfg.depth
    scene, cam = cfg.scene(), cfg.camera()
    T, R, A = a.threshold, a.light_size, 0.0
    disp = [[0.0, 0.0, 0.0] for _ in scene.spheres]
    disp[MOVER][0] = a.move
    doc = {"config": "c2", "view": "static", "width": W, "height": H, "depth": depth, "threshold": T,
           "moving_sphere": MOVER, "displacement": disp[MOVER], "light_size": R, "aperture": A, "rounds": a.rounds,
           "unit": "ms per frame (device events around a block of frames)", "device": torch.cuda.get_device_name(0),
           "cases": []}
    if a.case >= len(CASES):
        ap.error(f"--case must be below {len(CASES)}")
    for S_lo, S_hi, F in CASES if a.case < 0 else CASES[a.case:a.case + 1]:
        view = (cam, W, H, depth)
        legs = {"adaptive": AdaptiveLeg(scene, *view, S_lo, S_hi, T, A, R, F, disp),
                "full": Leg(scene, *view, samples=S_hi, aperture=A, light_size=R, disp=disp, shutter=F),
                "coarse": Leg(scene, *view, samples=S_lo, aperture=A, light_size=R, disp=disp, shutter=F),
                "plain": Leg(scene, *view)}
        for leg in legs.values():                       # first, calibration and cached renders
            for _ in range(4):
                leg.frame()
        torch.cuda.synchronize()
        ad, fu, co = legs["adaptive"], legs["full"], legs["coarse"]
        ref = ad.bufs["refined"].bool().unsqueeze(-1)
        same = torch.equal(ad.bufs["rgba8"], torch.where(ref, fu.bufs["rgba8"], co.bufs["rgba8"])) and \
            torch.equal(ad.bufs["rgba32f"].view(torch.int32),
                        torch.where(ref, fu.bufs["rgba32f"].view(torch.int32), co.bufs["rgba32f"].view(torch.int32)))
        what = f"({S_lo}, {S_hi}) F={F}"
        if not same:
            sys.exit(f"bench_lens_adaptive: {what}: the adaptive frame differs from `full where refined else coarse`")
        n_ref = int(ad.bufs["refined"].sum(dtype=torch.int64))
        listed = int(ad.bufs["workspace"][:4].cpu().numpy().view("uint32")[0])
        if listed != n_ref:
            sys.exit(f"bench_lens_adaptive: {what}: the work list holds {listed} pixels, `refined` {n_ref}")
        share = n_ref / (W * H)
        if a.frames > 0:
            for _ in range(a.frames):
                ad.frame()
            torch.cuda.synchronize()
            print(f"bench_lens_adaptive: {what}: {a.frames} adaptive frames, refined share {share:.4f}")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 3), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            case = {"samples_lo": S_lo, "samples_hi": S_hi, "shutter": F, "identical_bytes_to_cross_route": True,
                    "refined_pixels": n_ref, "refined_share": round(share, 5), "frames_per_block": n, "legs": {}}
            for k, v in times.items():
                case["legs"][k] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                                   "max_ms": round(max(v), 5)}
            Ad, Fu, Co = case["legs"]["adaptive"], case["legs"]["full"], case["legs"]["coarse"]
            model = Co["median_ms"] + share * Fu["median_ms"]
            case["model_ms_coarse_plus_share_times_full"] = round(model, 5)
            case["adaptive_over_model"] = round(Ad["median_ms"] / model, 4)
            case["full_over_adaptive"] = round(Fu["median_ms"] / Ad["median_ms"], 4)
            case["adaptive_over_coarse"] = round(Ad["median_ms"] / Co["median_ms"], 4)
            spread = (Ad["max_ms"] - Ad["min_ms"]) + (Fu["max_ms"] - Fu["min_ms"])
            case["adaptive_faster_than_full_by_more_than_both_spreads"] = bool(Fu["median_ms"] - Ad["median_ms"] > spread)
            doc["cases"].append(case)
        for leg in legs.values():
            leg.close()
        del legs, ad, fu, co
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
