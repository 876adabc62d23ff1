#!/usr/bin/env python3
"""What summing the samples in the render kernel buys: supersampled c2 frames (1920 x 1080 output, depth 1, static
view) at S = 2 and S = 4 samples per axis, three legs timed in one process, alternating in blocks:

  fused    rt_render_ss_dev writing RGBA32F + RGBA8 (the S x S samples summed in the wave, one store per pixel)
  unfused  rt_render_dev of the sample-grid camera at S W x S H into rgb64f, then the same pairwise tree with torch
           ops and the conversion to the same two images (S^2 times the pixels to HBM and a second pass over them)
  plain    the one-sample c2 frame (RGBA32F + RGBA8), for scale
  trace    rt_render_dev of the sample-grid camera with only rgba8 requested: the trace of the sample frame with
           almost no stores (fused / trace shows what the epilogue costs)

Before timing, fused and unfused must give identical bytes.  Every leg has its own context and is warmed through
its first, calibration and cached renders; a timed block is a few milliseconds of GPU work between two events.
Writes one JSON document (default profiles/ssaa/bench_ssaa.json) and prints it.

  python tools/bench_ssaa.py [--rounds 7] [--block-ms 20] [--out FILE]
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

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402
from tools.sampled_bench import block_ms  # noqa: E402


def camera_ss(cam, S):
    import ctypes
    out = abi.rt_camera()
    abi.check(abi.lib().rt_camera_supersample(ctypes.byref(cam), S, ctypes.byref(out)), "rt_camera_supersample")
    return out


class Unfused:
    """rt_render_dev of the sample frame into rgb64f + the reduction and conversions as torch ops."""

    def __init__(self, scene, cam_s, W, H, depth, S):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.cam_s, self.W, self.H, self.depth, self.S = cam_s, W, H, depth, S
        self.bufs = self.tr.alloc(S * W, S * H, rgba32f=False, rgb64f=True)
        dev = self.bufs["rgb64f"].device
        self.rgba32f = torch.ones((H, W, 4), dtype=torch.float32, device=dev)
        self.rgba8 = torch.full((H, W, 4), 255, dtype=torch.uint8, device=dev)

    def frame(self):
        S = self.S
        self.tr.render_into(self.cam_s, S * self.W, S * self.H, self.depth, self.bufs)
        v = self.bufs["rgb64f"].view(self.H, S, self.W, S, 3)
        n = S
        while n > 1:                                    # along a: v[a] <- v[2a] + v[2a + 1]
            v = v[:, :, :, 0::2] + v[:, :, :, 1::2]
            n //= 2
        v = v[:, :, :, 0]
        n = S
        while n > 1:                                    # then along b
            v = v[:, 0::2] + v[:, 1::2]
            n //= 2
        out = v[:, 0] * (1.0 / (S * S))
        self.rgba32f[..., :3] = out                     # (the copy converts to float32)
        self.rgba8[..., :3] = torch.floor(torch.clamp(out, 0.0, 1.0) * 255.0 + 0.5)


class Direct:
    """One render call per frame into fixed buffers: fused (samples = S), plain or trace-only (samples = 0)."""

    def __init__(self, scene, cam, W, H, depth, samples=0, rgba32f=True):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.args = (cam, W, H, depth)
        self.samples = samples
        self.bufs = self.tr.alloc(W, H, rgba32f=rgba32f, rgba8=True)

    def frame(self):
        if self.samples:
            self.tr.render_ss_into(*self.args, self.samples, self.bufs)
        else:
            self.tr.render_into(*self.args, self.bufs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=20.0, help="GPU work per timed block")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssaa", "bench_ssaa.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_ssaa: needs a HIP GPU")
    cfg = scenes.CONFIGS["c2"]
    W, H, depth = cfg.width, cfg.height, cfg.depth
    scene, cam = cfg.scene(), cfg.camera()
    doc = {"config": "c2", "view": "static", "width": W, "height": H, "depth": depth, "rounds": a.rounds,
           "unit": "ms per frame (device events around a block of frames)", "device": torch.cuda.get_device_name(0),
           "cases": []}
    for S in (2, 4):
        cam_s = camera_ss(cam, S)
        legs = {"fused": Direct(scene, cam, W, H, depth, samples=S),
                "unfused": Unfused(scene, cam_s, W, H, depth, S),
                "plain": Direct(scene, cam, W, H, depth),
                "trace": Direct(scene, cam_s, S * W, S * H, depth, rgba32f=False)}
        for leg in legs.values():                       # first, calibration and cached renders
            for _ in range(4):
                leg.frame()
        torch.cuda.synchronize()
        fu, un = legs["fused"], legs["unfused"]
        same = torch.equal(fu.bufs["rgba8"], un.rgba8) and \
            torch.equal(fu.bufs["rgba32f"].view(torch.int32), un.rgba32f.view(torch.int32))
        if not same:
            sys.exit(f"bench_ssaa: S={S}: the fused and unfused frames differ")
        n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 3), 1e-3))) for k, leg in legs.items()}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, leg in legs.items():
                times[k].append(block_ms(leg, n[k]))
        case = {"samples": S, "identical_bytes": True, "frames_per_block": n, "legs": {}}
        for k, v in times.items():
            case["legs"][k] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                               "max_ms": round(max(v), 5)}
        f, u, t = case["legs"]["fused"], case["legs"]["unfused"], case["legs"]["trace"]
        case["unfused_over_fused"] = round(u["median_ms"] / f["median_ms"], 4)
        case["fused_over_trace"] = round(f["median_ms"] / t["median_ms"], 4)
        case["fused_faster_than_unfused_by_more_than_its_spread"] = \
            bool(u["median_ms"] - f["median_ms"] > f["max_ms"] - f["min_ms"])
        doc["cases"].append(case)
        for leg in legs.values():
            leg.tr.close()
        del legs, fu, un
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
