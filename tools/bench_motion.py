#!/usr/bin/env python3
"""What the motion-blur kernel costs and what fusing it buys: c2 frames (1920 x 1080 output, depth 1, static view) at
S = 2 and S = 4 samples per axis, the sphere on c4 moving by |d| = 40 along x, shutter F = 1, pinhole (A = 0), point
lights (R = 0); the legs are timed in one process, alternating in blocks:

  fused            rt_render_motion_dev writing RGBA32F + RGBA8 (one launch: rays, times and sphere centres formed,
                   traced and reduced in the kernel)
  unfused          what a caller without the kernel does: for each of the S x S samples, rt_set_scene of the scene with
                   the spheres where they are at that sample's time and rt_trace_rays_dev on that sample's W H rays
                   (lists built once with torch); then torch's pairwise tree and the two conversions
  unfused_no_upload  the same with one context per sample, its displaced scene uploaded beforehand: the S x S traces,
                   the tree and the conversions without the scene uploads
  soft             rt_render_soft_dev of the same S, A and R writing RGBA32F + RGBA8: the same rays and shadow tests in
                   the frozen scene, i.e. the price of per-lane sphere centres
  pinhole          rt_render_ss_dev of the same S (the specialised render kernels)
  plain            the one-sample c2 frame

Before timing, the fused frame and both unfused frames must be equal byte for byte (no oracle involved).  Every leg
has its own context(s) and is warmed through its first, calibration and cached renders; a timed block is at least
--block-ms of GPU work between two events.  Reports median (min - max) per frame and the ratios of the fused leg to
the others; one leg is called faster only where the gap exceeds the two legs' spreads added.
Writes one JSON document (default profiles/motion/bench_motion.json) and prints it.

  python tools/bench_motion.py [--rounds 7] [--block-ms 20] [--move 40] [--shutter 1] [--frames N] [--out FILE]

--frames N (> 0) only runs N fused and N unfused_no_upload frames per S after the warm-up and writes nothing: the
workload for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_motion.py --frames 20).
"""
import argparse
import ctypes
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
from tools.bench_dof import block_ms, lens_rays  # noqa: E402
from tools.bench_soft import same_bytes  # noqa: E402

MOVER = 4                                      # c2's sphere on c4


def displaced_scene(scene, disp, S, F, a, b):
    """The rt_scene of `scene` with every sphere where it is at the time of sample (a, b) (include/rt_api.h, motion
    blur rules 2-3), in Python floats: IEEE binary64, one operation per product and sum."""
    s = scene.to_abi()
    n = a + S * b
    sigma = F * (float(2 * n + 1 - S * S) / float(S * S))
    for k in range(s.n_spheres):
        for q in range(3):
            s.spheres[k].center[q] = s.spheres[k].center[q] + (sigma * disp[k][q])
    return s


class Leg:
    """One frame per call into fixed buffers: fused (disp given), soft (light_size given), pinhole (samples > 0) or
    plain."""

    def __init__(self, scene, cam, W, H, depth, samples=0, aperture=0.0, light_size=None, disp=None, shutter=0.0):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        if disp is not None:
            self.tr.set_motion(disp)
        self.args = (cam, W, H, depth)
        self.samples, self.aperture, self.light_size = samples, aperture, light_size
        self.disp, self.shutter = disp, shutter
        self.bufs = self.tr.alloc(W, H, rgba32f=True, rgba8=True)

    def frame(self):
        if self.disp is not None:
            self.tr.render_motion_into(*self.args, self.samples, self.aperture, self.light_size, self.shutter, self.bufs)
        elif self.light_size is not None:
            self.tr.render_soft_into(*self.args, self.samples, self.aperture, self.light_size, self.bufs)
        elif self.samples:
            self.tr.render_ss_into(*self.args, self.samples, self.bufs)
        else:
            self.tr.render_into(*self.args, self.bufs)

    def close(self):
        self.tr.close()


class Unfused:
    """S x S times [the displaced scene, rt_trace_rays_dev on the sample's rays], torch's pairwise tree (along a, then
    along b, times 1 / S^2) and the conversions to RGBA32F and RGBA8.  upload: one context, rt_set_scene before every
    trace; otherwise one context per sample with its scene uploaded here."""

    def __init__(self, scene, cam, W, H, depth, S, disp, F, upload):
        dev = torch.device("cuda", 0)
        self.W, self.H, self.S, self.depth, self.upload = W, H, S, depth, upload
        # (to_abi() replaces scene._keep, the arrays its rt_scene points to, on every call: hold every sample's)
        self.scenes, self.keep = [], []
        for b in range(S):
            row = []
            for a in range(S):
                row.append(displaced_scene(scene, disp, S, F, a, b))
                self.keep.append(scene._keep)
            self.scenes.append(row)
        n_tr = 1 if upload else S * S
        self.trs = [Tracer(0) for _ in range(n_tr)]
        if not upload:
            for b in range(S):
                for a in range(S):
                    self.trs[b * S + a].set_scene(self.scenes[b][a])
        starts, ends = lens_rays(cam, W, H, S, 0.0, dev)
        starts, ends = starts.view(S * H, S * W, 3), ends.view(S * H, S * W, 3)
        self.starts = [[starts[b::S, a::S].reshape(-1, 3).contiguous() for a in range(S)] for b in range(S)]
        self.ends = [[ends[b::S, a::S].reshape(-1, 3).contiguous() for a in range(S)] for b in range(S)]
        del starts, ends
        self.rgb = torch.empty((S, S, H, W, 3), dtype=torch.float64, device=dev)      # [b, a]
        self.bufs = {"rgba32f": torch.ones((H, W, 4), dtype=torch.float32, device=dev),
                     "rgba8": torch.full((H, W, 4), 255, dtype=torch.uint8, device=dev)}

    def frame(self):
        st = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        S = self.S
        for b in range(S):
            for a in range(S):
                tr = self.trs[0] if self.upload else self.trs[b * S + a]
                if self.upload:
                    tr.set_scene(self.scenes[b][a])
                abi.check(abi.lib().rt_trace_rays_dev(tr._ctx, ctypes.c_void_p(self.starts[b][a].data_ptr()),
                                                      ctypes.c_void_p(self.ends[b][a].data_ptr()), self.W * self.H,
                                                      self.depth, ctypes.c_void_p(self.rgb[b, a].data_ptr()), None, st),
                          "rt_trace_rays_dev")
        v = self.rgb
        n = S
        while n > 1:
            v = v[:, 0::2] + v[:, 1::2]
            n //= 2
        v = v[:, 0]
        n = S
        while n > 1:
            v = v[0::2] + v[1::2]
            n //= 2
        rgb = v[0] * (1.0 / (S * S))
        self.bufs["rgba32f"][..., :3] = rgb.float()
        self.bufs["rgba8"][..., :3] = torch.floor(torch.nan_to_num(rgb, nan=0.0).clamp(0.0, 1.0) * 255.0 + 0.5) \
            .to(torch.uint8)

    def close(self):
        for t in self.trs:
            t.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=20.0, help="GPU work per timed block")
    ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
    ap.add_argument("--shutter", type=float, default=1.0)
    ap.add_argument("--frames", type=int, default=0, help="> 0: only this many fused and unfused frames per S")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion", "bench_motion.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_motion: needs a HIP GPU")
    cfg = scenes.CONFIGS["c2"]
    W, H, depth = cfg.width, cfg.height, cfg.depth
    scene, cam = cfg.scene(), cfg.camera()
    F = a.shutter
    disp = [[0.0, 0.0, 0.0] for _ in scene.spheres]
    disp[MOVER][0] = a.move
    doc = {"config": "c2", "view": "static", "width": W, "height": H, "depth": depth, "moving_sphere": MOVER,
           "displacement": disp[MOVER], "shutter": F, "light_size": 0.0, "aperture": 0.0,
           "rounds": a.rounds, "unit": "ms per frame (device events around a block of frames)",
           "device": torch.cuda.get_device_name(0), "cases": []}
    for S in (2, 4):
        legs = {"fused": Leg(scene, cam, W, H, depth, samples=S, light_size=0.0, disp=disp, shutter=F),
                "unfused": Unfused(cfg.scene(), cam, W, H, depth, S, disp, F, upload=True),
                "unfused_no_upload": Unfused(cfg.scene(), cam, W, H, depth, S, disp, F, upload=False),
                "soft": Leg(scene, cam, W, H, depth, samples=S, light_size=0.0),
                "pinhole": Leg(scene, cam, W, H, depth, samples=S),
                "plain": Leg(scene, cam, W, H, depth)}
        for leg in legs.values():                       # first, calibration and cached renders
            for _ in range(4):
                leg.frame()
        torch.cuda.synchronize()
        fu = legs["fused"]
        for k in ("unfused", "unfused_no_upload"):
            if not same_bytes(fu, legs[k]):
                sys.exit(f"bench_motion: S={S}: the fused frame differs from the {k} route")
        changed = float((fu.bufs["rgba8"] != legs["soft"].bufs["rgba8"]).any(dim=2).double().mean())
        if a.frames > 0:
            for leg in (fu, legs["unfused_no_upload"]):
                for _ in range(a.frames):
                    leg.frame()
            torch.cuda.synchronize()
            print(f"bench_motion: S={S}: {a.frames} fused and unfused_no_upload frames")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 3), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            case = {"samples": S, "identical_bytes_fused_and_unfused": True,
                    "rgba8_pixels_changed_by_the_motion": round(changed, 5), "frames_per_block": n, "legs": {}}
            for k, v in times.items():
                case["legs"][k] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                                   "max_ms": round(max(v), 5)}
            L = case["legs"]
            for other in ("unfused", "unfused_no_upload", "soft", "pinhole", "plain"):
                Fu, O = L["fused"], L[other]
                case[f"fused_over_{other}"] = round(Fu["median_ms"] / O["median_ms"], 4)
                spread = (Fu["max_ms"] - Fu["min_ms"]) + (O["max_ms"] - O["min_ms"])
                gap = O["median_ms"] - Fu["median_ms"]
                case[f"fused_vs_{other}"] = "faster" if gap > spread else "slower" if -gap > spread else "no difference"
            doc["cases"].append(case)
        for leg in legs.values():
            leg.close()
        del legs, fu
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
