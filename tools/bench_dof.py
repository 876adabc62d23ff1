#!/usr/bin/env python3
"""What the thin-lens kernel costs and what fusing it buys: c2 frames (1920 x 1080 output, depth 1, static view) at
S = 2 and S = 4 samples per axis and lens half-width A = 8, four legs timed in one process, alternating in blocks:

  fused     rt_render_dof_dev writing RGBA32F + RGBA8 (one launch: rays formed, traced and reduced in the kernel)
  unfused   the same rays as a list built once with torch, traced by rt_trace_rays_dev, then torch's pairwise tree
            and the two conversions; timed from the trace onward (building the list is not counted)
  pinhole   rt_render_ss_dev of the same S writing RGBA32F + RGBA8: the price of the lens is the generic trace path
            against the specialised render kernels
  plain     the one-sample c2 frame (RGBA32F + RGBA8)

Before timing, the fused and the unfused frame must be equal byte for byte (no oracle involved).  Every leg has its
own context and is warmed through its first, calibration and cached renders; a timed block is at least --block-ms
of GPU work between two events.  Reports median (min - max) per frame and the ratios fused / unfused and
fused / pinhole; one leg is called faster only where the gap exceeds the two legs' spreads added.
Writes one JSON document (default profiles/dof/bench_dof.json) and prints it.

  python tools/bench_dof.py [--rounds 7] [--block-ms 20] [--aperture 8] [--frames N] [--out FILE]

--frames N (> 0) only runs N fused and N unfused frames per S after the warm-up and writes nothing: the workload
for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_dof.py --frames 20).
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

from oracle import pyoracle as po  # noqa: E402
from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402


def lens_rays(cam, W, H, S, A, dev):
    """The contract's rays in sample-grid order -> (starts, ends) [S H * S W, 3] float64 on `dev`; each product and
    sum is one IEEE operation, in the contract's order."""
    cam_s = abi.rt_camera()
    abi.check(abi.lib().rt_camera_supersample(ctypes.byref(cam), S, ctypes.byref(cam_s)), "rt_camera_supersample")
    right, upp = (torch.tensor(v, dtype=torch.float64, device=dev) for v in po.camera_basis(cam_s))
    look = torch.tensor(cam_s.look_at[:], dtype=torch.float64, device=dev)
    eye = torch.tensor(cam_s.eye[:], dtype=torch.float64, device=dev)
    ii = torch.arange(S * W, device=dev)
    jj = torch.arange(S * H, device=dev)
    a = cam_s.pitch * (ii + cam_s.bottom_x).double()
    b = cam_s.pitch * (jj + cam_s.bottom_y).double()
    ends = (look + a[None, :, None] * right) + b[:, None, None] * upp
    ta = (2 * (ii % S) + 1 - S).double() / float(S)
    tb = (2 * (jj % S) + 1 - S).double() / float(S)
    starts = (eye + (A * ta)[None, :, None] * right) + (A * tb)[:, None, None] * upp
    return starts.expand_as(ends).reshape(-1, 3).contiguous(), ends.reshape(-1, 3).contiguous()


class Leg:
    """One frame per call into fixed buffers: fused (aperture given), pinhole (samples > 0) or plain."""

    def __init__(self, scene, cam, W, H, depth, samples=0, aperture=None):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.args = (cam, W, H, depth)
        self.samples, self.aperture = samples, aperture
        self.bufs = self.tr.alloc(W, H, rgba32f=True, rgba8=True)

    def frame(self):
        if self.aperture is not None:
            self.tr.render_dof_into(*self.args, self.samples, self.aperture, self.bufs)
        elif self.samples:
            self.tr.render_ss_into(*self.args, self.samples, self.bufs)
        else:
            self.tr.render_into(*self.args, self.bufs)


class Unfused:
    """rt_trace_rays_dev on the ray list, torch's pairwise tree (along a, then along b, times 1 / S^2) and the
    conversions to RGBA32F and RGBA8."""

    def __init__(self, scene, cam, W, H, depth, S, A):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        dev = torch.device("cuda", 0)
        self.W, self.H, self.S, self.depth = W, H, S, depth
        self.starts, self.ends = lens_rays(cam, W, H, S, A, dev)
        self.rgb = torch.empty((self.starts.shape[0], 3), dtype=torch.float64, device=dev)
        self.bufs = {"rgba32f": torch.ones((H, W, 4), dtype=torch.float32, device=dev),
                     "rgba8": torch.full((H, W, 4), 255, dtype=torch.uint8, device=dev)}

    def frame(self):
        st = torch.cuda.current_stream(0)
        abi.check(abi.lib().rt_trace_rays_dev(self.tr._ctx, ctypes.c_void_p(self.starts.data_ptr()),
                                              ctypes.c_void_p(self.ends.data_ptr()), self.starts.shape[0], self.depth,
                                              ctypes.c_void_p(self.rgb.data_ptr()), None,
                                              ctypes.c_void_p(st.cuda_stream)), "rt_trace_rays_dev")
        v = self.rgb.view(self.H, self.S, self.W, self.S, 3)
        n = self.S
        while n > 1:
            v = v[:, :, :, 0::2] + v[:, :, :, 1::2]
            n //= 2
        v = v[:, :, :, 0]
        n = self.S
        while n > 1:
            v = v[:, 0::2] + v[:, 1::2]
            n //= 2
        rgb = v[:, 0] * (1.0 / (self.S * self.S))
        self.bufs["rgba32f"][..., :3] = rgb.float()
        self.bufs["rgba8"][..., :3] = torch.floor(torch.nan_to_num(rgb, nan=0.0).clamp(0.0, 1.0) * 255.0 + 0.5) \
            .to(torch.uint8)


def block_ms(leg, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        leg.frame()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=20.0, help="GPU work per timed block")
    ap.add_argument("--aperture", type=float, default=8.0)
    ap.add_argument("--frames", type=int, default=0, help="> 0: only this many fused and unfused frames per S")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dof", "bench_dof.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_dof: needs a HIP GPU")
    cfg = scenes.CONFIGS["c2"]
    W, H, depth = cfg.width, cfg.height, cfg.depth
    scene, cam = cfg.scene(), cfg.camera()
    doc = {"config": "c2", "view": "static", "width": W, "height": H, "depth": depth, "aperture": a.aperture,
           "rounds": a.rounds, "unit": "ms per frame (device events around a block of frames)",
           "device": torch.cuda.get_device_name(0), "cases": []}
    for S in (2, 4):
        legs = {"fused": Leg(scene, cam, W, H, depth, samples=S, aperture=a.aperture),
                "unfused": Unfused(scene, cam, W, H, depth, S, a.aperture),
                "pinhole": Leg(scene, cam, W, H, depth, samples=S),
                "plain": Leg(scene, cam, W, H, depth)}
        for leg in legs.values():                       # first, calibration and cached renders
            for _ in range(4):
                leg.frame()
        torch.cuda.synchronize()
        fu, un = legs["fused"], legs["unfused"]
        same = torch.equal(fu.bufs["rgba8"], un.bufs["rgba8"]) and \
            torch.equal(fu.bufs["rgba32f"].view(torch.int32), un.bufs["rgba32f"].view(torch.int32))
        if not same:
            sys.exit(f"bench_dof: S={S}: the fused frame differs from the ray-list route")
        changed = float((fu.bufs["rgba8"] != legs["pinhole"].bufs["rgba8"]).any(dim=2).double().mean())
        if a.frames > 0:
            for leg in (fu, un):
                for _ in range(a.frames):
                    leg.frame()
            torch.cuda.synchronize()
            print(f"bench_dof: S={S}: {a.frames} fused and unfused frames")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 3), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            case = {"samples": S, "identical_bytes_fused_and_unfused": True,
                    "rgba8_pixels_changed_by_the_lens": round(changed, 5), "frames_per_block": n, "legs": {}}
            for k, v in times.items():
                case["legs"][k] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                                   "max_ms": round(max(v), 5)}
            L = case["legs"]
            for other in ("unfused", "pinhole", "plain"):
                F, O = L["fused"], L[other]
                case[f"fused_over_{other}"] = round(F["median_ms"] / O["median_ms"], 4)
                spread = (F["max_ms"] - F["min_ms"]) + (O["max_ms"] - O["min_ms"])
                gap = O["median_ms"] - F["median_ms"]
                case[f"fused_vs_{other}"] = "faster" if gap > spread else "slower" if -gap > spread else "no difference"
            doc["cases"].append(case)
        for leg in legs.values():
            leg.tr.close()
        del legs, fu, un
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
