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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402
from tools.sampled_bench import (Leg, convert, current_stream, lens_rays, parse_args, run, trace_rays,  # noqa: E402
                                 unfused_bufs)


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
        self.bufs = unfused_bufs(W, H, dev)

    def frame(self):
        trace_rays(self.tr, self.starts, self.ends, self.depth, self.rgb, current_stream())
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
        convert(v[:, 0] * (1.0 / (self.S * self.S)), self.bufs)

    def close(self):
        self.tr.close()


def main():
    a = parse_args("bench_dof", __doc__, lambda ap: ap.add_argument("--aperture", type=float, default=8.0))

    def legs(cfg, S):
        scene, view = cfg.scene(), (cfg.camera(), cfg.width, cfg.height, cfg.depth)
        return {"fused": Leg(scene, *view, samples=S, aperture=a.aperture),
                "unfused": Unfused(scene, *view, S, a.aperture),
                "pinhole": Leg(scene, *view, samples=S),
                "plain": Leg(scene, *view)}

    run("bench_dof", a, {"aperture": a.aperture}, legs, {"unfused": "ray-list"}, "pinhole",
        "rgba8_pixels_changed_by_the_lens", "unfused")


if __name__ == "__main__":
    main()
