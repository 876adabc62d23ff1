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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from tools.sampled_bench import Leg, Unfused, parse_args, run  # noqa: E402

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


def main():
    def options(ap):
        ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
        ap.add_argument("--shutter", type=float, default=1.0)

    a = parse_args("bench_motion", __doc__, options)
    F = a.shutter
    disp = [[0.0, 0.0, 0.0] for _ in scenes.CONFIGS["c2"].scene().spheres]
    disp[MOVER][0] = a.move

    def legs(cfg, S):
        scene, view = cfg.scene(), (cfg.camera(), cfg.width, cfg.height, cfg.depth)

        def unfused(upload):
            sc = cfg.scene()
            return Unfused(sc, lambda i, j: displaced_scene(sc, disp, S, F, i, j), *view, S, 0.0, upload)

        return {"fused": Leg(scene, *view, samples=S, aperture=0.0, light_size=0.0, disp=disp, shutter=F),
                "unfused": unfused(True),
                "unfused_no_upload": unfused(False),
                "soft": Leg(scene, *view, samples=S, aperture=0.0, light_size=0.0),
                "pinhole": Leg(scene, *view, samples=S),
                "plain": Leg(scene, *view)}

    run("bench_motion", a, {"moving_sphere": MOVER, "displacement": disp[MOVER], "shutter": F, "light_size": 0.0,
                            "aperture": 0.0}, legs,
        {"unfused": "unfused", "unfused_no_upload": "unfused_no_upload"}, "soft",
        "rgba8_pixels_changed_by_the_motion", "unfused_no_upload")


if __name__ == "__main__":
    main()
