#!/usr/bin/env python3
"""What the soft-shadow kernel costs and what fusing it buys: c2 frames (1920 x 1080 output, depth 1, static view) at
S = 2 and S = 4 samples per axis, light half-width R = 40, pinhole (A = 0); the legs are timed in one process,
alternating in blocks:

  fused            rt_render_soft_dev writing RGBA32F + RGBA8 (one launch: rays and light points formed, traced and
                   reduced in the kernel)
  unfused          what a caller without the kernel does: for each of the S x S samples, rt_set_scene of the scene with
                   the lights at that sample's panel points and rt_trace_rays_dev on that sample's W H rays (lists built
                   once with torch); then torch's pairwise tree and the two conversions
  unfused_no_upload  the same with one context per sample, its displaced scene uploaded beforehand: the S x S traces,
                   the tree and the conversions without the scene uploads
  lens             rt_render_dof_dev of the same S and A writing RGBA32F + RGBA8: the same rays with point lights, i.e.
                   the price of losing the light-cone filter of the shadow test
  pinhole          rt_render_ss_dev of the same S (the specialised render kernels)
  plain            the one-sample c2 frame

Before timing, the fused frame and both unfused frames must be equal byte for byte (no oracle involved).  Every leg
has its own context(s) and is warmed through its first, calibration and cached renders; a timed block is at least
--block-ms of GPU work between two events.  Reports median (min - max) per frame and the ratios of the fused leg to
the others; one leg is called faster only where the gap exceeds the two legs' spreads added.
Writes one JSON document (default profiles/soft/bench_soft.json) and prints it.

  python tools/bench_soft.py [--rounds 7] [--block-ms 20] [--light-size 40] [--aperture 0] [--frames N] [--out FILE]

--frames N (> 0) only runs N fused and N unfused_no_upload frames per S after the warm-up and writes nothing: the
workload for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_soft.py --frames 20).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.sampled_bench import Leg, Unfused, parse_args, run  # noqa: E402


def displaced_scene(scene, S, R, a, b):
    """The rt_scene of `scene` with every light at point (a, b) of its panel (include/rt_api.h, soft shadows rule 2),
    in Python floats: IEEE binary64, one operation per product and sum."""
    s = scene.to_abi()
    ta, tb = float(2 * a + 1 - S) / float(S), float(2 * b + 1 - S) / float(S)
    for k in range(s.n_lights):
        s.lights[k].position[0] = s.lights[k].position[0] + (R * ta)
        s.lights[k].position[2] = s.lights[k].position[2] + (R * tb)
    return s


def main():
    def options(ap):
        ap.add_argument("--light-size", type=float, default=40.0)
        ap.add_argument("--aperture", type=float, default=0.0)

    a = parse_args("bench_soft", __doc__, options)
    R, A = a.light_size, a.aperture

    def legs(cfg, S):
        scene, view = cfg.scene(), (cfg.camera(), cfg.width, cfg.height, cfg.depth)

        def unfused(upload):
            sc = cfg.scene()
            return Unfused(sc, lambda i, j: displaced_scene(sc, S, R, i, j), *view, S, A, upload)

        return {"fused": Leg(scene, *view, samples=S, aperture=A, light_size=R),
                "unfused": unfused(True),
                "unfused_no_upload": unfused(False),
                "lens": Leg(scene, *view, samples=S, aperture=A),
                "pinhole": Leg(scene, *view, samples=S),
                "plain": Leg(scene, *view)}

    run("bench_soft", a, {"light_size": R, "aperture": A}, legs,
        {"unfused": "unfused", "unfused_no_upload": "unfused_no_upload"}, "lens",
        "rgba8_pixels_changed_by_the_light_size", "unfused_no_upload")


if __name__ == "__main__":
    main()
