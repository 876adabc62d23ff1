#!/usr/bin/env python3
"""What stopping converged pixels saves, and what the bookkeeping costs: bench_accum.py's c2 frames (1920 x 1080 output,
depth 1), square light panels of half-width R = 40, the sphere on c4 moving by |d| = 40 along x, shutter F = 1, pinhole
(A = 0), the eye moving by |move| = 40 along y, J = 16 sub-positions, a budget of K = 64 passes, M = 4; per
(S, E) in {1, 2} x {1 / 255, 4 / 255} three legs are timed in one process, alternating in blocks:

  converge   one rt_render_converge_dev call of K passes from a zeroed count (the zeroing is part of the leg), writing
             RGBA32F + RGBA8 of the mean and the active count
  accum      one rt_render_accum_dev call (0, K), writing both images: every pixel gets every pass
  nostop     the converge leg with M = K + 1: nothing stops, so it traces what the accum leg traces and pays for the
             sums of squares and the rule on top

Before timing, the nostop leg's sums and images must be the accum leg's bytes and a second converge call must repeat the
first.  Every leg has its own context and is warmed through two calls; a timed block is at least --block-ms of GPU work
between two events.  Reports median (min - max) per call; from the converge leg's `count` the share of pixel-passes
traced and the share of wave-passes traced (a wave runs as many passes as the pixel of its 8 x 8 sample tile that
receives most), also per launch of 4 passes; `active`; and the RMS difference of each leg's RGB64F mean to the mean of 256 rt_render_accum_dev passes.
A leg is called slower or faster only where the gap exceeds the two legs' spreads added.  Writes one JSON document
(default profiles/converge/bench_converge.json) and prints it.

  python tools/bench_converge.py [--rounds 7] [--block-ms 20] [--move 40] [--eye-move 40] [--light-size 40] [--seed 1]
                                 [--passes 64] [--frames N [--legs converge,accum]] [--case N] [--out FILE]

--frames N (> 0) only runs N calls of each leg of --legs, in that order, per case after the warm-up and writes nothing:
the workload for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_converge.py --frames 5 --case 2)
or for counters (rocprofv3 --pmc ... -- python tools/bench_converge.py --frames 2 --case 2 --legs nostop,accum: the
last 2 x 16 dispatches of each kernel are those calls).
"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402
from tools.bench_accum import J, MOVER, stats, verdict  # noqa: E402
from tools.sampled_bench import block_ms, parse_args  # noqa: E402

M = 4
REF_PASSES = 256


class Leg:
    """One call of the leg `kind` per frame() into fixed buffers."""

    def __init__(self, kind, scene, cam, W, H, depth, S, K, E, R, F, disp, seed, camera):
        self.tr = Tracer(0)
        self.tr.set_scene(scene)
        self.tr.set_motion(disp)
        self.kind, self.K, self.E, self.seed = kind, K, E, seed
        self.cam, self.camera, self.size, self.tail = cam, camera, (W, H, depth, S, J), (0.0, R, F)
        self.bufs = self.tr.alloc(W, H, rgba32f=True, rgba8=True)
        self.state = self.tr.alloc_converge(W, H)
        self.acc = self.state[0]
        self.active = torch.zeros((1,), dtype=torch.int32, device=self.acc.device)

    def frame(self, bufs=None):
        t, bufs = self.tr, bufs or self.bufs
        if self.kind == "accum":
            t.render_accum_into(self.cam, self.camera, *self.size, self.seed, 0, self.K, *self.tail, self.acc, bufs)
        else:
            self.state[2].zero_()
            t.render_converge_into(self.cam, self.camera, *self.size, self.seed, self.K,
                                   self.K + 1 if self.kind == "nostop" else M, self.E, *self.tail, self.state, bufs,
                                   self.active)

    def mean(self, W, H):
        """The leg's RGB64F mean, from a call outside the timing."""
        bufs = self.tr.alloc(W, H, rgba32f=False, rgb64f=True)
        self.frame(bufs)
        torch.cuda.synchronize()
        return bufs["rgb64f"]

    def close(self):
        self.tr.close()


def shares(count, S, K, L=4):
    """(pixel-passes, wave-passes) traced over those of K passes for every pixel, and per launch of L passes (the
    default launch split) the wave-passes traced over L passes for every wave."""
    n = count.to(torch.int64)
    t = 8 // S
    H, W = n.shape
    pad = torch.zeros(((H + t - 1) // t * t, (W + t - 1) // t * t), dtype=torch.int64, device=n.device)
    pad[:H, :W] = n
    tiles = pad.view(pad.shape[0] // t, t, pad.shape[1] // t, t).amax(dim=(1, 3))
    by_launch = [round(float((tiles - p).clamp(0, L).sum()) / (tiles.numel() * L), 5) for p in range(0, K, L)]
    return float(n.sum()) / (H * W * K), float(tiles.sum()) / (tiles.numel() * K), by_launch


def main():
    def options(ap):
        ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
        ap.add_argument("--eye-move", type=float, default=40.0, help="|move| of the eye, along y")
        ap.add_argument("--light-size", type=float, default=40.0)
        ap.add_argument("--shutter", type=float, default=1.0)
        ap.add_argument("--seed", type=int, default=1)
        ap.add_argument("--passes", type=int, default=64, help="the budget K")
        ap.add_argument("--case", type=int, default=-1, help="only case N of the four (S, E) cases (for a kernel trace)")
        ap.add_argument("--legs", default="converge,accum", help="the legs --frames runs, in this order")

    a = parse_args("bench_converge", __doc__, options)
    cfg = scenes.CONFIGS["c2"]
    K = a.passes
    disp = [[0.0, 0.0, 0.0] for _ in cfg.scene().spheres]
    disp[MOVER][0] = a.move
    eye_move = [0.0, a.eye_move, 0.0]
    W, H = cfg.width, cfg.height
    doc = {"config": "c2", "view": "static", "width": W, "height": H, "depth": cfg.depth, "moving_sphere": MOVER,
           "displacement": disp[MOVER], "eye_move": eye_move, "look_at_move": [0.0, 0.0, 0.0], "shutter": a.shutter,
           "light_size": a.light_size, "aperture": 0.0, "jitter": J, "seed": a.seed, "budget": K, "min_passes": M,
           "reference_passes": REF_PASSES, "rounds": a.rounds,
           "unit": "ms per call (device events around a block of calls)", "device": torch.cuda.get_device_name(0),
           "not_measured": "other scenes, depths and motions", "cases": []}
    cases = ((1, 1.0 / 255.0), (1, 4.0 / 255.0), (2, 1.0 / 255.0), (2, 4.0 / 255.0))
    kinds = ("converge", "accum", "nostop")
    for S, E in cases if a.case < 0 else cases[a.case:a.case + 1]:
        view = (cfg.camera(), W, H, cfg.depth)
        legs = {k: Leg(k, cfg.scene(), *view, S, K, E, a.light_size, a.shutter, disp, a.seed,
                       scenes.camera_motion(eye=eye_move)) for k in kinds}
        for leg in legs.values():
            for _ in range(2):
                leg.frame()
        torch.cuda.synchronize()
        co, ac, ns = legs["converge"], legs["accum"], legs["nostop"]
        if not torch.equal(ns.acc.view(torch.int64), ac.acc.view(torch.int64)):
            sys.exit(f"bench_converge: S={S}: the sums of the nostop leg differ from the accum leg's")
        if not (torch.equal(ns.bufs["rgba8"], ac.bufs["rgba8"]) and
                torch.equal(ns.bufs["rgba32f"].view(torch.int32), ac.bufs["rgba32f"].view(torch.int32))):
            sys.exit(f"bench_converge: S={S}: the images of the nostop leg differ from the accum leg's")
        if int(ns.active[0]) != W * H or not bool((ns.state[2] == K).all()):
            sys.exit(f"bench_converge: S={S}: the nostop leg stopped a pixel")
        first = [t.clone() for t in (*co.state, co.bufs["rgba8"], co.bufs["rgba32f"], co.active)]
        co.frame()
        torch.cuda.synchronize()
        now = (*co.state, co.bufs["rgba8"], co.bufs["rgba32f"], co.active)
        if not all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(first, now)):
            sys.exit(f"bench_converge: S={S} E={E}: two converge calls of equal arguments differ")
        if a.frames > 0:
            for k in a.legs.split(","):
                for _ in range(a.frames):
                    legs[k].frame()
            torch.cuda.synchronize()
            print(f"bench_converge: S={S} E={E}: {a.frames} calls of each of the legs {a.legs}")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 2), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            L = {k: stats(v) for k, v in times.items()}
            px_share, wave_share, by_launch = shares(co.state[2], S, K)
            ref_leg = Leg("accum", cfg.scene(), *view, S, REF_PASSES, E, a.light_size, a.shutter, disp, a.seed,
                          scenes.camera_motion(eye=eye_move))
            ref = ref_leg.mean(W, H)
            rms = {k: float(torch.sqrt(torch.mean((legs[k].mean(W, H) - ref) ** 2))) for k in kinds}
            ref_leg.close()
            del ref
            ratio = L["converge"]["median_ms"] / L["accum"]["median_ms"]
            case = {"samples": S, "tolerance": E, "nostop_is_accum_bytes": True, "calls_per_block": n, "legs": L,
                    "active": int(co.active[0]), "active_share": round(int(co.active[0]) / (W * H), 5),
                    "pixel_passes_traced_share": round(px_share, 5), "wave_passes_traced_share": round(wave_share, 5),
                    "wave_passes_traced_share_by_launch_of_4": by_launch,
                    "rms_to_256_pass_mean": {k: float(f"{v:.6g}") for k, v in rms.items()},
                    "nostop_over_accum": round(L["nostop"]["median_ms"] / L["accum"]["median_ms"], 4),
                    "nostop_vs_accum": verdict(L["nostop"], L["accum"]),
                    "converge_over_accum": round(ratio, 4), "converge_vs_accum": verdict(L["converge"], L["accum"]),
                    "converge_over_accum_minus_wave_share": round(ratio - wave_share, 4)}
            doc["cases"].append(case)
        for leg in legs.values():
            leg.close()
        del legs, co, ac, ns, first, now
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
