#!/usr/bin/env python3
"""What a list of windows saves: tools/bench_window.py's c2 frames and arguments (1920 x 1080 output, depth 1, R = 40,
the sphere on c4 moving by |d| = 40, F = 1, A = 0, the eye moving by 40 along y, J = 16; accum (0, 16) and converge K = 64,
M = 4, E = 1 / 255 from a zeroed count, RGBA32F + RGBA8), per S in {1, 2} and per call these legs, every one in place in
full-frame buffers, timed in one process, alternating in blocks:

  full          the un-windowed call
  whole         the single-window call on (0, 0, width, height)
  one           the list call on the list of that one window: against `whole`, the price of the lookup alone
  grid4x4.calls, grid4x4.list
                the frame as 4 x 4 tiles of 480 x 270: one single-window call per tile / one list call
  strips8.calls, strips8.list
                the frame as distributed.window_plan(width, height, 8) strips, likewise
  bands.calls, bands.list
                rank 0's distributed.band_windows(width, height, 8, 0, 8): 17 bands of 8 rows, an eighth of the frame
  region.calls, region.list
                the 512 x 512 region at (704, 284): one single-window call on it / the list of its 4096 windows of
                8 x 8 pixels (RT_MAX_WINDOWS; the whole frame would be 32 400): what a device-built list of live tiles
                would pay per tile, at worst

Before timing, every leg's sums (for converge also the sums of squares and counts) and both images must be the `full`
leg's bytes on the leg's own pixels; the list's `active` must be the sum of its `.calls` leg's, and the partitions' must
be the un-windowed call's.  Every leg has its own context and is warmed through two calls; a timed block is at least
--block-ms of GPU work between two events.  Reports median (min - max) per frame of the leg; a leg is called slower or
faster than another only where the gap exceeds the two legs' spreads added.  Writes one JSON document (default
profiles/window_list/bench_window_list.json) and prints it.

  python tools/bench_window_list.py [--rounds 7] [--block-ms 20] [--seed 1] [--frames N [--legs full,grid4x4.list]]
                                    [--case N] [--out FILE]

--frames N (> 0) only runs N frames of each leg of --legs per case after the warm-up and writes nothing: the workload
for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_window_list.py --frames 5 --case 0).
"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.distributed import band_windows, window_plan  # noqa: E402
from tools.bench_accum import J, MOVER, stats, verdict  # noqa: E402
from tools.bench_window import E, M, PASSES, Leg, grid_plan  # noqa: E402
from tools.sampled_bench import block_ms, parse_args  # noqa: E402

REGION = (704, 284, 512, 512)
PAIRS = ("grid4x4", "strips8", "bands", "region")
PARTITIONS = ("grid4x4", "strips8")


class ListLeg(Leg):
    """One frame of the call `kind` per frame(): one list call on `windows`, in place."""

    def __init__(self, kind, windows, *rest):
        super().__init__(kind, windows, False, *rest)
        self.tr.set_windows(*self.frame_size, windows, "inplace")

    def frame(self, count_active=False):
        t = self.tr
        if self.kind == "accum":
            t.render_accum_windows_into(self.cam, self.camera, *self.frame_size, *self.size, self.seed, 0, self.K,
                                        *self.tail, self.state[0], self.bufs)
        else:
            self.state[2].zero_()
            t.render_converge_windows_into(self.cam, self.camera, *self.frame_size, *self.size, self.seed, self.K, M, E,
                                           *self.tail, self.state, self.bufs, self.active)
        self.active_sum = int(self.active[0]) if count_active and self.kind == "converge" else 0


def mask_of(windows, W, H, dev):
    m = torch.zeros((H, W), dtype=torch.bool, device=dev)
    for x0, y0, w, h in windows:
        m[y0:y0 + h, x0:x0 + w] = True
    return m


def same_on(x, y, m):
    """x and y hold the same bytes on the pixels of the mask m."""
    xb = x.contiguous().view(torch.uint8).reshape(m.shape + (-1,))
    yb = y.contiguous().view(torch.uint8).reshape(m.shape + (-1,))
    return bool(torch.equal(xb[m], yb[m]))


def main():
    def options(ap):
        ap.add_argument("--move", type=float, default=40.0, help="|d| of the moving sphere, along x")
        ap.add_argument("--eye-move", type=float, default=40.0, help="|move| of the eye, along y")
        ap.add_argument("--light-size", type=float, default=40.0)
        ap.add_argument("--shutter", type=float, default=1.0)
        ap.add_argument("--seed", type=int, default=1)
        ap.add_argument("--case", type=int, default=-1, help="only case N of the four (S, call) cases (for a kernel trace)")
        ap.add_argument("--legs", default="full,grid4x4.list", help="the legs --frames runs, in this order")

    a = parse_args("bench_window_list", __doc__, options)
    cfg = scenes.CONFIGS["c2"]
    disp = [[0.0, 0.0, 0.0] for _ in cfg.scene().spheres]
    disp[MOVER][0] = a.move
    eye_move = [0.0, a.eye_move, 0.0]
    W, H = cfg.width, cfg.height
    rx, ry, rw, rh = REGION
    lists = {"grid4x4": grid_plan(W, H, 4, 4), "strips8": window_plan(W, H, 8), "bands": band_windows(W, H, 8, 0, 8),
             "region": [(rx + 8 * i, ry + 8 * j, 8, 8) for j in range(rh // 8) for i in range(rw // 8)]}
    assert len(lists["region"]) == 4096
    # leg -> (its windows, None: the un-windowed call; as a list call)
    plans = {"full": (None, False), "whole": ([(0, 0, W, H)], False), "one": ([(0, 0, W, H)], True)}
    for k in PAIRS:
        plans[k + ".calls"] = ([REGION] if k == "region" else lists[k], False)
        plans[k + ".list"] = (lists[k], True)
    doc = {"config": "c2", "view": "static", "width": W, "height": H, "depth": cfg.depth, "moving_sphere": MOVER,
           "displacement": disp[MOVER], "eye_move": eye_move, "look_at_move": [0.0, 0.0, 0.0], "shutter": a.shutter,
           "light_size": a.light_size, "aperture": 0.0, "jitter": J, "seed": a.seed, "passes": PASSES, "min_passes": M,
           "tolerance": E, "windows": {k: (len(v), v[:2]) for k, v in lists.items()}, "region": REGION,
           "rounds": a.rounds, "unit": "ms per frame of the leg (device events around a block of frames)",
           "device": torch.cuda.get_device_name(0), "not_measured": "other scenes, depths and motions", "cases": []}
    if a.frames > 0:                                        # a trace holds the kernels of the legs asked for alone
        plans = {k: v for k, v in plans.items() if k == "full" or k in a.legs.split(",")}
    cases = [(S, kind) for S in (1, 2) for kind in ("accum", "converge")]
    for S, kind in cases if a.case < 0 else cases[a.case:a.case + 1]:
        rest = (cfg.scene(), cfg.camera(), W, H, cfg.depth, S, a.light_size, a.shutter, disp, a.seed,
                scenes.camera_motion(eye=eye_move))
        legs = {k: (ListLeg(kind, wins, *rest) if as_list else Leg(kind, wins, False, *rest))
                for k, (wins, as_list) in plans.items()}
        for leg in legs.values():
            leg.frame()
            leg.frame(count_active=True)
        torch.cuda.synchronize()
        full, active_full = legs["full"].tensors(), legs["full"].active_sum
        dev = full["accum"].device
        for k, leg in legs.items():
            wins = plans[k][0]
            m = mask_of(wins if wins is not None else [(0, 0, W, H)], W, H, dev)
            for name, t in leg.tensors().items():
                if not same_on(t, full[name], m):
                    sys.exit(f"bench_window_list: S={S} {kind}: {name} of the leg {k} differs from the un-windowed call's")
        if kind == "converge":
            for k in PAIRS:
                if k + ".list" in legs and k + ".calls" in legs and k != "region" and \
                        legs[k + ".list"].active_sum != legs[k + ".calls"].active_sum:
                    sys.exit(f"bench_window_list: S={S}: the active count of the list {k} is not its calls' sum")
            for k in ("whole", "one") + tuple(p + ".list" for p in PARTITIONS):
                if k in legs and legs[k].active_sum != active_full:
                    sys.exit(f"bench_window_list: S={S}: the active count of the leg {k} is off")
        if a.frames > 0:
            for k in a.legs.split(","):
                for _ in range(a.frames):
                    legs[k].frame()
            torch.cuda.synchronize()
            print(f"bench_window_list: S={S} {kind}: {a.frames} frames of each of the legs {a.legs}")
        else:
            n = {k: max(3, math.ceil(a.block_ms / max(block_ms(leg, 2), 1e-3))) for k, leg in legs.items()}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, leg in legs.items():
                    times[k].append(block_ms(leg, n[k]))
            L = {k: stats(v) for k, v in times.items()}
            groups = math.ceil(PASSES[kind] / 4)
            case = {"samples": S, "call": kind, "identical_bytes": True, "frames_per_block": n, "legs": L,
                    "launches_per_frame": {k: (1 if wins is None or as_list else len(wins)) * groups
                                           for k, (wins, as_list) in plans.items()}}
            if kind == "converge":
                case["active"] = {k: leg.active_sum for k, leg in legs.items()}
            ratio = lambda x, y: round(L[x]["median_ms"] / L[y]["median_ms"], 4)  # noqa: E731
            case["one_over_whole"], case["one_vs_whole"] = ratio("one", "whole"), verdict(L["one"], L["whole"])
            case["one_over_full"], case["whole_over_full"] = ratio("one", "full"), ratio("whole", "full")
            for k in PAIRS:
                case[f"{k}_list_over_calls"] = ratio(k + ".list", k + ".calls")
                case[f"{k}_list_vs_calls"] = verdict(L[k + ".list"], L[k + ".calls"])
            for k in PARTITIONS:
                case[f"{k}_list_over_full"] = ratio(k + ".list", "full")
                case[f"{k}_list_vs_full"] = verdict(L[k + ".list"], L["full"])
                case[f"{k}_calls_over_full"] = ratio(k + ".calls", "full")
            doc["cases"].append(case)
        for leg in legs.values():
            leg.close()
        del legs, full
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
