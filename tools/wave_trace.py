#!/usr/bin/env python3
"""Per-wave timeline of one rt_render_kernel launch (diagnostic; needs the RT_WAVE_TRACE=1 build (copied over lib/librt_amd.so) from
tools/variants.sh, e.g. `bash tools/variants.sh trace=-DRT_WAVE_TRACE=1`).
Reports wave durations, concurrent waves over time (per XCD and total) and the tail.
The traced launch is a cached render of the calibrated view: with runs of sky tiles (RT_SKY_RUN_MAX, 16 by default) it
has one wave per dispatch position — a tracing tile or a run — and the kernel records waves by position, so the
positions the launch really had (rt_diag_disp_count) say how many records to read; RT_SKY_RUN_MAX=1 in the environment
traces the plain table, one wave per tile.
Every record names its position's tile, and the context's class grid (rt_diag_tile_class_grid: decided at calibration
whether or not RT_TILE_CLASSES lets the records carry it) splits the per-phase figures into sky positions, sphere-free
tiles and the other tracing tiles — under RT_TILE_CLASSES=0 the same tiles on the general path.  The sphere-free tiles
are split again by the flat grid (rt_diag_flat_tile_grid, likewise decided whatever RT_FLAT_TILES says): flat tiles, on the
straight-line path or (RT_FLAT_TILES=0) on the sphere-free one, and the sphere-free tiles that are not flat.
usage: wave_trace.py [config]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "c2"
    cfg = scenes.CONFIGS[name]
    W, H = cfg.width, cfg.height
    t = Tracer(0)
    t.set_scene(cfg.scene())
    bufs = t.alloc(W, H, rgba32f=True, rgba8=True)
    nwg = ((W + 7) // 8) * ((H + 7) // 8)
    tr = torch.zeros(nwg * 7, dtype=torch.int64, device="cuda")   # RT_WAVE_TRACE=2: + {tile row, cone, trace} stamps
    lib = abi.lib()
    lib.rt_debug_wave_trace.argtypes = [ctypes.c_void_p]
    for _ in range(3):
        t.render_into(cfg.camera(), W, H, cfg.depth, bufs)
    torch.cuda.synchronize()
    assert lib.rt_debug_wave_trace(ctypes.c_void_p(tr.data_ptr())) == 0
    t.render_into(cfg.camera(), W, H, cfg.depth, bufs)
    torch.cuda.synchronize()
    # the traced launch's positions: records 0 .. n - 1 of both blocks (the second starts behind 4 words per TILE)
    pos, tiles, run_max = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    abi.check(lib.rt_diag_disp_count(t._ctx, ctypes.byref(pos), ctypes.byref(tiles), ctypes.byref(run_max)),
              "rt_diag_disp_count")
    n = pos.value if tiles.value == nwg else nwg
    ab = tr.cpu().numpy()
    a = ab[: nwg * 4].reshape(nwg, 4)[:n]
    b = ab[nwg * 4:].reshape(nwg, 3)[:n]
    if not a[:, 0].all():
        raise SystemExit(f"wave_trace: {int((a[:, 0] == 0).sum())} of {n} positions left no record "
                         "(is lib/librt_amd.so an RT_WAVE_TRACE build?)")
    st, en, hw, md = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    t0 = st.min()
    st, en, md = ((x - t0) * 10.0 / 1000.0 for x in (st, en, md))      # 100 MHz ticks -> us
    t_ty, t_cone, t_tr = ((x - t0) * 10.0 / 1000.0 for x in (b[:, 0], b[:, 1], b[:, 2]))
    dur = en - st
    hwid = hw & 0xFFFFFFFF
    xcc = (hw >> 32) & 0xF
    tile_x, tile_y = (hw >> 36) & 0x3FFF, (hw >> 50) & 0x3FFF
    cu = (hwid >> 8) & 0xF
    se = (hwid >> 13) & 0x7
    simd = (hwid >> 4) & 0x3
    grid = np.linspace(0, en.max(), 41)
    conc = [int(((st <= x) & (en > x)).sum()) for x in grid]
    out = {
        "config": name, "waves": int(n), "tiles": int(nwg), "run_max": run_max.value, "span_us": round(float(en.max()), 2),
        "dur_us": {q: round(float(np.percentile(dur, q)), 2) for q in (5, 25, 50, 75, 95, 99, 100)},
        "mean_dur_us": round(float(dur.mean()), 3),
        "prologue_us": {q: round(float(np.percentile(md - st, q)), 2) for q in (5, 50, 95)},
        "mean_prologue_us": round(float((md - st).mean()), 3),
        "mean_to_tile_row_us": round(float((t_ty - st).mean()), 3) if b[:, 0].any() else None,
        "mean_to_cone_us": round(float((t_cone - st).mean()), 3) if b[:, 0].any() else None,
        "sum_dur_us_per_slot": round(float(dur.sum()) / (256 * 4 * 5), 2),
        "last_start_us": round(float(st.max()), 2),
        "p99_end_us": round(float(np.percentile(en, 99)), 2),
        "concurrency_over_time": conc,
        "xcc_counts": np.bincount(xcc, minlength=8).tolist(),
        "xcc_last_end_us": [round(float(en[xcc == k].max()), 2) if (xcc == k).any() else None for k in range(8)],
        "distinct_cu": int(len(set(zip(xcc.tolist(), se.tolist(), cu.tolist())))),
        "simd_counts": np.bincount(simd, minlength=4).tolist(),
    }
    # Attribution of the launch (r05): every wave slot over the span is either inside a wave phase or idle
    # (ramp: before the resident count first reaches 95% of its maximum; drain: after it last falls below; gaps).
    if b[:, 2].any():
        span = float(en.max())
        dt = 0.02
        tg = np.arange(0.0, span + dt, dt)
        ev_t = np.concatenate([st, en])
        ev_d = np.concatenate([np.ones_like(st), -np.ones_like(en)])
        o = np.argsort(ev_t, kind="stable")
        cum = np.cumsum(ev_d[o])
        conc_f = cum[np.searchsorted(ev_t[o], tg, side="right") - 1].astype(float)
        conc_f[tg < ev_t[o][0]] = 0.0
        cap = float(conc_f.max())
        full = np.nonzero(conc_f >= 0.95 * cap)[0]
        t_full, t_drop = tg[full[0]], tg[full[-1]]
        idle = (cap - conc_f) * dt
        phases = {"to_tile_row": float((t_ty - st).sum()), "tile_row_to_cone": float((t_cone - t_ty).sum()),
                  "cone_to_ray": float((md - t_cone).sum()), "trace": float((t_tr - md).sum()),
                  "stores": float((en - t_tr).sum())}
        att = {k: round(v / cap, 3) for k, v in phases.items()}
        att["idle_ramp"] = round(float(idle[tg < t_full].sum()) / cap, 3)
        att["idle_mid"] = round(float(idle[(tg >= t_full) & (tg <= t_drop)].sum()) / cap, 3)
        att["idle_drain"] = round(float(idle[tg > t_drop].sum()) / cap, 3)
        out["attribution_us"] = att                    # sums to the span: slot-us of each phase / resident maximum
        out["resident_max"] = int(cap)
        out["t_full_us"], out["t_drop_us"] = round(float(t_full), 2), round(float(t_drop), 2)
        out["mean_phase_us"] = {k: round(v / n, 3) for k, v in phases.items()}
        sky = dur <= np.percentile(dur, 50)
        out["trace_us_short_half"] = round(float((t_tr - md)[sky].mean()), 3)
        out["trace_us_long_half"] = round(float((t_tr - md)[~sky].mean()), 3)
    # the same per-phase means by the class of the position's tile (0 tracing, 1 sky, 2 sphere-free, 3 flat)
    tx_n, ty_n = (W + 7) // 8, (H + 7) // 8
    grid = np.zeros((ty_n, tx_n), np.uint8)
    if hasattr(lib, "rt_diag_tile_class_grid") and lib.rt_diag_tile_class_grid(t._ctx, grid.ctypes.data, grid.size) == 0:
        cls = grid[np.minimum(tile_y, ty_n - 1), np.minimum(tile_x, tx_n - 1)]
        out["tile_classes_env"] = os.environ.get("RT_TILE_CLASSES", "")
        flat = np.zeros((ty_n, tx_n), np.uint8)
        if hasattr(lib, "rt_diag_flat_tile_grid") and lib.rt_diag_flat_tile_grid(t._ctx, flat.ctypes.data, flat.size) == 0:
            out["flat_tiles_env"] = os.environ.get("RT_FLAT_TILES", "")
            cls = np.where((cls == 2) & (flat[np.minimum(tile_y, ty_n - 1), np.minimum(tile_x, tx_n - 1)] != 0), 3, cls)
        out["by_class"] = {}
        for name_c, code in (("tracing_other", 0), ("sky", 1), ("sphere_free", 2), ("flat", 3)):
            m = cls == code
            if not m.any():
                continue
            e = {"waves": int(m.sum()), "mean_dur_us": round(float(dur[m].mean()), 3),
                 "sum_dur_us": round(float(dur[m].sum()), 1),
                 "dur_us": {q: round(float(np.percentile(dur[m], q)), 2) for q in (5, 50, 95)},
                 "mean_prologue_us": round(float((md - st)[m].mean()), 3)}
            if b[:, 2].any():
                e["mean_phase_us"] = {"to_tile_row": round(float((t_ty - st)[m].mean()), 3),
                                      "tile_row_to_cone": round(float((t_cone - t_ty)[m].mean()), 3),
                                      "cone_to_ray": round(float((md - t_cone)[m].mean()), 3),
                                      "trace": round(float((t_tr - md)[m].mean()), 3),
                                      "stores": round(float((en - t_tr)[m].mean()), 3)}
            out["by_class"][name_c] = e
    # duration by dispatch row (one wave per tile: rows of tiles_x positions, in the view's dispatch order), or, with
    # runs, by sixteenths of the dispatch positions
    rows = (H + 7) // 8
    if n == nwg:
        d2 = dur.reshape(rows, (W + 7) // 8)
        out["dur_by_tile_row_us"] = [round(float(x), 2) for x in d2.mean(axis=1)[:: max(1, rows // 16)]]
    else:
        out["dur_by_position_16ths_us"] = [round(float(x.mean()), 2) for x in np.array_split(dur, 16)]
    print(json.dumps(out))
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    np.savez(os.path.join(ROOT, "gpurun_out", f"wave_trace_{name}.npz"), start_us=st, end_us=en, hw=hw, mid_us=md,
             ty_us=t_ty, cone_us=t_cone, trace_us=t_tr,
             tiles_x=(W + 7) // 8, tiles_y=(H + 7) // 8, positions=n)


if __name__ == "__main__":
    main()
