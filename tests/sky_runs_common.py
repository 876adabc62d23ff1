"""Shared by the sky-run tests (test_sky_runs.py on the CPU, test_gpu_sky_runs.py on the GPU): the host's run plan
(rt_diag_sky_run_plan) and what a context's last cached render launched (rt_diag_disp_count)."""
import ctypes

import numpy as np

from ray_tracer_fragment_shader_amd import abi


def plan(sky, R):
    """rt_diag_sky_run_plan of the verdict grid `sky` [tile rows, tiles_x] -> (run int32 [tile rows, tiles_x]: 0 a
    tracing tile, len the head of a run, -1 a run's other tiles; the dispatch positions)."""
    sky = np.ascontiguousarray(sky, np.uint8)
    ty, tx = sky.shape
    run = np.full((ty, tx), -7, np.int32)
    n = ctypes.c_int(-1)
    abi.check(abi.lib().rt_diag_sky_run_plan(sky.ctypes.data, tx, ty, R, run.ctypes.data, ctypes.byref(n)),
              "rt_diag_sky_run_plan")
    return run, n.value


def disp_count(tracer):
    """rt_diag_disp_count -> (positions, tiles, run_max) of the context's last cached render."""
    p, t, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    abi.check(abi.lib().rt_diag_disp_count(tracer._ctx, ctypes.byref(p), ctypes.byref(t), ctypes.byref(r)),
              "rt_diag_disp_count")
    return p.value, t.value, r.value
