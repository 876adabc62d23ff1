#!/usr/bin/env python3
"""Small frames through every kind of render launch, for a kernel trace: which kernels a build launches, in order.

usage: route_probe.py [build]      build: a name under tools/_ab/ (tools/build_rev.sh), default the in-tree library

64 x 48 frames through the public Tracer calls — plain RGBA with all four outputs, a packed byte image (GRAY8 for an
achromatic scene, else RGB8) and render_ss with S = 2 — three renders of the same view each, so the first render, the
calibration render (with the level-mask launch and the dispatch-table kernels behind it) and a render in calibrated
order all occur; then c2 and c5 plain again under each A/B knob, one fresh Tracer per setting.  Prints one label per
step and nothing else.  Run under `rocprofv3 --kernel-trace` once per build and compare the ordered kernel names with
their grid and workgroup sizes (profiles/route/): a refactor of the launch code must leave them as they were.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) > 1 and sys.argv[1] != "base":
    os.environ["RT_LIB_PATH"] = os.path.join(ROOT, "tools", "_ab", sys.argv[1], "librt_amd.so")

import torch  # noqa: E402

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402

W, H = 64, 48


def scene68():
    """c5's 64 spheres and four more above them: the culling kernels' general stride."""
    sc = scenes.CONFIGS["c5"].scene()
    sc.spheres += [scenes.SphereSpec(sq, 10.0, 100.0) for sq in ("a1", "c3", "e5", "g7")]
    return sc


def achromatic(scene):
    out = ctypes.c_int()
    sa = scene.to_abi()
    abi.check(abi.lib().rt_scene_achromatic(ctypes.byref(sa), ctypes.byref(out)), "rt_scene_achromatic")
    return bool(out.value)


def plain(tr, cam, depth):
    bufs = tr.alloc(W, H, None, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    for _ in range(3):
        tr.render_into(cam, W, H, depth, bufs)
    torch.cuda.synchronize()


def main():
    c2, c5 = scenes.CONFIGS["c2"], scenes.CONFIGS["c5"]
    cam = c2.camera(W, H)
    cases = [("c2", c2.scene(), (1, 3, 4)), ("c5", c5.scene(), (2, 3, 5)), ("s68", scene68(), (3,)),
             ("demo", scenes.CONFIGS["demo"].scene(), (5,)), ("tree_demo", scenes.tree_case("tree_demo")[0], (5,))]
    tr = Tracer(0)
    for name, scene, depths in cases:
        tr.set_scene(scene)
        byte_format = abi.RT_PIXEL_GRAY8 if achromatic(scene) else abi.RT_PIXEL_RGB8
        for depth in depths:
            print(f"{name} depth {depth} plain", flush=True)
            plain(tr, cam, depth)
            print(f"{name} depth {depth} packed", flush=True)
            for _ in range(3):
                tr.render_packed(cam, W, H, depth, None, byte_format)
            torch.cuda.synchronize()
            print(f"{name} depth {depth} ss", flush=True)
            bufs = tr.alloc_ss(W, H, None, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
            for _ in range(3):
                tr.render_ss_into(cam, W, H, depth, 2, bufs)
            torch.cuda.synchronize()
    tr.close()
    for env in ("RT_SCENE_IN_LDS=1", "RT_WG_STAGING=1", "RT_MIN_WAVES=0", "RT_ACHRO_OFF=1"):
        var, value = env.split("=")
        os.environ[var] = value                   # read when the context is created
        for name, scene, depths in cases[:2]:
            t = Tracer(0)
            t.set_scene(scene)
            for depth in depths:
                print(f"{name} depth {depth} plain {env}", flush=True)
                plain(t, cam, depth)
            t.close()
        os.environ.pop(var)


if __name__ == "__main__":
    main()
