"""GPU test of bench.py's plain run: the lean line and `--dump-outputs` (the last timed step's buffers)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_tracer_fragment_shader_amd import scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_the_timed_frame(tmp_path):
    """One plain c1 run (640x480, the smallest config): the line carries the headline keys and none of the --full
    legs, `--steps` is the timed step count, and the dumped buffers are the frame rt_render_dev renders, whole, in
    float32."""
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--steps", "4",
                        "--warmup", "2", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 4 and res["warmup"] == 2 and res["n_gpus"] == 1 and res["full"] is False
    assert res["unit"] == "Mray/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region: rays per step / time per step (ms_per_step is printed
    # to 4 decimals, so it is within 5e-5 ms of the time `value` was divided by; value itself to 3 decimals)
    want = scenes.PINNED_RAYS["c1"] / (res["ms_per_step"] * 1e-3) / 1e6
    assert abs(res["value"] - want) <= want * 5.1e-5 / (res["ms_per_step"] - 5e-5) + 1e-3
    for leg in ("c4", "configs", "drop_in", "cpu_baseline"):
        assert leg not in res, f"{leg} belongs to --full"
    assert res["roofline"]["kernel_ms_serial"] is None

    cfg = scenes.CONFIGS["c1"]
    W, H = cfg.width, cfg.height
    assert res["dump_outputs"]["pixels"] == res["dump_outputs"]["of_pixels"] == W * H
    assert sorted(os.listdir(d)) == ["rgba32f.npy", "rgba8.npy"]
    got32, got8 = np.load(d / "rgba32f.npy"), np.load(d / "rgba8.npy")
    assert got32.dtype == got8.dtype == np.float32 and got32.shape == got8.shape == (H, W, 4)
    assert got32.nbytes + got8.nbytes <= 64_000_000
    tr = Tracer(0)
    tr.set_scene(cfg.scene())
    b = tr.render(cfg.camera(), W, H, cfg.depth, rgba32f=True, rgba8=True)
    torch.cuda.synchronize()
    assert np.array_equal(got32, b["rgba32f"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(got8, b["rgba8"].cpu().numpy().astype(np.float32))
    tr.close()
