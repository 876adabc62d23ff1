"""GPU tests of the runs of sky tiles (rt_render.hpp render_body, rt_plain.hip rt_run_plan_kernel): a cached render of
a calibrated static view sends one wave per run of up to RT_SKY_RUN_MAX adjacent sky tiles, which stores the miss
constants of the whole run.  Every frame equals the oracle bit for bit and the frame of a twin context created under
RT_SKY_RUN_MAX=1 (the plain table) byte for byte; the output buffers are filled with a sentinel before every render (the
run constants are zeros: a recycled buffer would hide a tile no wave wrote); and rt_diag_disp_count shows that the
cached renders really launched the host plan's positions, fewer than the tiles."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402

from oracle import pyoracle as po  # noqa: E402

from . import sky_common as sk  # noqa: E402
from .sky_runs_common import disp_count, plan  # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("rgba32f", "rgba8", "rgb64f", "raycount")
SENTINEL = 0xA5
DEPTH = {"c2": 1, "c5": 3, "noboard": 1}
PARITY = [("c2", 321, 203), ("c2", 64, 40), ("c5", 321, 203), ("c5", 64, 40), ("noboard", 320, 184)]


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _tracer(**kv):
    """A context created under the given knobs (rt_ctx_create reads them)."""
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    with _env(**kv):
        return Tracer(0)


def _default_run_max():
    """The run maximum of a context created with the environment as it is (the library's default: 16)."""
    return int(os.environ.get("RT_SKY_RUN_MAX", "16")) or 65535


@pytest.fixture(scope="module")
def pair():
    """(on, off): a context with runs and its RT_SKY_RUN_MAX=1 twin."""
    on, off = _tracer(), _tracer(RT_SKY_RUN_MAX=1)
    yield on, off
    on.close()
    off.close()


@functools.lru_cache(maxsize=None)
def _oracle(name, W, H, eye=None, rows_key=None):
    rows = scenes.rows(*rows_key) if rows_key else None
    return po.render(sk.scene_named(name).to_abi(), sk.camera(W, H, eye), W, H, DEPTH[name], rows)


def _fill(t):
    t.view(torch.uint8).fill_(SENTINEL)


def _render(t, cam, W, H, depth, rows=None, stream=None):
    """One render into fresh buffers filled with the sentinel (on the render's stream)."""
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        bufs = t.alloc(W, H, rows, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
        for k in OUTS:
            _fill(bufs[k])
    return t.render_into(cam, W, H, depth, bufs, rows, stream)


def _render_both(pair, cam, W, H, depth, rows=None):
    a, b = (_render(t, cam, W, H, depth, rows) for t in pair)
    torch.cuda.synchronize()
    return a, b


def _check(a, b, want, what):
    rgb, rc = want
    assert np.array_equal(a["rgb64f"].cpu().numpy(), rgb, equal_nan=True), what
    assert np.array_equal(a["raycount"].cpu().numpy().view(np.uint32), rc), what
    for k in OUTS:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs from the RT_SKY_RUN_MAX=1 twin"


def _static_view(pair, name, W, H, R, rows_key=None, cached=3):
    """First render, calibration, `cached` cached renders of the canonical view on both contexts, each checked; then
    the counts: the context with runs launched the host plan's positions, its twin one per tile."""
    sc = sk.scene_named(name)
    for t in pair:
        t.set_scene(sc)
    rows = scenes.rows(*rows_key) if rows_key else None
    cam = sk.camera(W, H)
    want = _oracle(name, W, H, None, rows_key)
    for what in ["first", "calibration"] + [f"cached {k}" for k in range(cached)]:
        a, b = _render_both(pair, cam, W, H, DEPTH[name], rows)
        _check(a, b, want, f"{name} {W}x{H} R={R} {what}")
    host = sk.host_verdict(sc.to_abi(), cam, W, H, rows)
    positions = plan(host, R)[1]
    assert positions < host.size
    assert disp_count(pair[0]) == (positions, host.size, R)
    assert disp_count(pair[1]) == (host.size, host.size, 1)
    return cam, want


@pytest.mark.parametrize("name,W,H", PARITY, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in PARITY])
def test_static_view_equals_oracle_and_twin(pair, name, W, H):
    _static_view(pair, name, W, H, _default_run_max())


@pytest.mark.parametrize("R", [4, 64])
@pytest.mark.parametrize("name,W,H", PARITY, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in PARITY])
def test_run_lengths(pair, name, W, H, R):
    """R = 4, and R = 64: longer than a tile row at 64x40 (8 tiles)."""
    on = _tracer(RT_SKY_RUN_MAX=R)
    try:
        _static_view((on, pair[1]), name, W, H, R, cached=2)
    finally:
        on.close()


def test_whole_streaks(pair):
    """RT_SKY_RUN_MAX=0: a streak of sky tiles is one run however long."""
    on = _tracer(RT_SKY_RUN_MAX=0)
    try:
        _static_view((on, pair[1]), "c2", 321, 203, 65535, cached=2)
    finally:
        on.close()


def test_mixed_sequence(pair):
    """Cached, two renders of a moving camera (verdicts computed per wave, one position per tile), cached again."""
    name, W, H = "c2", 321, 203
    cam, want = _static_view(pair, name, W, H, _default_run_max(), cached=1)
    eyes = sk.orbit_eyes()
    for k in (3, 11):
        a, b = _render_both(pair, sk.camera(W, H, eyes[k]), W, H, DEPTH[name])
        _check(a, b, _oracle(name, W, H, eyes[k]), f"moving {k}")
    for k in range(2):
        a, b = _render_both(pair, cam, W, H, DEPTH[name])
        _check(a, b, want, f"cached again {k}")
    assert disp_count(pair[0])[0] < disp_count(pair[0])[1]


def test_moving_order_reads_the_plain_table(pair):
    """RT_MOVING_ORDER=1: a render of another camera reuses the calibrated view's dispatch order — the plain table's,
    in which every tile has a position — and computes its own verdicts."""
    name, W, H = "c2", 321, 203
    on = _tracer(RT_MOVING_ORDER=1)
    try:
        both = (on, pair[1])
        cam, want = _static_view(both, name, W, H, _default_run_max(), cached=1)
        eyes = sk.orbit_eyes()
        for k in (5, 13):
            a, b = _render_both(both, sk.camera(W, H, eyes[k]), W, H, DEPTH[name])
            _check(a, b, _oracle(name, W, H, eyes[k]), f"RT_MOVING_ORDER=1, eye {k}")
        a, b = _render_both(both, cam, W, H, DEPTH[name])
        _check(a, b, want, "cached again")
    finally:
        on.close()


@pytest.mark.parametrize("name", ["c2", "c5"])
def test_packed_gray8(pair, name):
    """The packed instances: GRAY8 frames (first, calibration, cached) equal the R channel of the twin's RGBA8."""
    W, H = 321, 203
    sc = sk.scene_named(name)
    for t in pair:
        t.set_scene(sc)
    cam = sk.camera(W, H)
    ref = _render(pair[1], cam, W, H, DEPTH[name])["rgba8"][..., :1].clone()
    st = torch.cuda.current_stream()
    for k in range(4):
        g = torch.empty((H, W, 1), dtype=torch.uint8, device="cuda")
        _fill(g)
        abi.check(abi.lib().rt_render_dev_packed(pair[0]._ctx, ctypes.byref(cam), W, H, DEPTH[name], None,
                                                 abi.RT_PIXEL_RGBA32F, None, abi.RT_PIXEL_GRAY8,
                                                 ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(st.cuda_stream)),
                  "rt_render_dev_packed")
        torch.cuda.synchronize()
        assert torch.equal(g, ref), f"GRAY8 render {k}"
    positions, tiles, _ = disp_count(pair[0])
    assert positions == plan(sk.host_verdict(sc.to_abi(), cam, W, H), _default_run_max())[1] < tiles


@pytest.mark.parametrize("rank", [0, 1])
def test_banded_rows(pair, rank):
    """A rank's rows of a two-rank frame, bands of 8 rows."""
    _static_view(pair, "c2", 320, 184, _default_run_max(), rows_key=(8, 2, rank), cached=2)


def test_supersampled_view_keeps_the_plain_table(pair):
    """A supersampled render whose sample grid has the calibrated size: its epilogue reduces over the wave, so its view
    never reads runs.  First, calibration and two cached renders equal the twin's."""
    name, W, H, S = "c2", 160, 92, 2
    _static_view(pair, name, W * S, H * S, _default_run_max(), cached=1)
    cam = sk.camera(W, H)
    for k in range(4):
        out = []
        for t in pair:
            bufs = t.alloc_ss(W, H, None, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
            for key in OUTS:
                _fill(bufs[key])
            out.append(t.render_ss_into(cam, W, H, DEPTH[name], S, bufs))
        torch.cuda.synchronize()
        for key in OUTS:
            assert torch.equal(out[0][key], out[1][key]), f"supersampled render {k}: {key}"
        assert not (out[0]["rgba8"] == SENTINEL).all(dim=-1).any(), "a pixel no wave wrote"
    positions, tiles, run_max = disp_count(pair[0])
    assert (positions, run_max) == (tiles, 1)


def test_two_streams(pair):
    """One context rendered alternately on two streams (the group's pattern): 6 frames of one static view, every frame
    equal to the first and to the oracle."""
    name, W, H = "c2", 321, 203
    on = pair[0]
    on.set_scene(sk.scene_named(name))
    cam = sk.camera(W, H)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    frames = [_render(on, cam, W, H, DEPTH[name], stream=streams[k % 2]) for k in range(6)]
    torch.cuda.synchronize()
    rgb, rc = _oracle(name, W, H)
    assert np.array_equal(frames[0]["rgb64f"].cpu().numpy(), rgb, equal_nan=True)
    assert np.array_equal(frames[0]["raycount"].cpu().numpy().view(np.uint32), rc)
    for k, f in enumerate(frames[1:], 1):
        for key in OUTS:
            assert torch.equal(f[key], frames[0][key]), f"frame {k}: {key}"
    positions, tiles, _ = disp_count(on)
    assert positions == plan(sk.host_verdict(sk.scene_named(name).to_abi(), cam, W, H), _default_run_max())[1] < tiles
