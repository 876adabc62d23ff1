"""GPU tests of the flat tiles (rt_device.hpp trace_flat, rt_plain.hip rt_flat_kernel): the calibration of a static view
of a fast-kernel scene marks the sphere-free tiles all of whose 64 primary rays hit the board, and the cached renders
trace those tiles on the straight-line path.  Every frame equals the oracle bit for bit and the frame of a twin context
created under RT_FLAT_TILES=0 byte for byte in all four outputs, with the output buffers filled with a sentinel before
every render.  The verdict is exact: the flat grid equals (sphere-free in the class grid) and (all 64 lanes hit the board
in the oracle) and (the wave-uniform gates); and every flat tile is flat in the oracle — lit by every light, no reflected
hit (at depth 0, where no reflected ray is traced and no level mask speaks of one: lit by every light).

Flat tiles the calibration reported on an MI355X: c2 321x203 36 of 80 sphere-free tiles (the oracle has 215 all-board
tiles, 116 of them flat), the `rise` scene 37 of 81 (profiles/flat/README.md has the other shapes).

Cases: c2 at depth 1 and depth 0, c3 at depth 2, the board-less scene, the `rise` scene; shapes 321x203, 320x184, 64x40.

The gates.  The board's origin-skip limit of these scenes is |eye.y| <= 1,876,499.5 (rt_host.cpp board_skip_y, recomputed
in _board_skip_y); an eye at twice that height still sees 517 all-board tiles at 321x203 (the oracle), so a finite camera
reaches the gate and it is tested on the device.  hits_ok, the bounding-sphere shortcut of rays from hit points, goes off
only for eyes much farther away than that (rt_host.cpp hits_limit: about 1e8 for scenes of this size), beyond the
origin-skip gate: a view with hits_ok off is tested at eye.y = 1e10, where no tile may be flat."""
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

from . import flat_tiles_common as fc  # noqa: E402
from . import sky_common as sk  # noqa: E402
from .tile_classes_common import SPHERE_FREE, TRACE, class_grid  # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("rgba32f", "rgba8", "rgb64f", "raycount")
SENTINEL = 0xA5
CASES = {"c2": ("c2", 1), "c2d0": ("c2", 0), "c3": ("c3", 2), "noboard": ("noboard", 1), "rise": ("rise", 1)}
SHAPES = [(321, 203), (320, 184), (64, 40)]
PARITY = [(c, W, H) for c in CASES for (W, H) in SHAPES]
MUST_OCCUR = {(c, W, H) for c in ("c2", "c2d0", "c3") for (W, H) in SHAPES[:2]}
MUST_NOT_OCCUR = {("c2", 64, 40), ("c2d0", 64, 40)} | {("noboard", W, H) for (W, H) in SHAPES}


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


@pytest.fixture(scope="module")
def pair():
    """(on, off): a context with flat tiles and its RT_FLAT_TILES=0 twin."""
    on, off = _tracer(RT_FLAT_TILES=1), _tracer(RT_FLAT_TILES=0)
    yield on, off
    on.close()
    off.close()


@functools.lru_cache(maxsize=None)
def _oracle(case, W, H, eye=None, rows_key=None):
    name, depth = CASES[case]
    rows = scenes.rows(*rows_key) if rows_key else None
    return po.render(sk.scene_named(name).to_abi(), sk.camera(W, H, eye), W, H, depth, rows)


def _board_skip_y(name):
    """rt_host.cpp's board_skip_y of the scene (board normal (0, -1, 0))."""
    sc = sk.scene_named(name).to_abi()
    eps2 = sc.small_number * sc.small_number
    return (eps2 / 2 / 2.0 ** -50 - 5 * abs(sk.board_y(sc)) - 1) / 3


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
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs from the RT_FLAT_TILES=0 twin"


def _check_grids(pair, case, W, H, eye=None, rows_key=None):
    """The verdicts of both contexts' last calibration against the class grid and the oracle: -> (flat, class grid)."""
    name, depth = CASES[case]
    rows = scenes.rows(*rows_key) if rows_key else None
    nl = scenes.local_rows(H, rows)
    ty, tx = (nl + 7) // 8, (W + 7) // 8
    truth = fc.oracle_truth(name, W, H, eye, rows_key)
    # the wave-uniform gates (flat_gates): the board, and the eye inside the board's origin-skip limit
    eye_y = sk.camera(W, H, eye).eye[1]
    gates = bool(sk.scene_named(name).has_board) and abs(eye_y) <= _board_skip_y(name)
    # at depth 0 no reflected ray is traced (and no level mask speaks of one): lit by every light is all there is
    truth_flat = truth["flat"] if depth >= 1 else truth["lit"]
    out = None
    for t in pair:                                          # (the twin decides the same verdicts: it only leaves them
        tiles, n = fc.flat_counts(t)                        # out of its records)
        flat, cls = fc.flat_grid(t, ty, tx), class_grid(t, ty, tx)
        assert tiles == ty * tx and n == int(flat.sum())
        assert np.array_equal(flat, (cls == SPHERE_FREE) & truth["board"] & gates), \
            f"{case} {W}x{H}: the flat grid is not (sphere-free) & (all 64 lanes hit the board in the oracle) & gates"
        bad = np.argwhere(flat & ~truth_flat)
        assert bad.size == 0, f"{case} {W}x{H}: flat tiles that are shadowed or reflect something: {bad[:8].tolist()}"
        out = out or (flat, cls)
    flat, cls = out
    print(f"flat tiles {case} {W}x{H} rows={rows_key} eye={eye}: {int(flat.sum())} flat of "
          f"{int((cls == SPHERE_FREE).sum())} sphere-free, {int((cls == TRACE).sum())} other tracing tiles; the oracle: "
          f"{int(truth['flat'].sum())} flat, {int(truth['board'].sum())} all-board")
    return flat, cls


def _static_view(pair, case, W, H, eye=None, rows_key=None, cached=2):
    """First render, calibration, `cached` cached renders of the view on both contexts, each checked against the oracle
    and the twin; then the verdicts."""
    name, depth = CASES[case]
    for t in pair:
        t.set_scene(sk.scene_named(name))
    rows = scenes.rows(*rows_key) if rows_key else None
    cam = sk.camera(W, H, eye)
    want = _oracle(case, W, H, eye, rows_key)
    for what in ["first", "calibration"] + [f"cached {k}" for k in range(cached)]:
        a, b = _render_both(pair, cam, W, H, depth, rows)
        _check(a, b, want, f"{case} {W}x{H} {what}")
    flat, cls = _check_grids(pair, case, W, H, eye, rows_key)
    return cam, want, flat, cls


@pytest.mark.parametrize("case,W,H", PARITY, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in PARITY])
def test_static_view_equals_oracle_and_twin(pair, case, W, H):
    """Parity, the exact class, the subset of the oracle, and that both paths ran."""
    _, _, flat, cls = _static_view(pair, case, W, H)
    key = (case, W, H)
    if key in MUST_OCCUR:
        assert flat.any(), f"{key}: the class does not occur"
        assert ((cls == SPHERE_FREE) & ~flat).any() and (cls == TRACE).any(), f"{key}: only the flat path ran"
    if key in MUST_NOT_OCCUR:
        assert not flat.any(), f"{key}: the class occurs"
    if key in {("c2", 64, 40), ("c2d0", 64, 40)}:
        assert (cls == SPHERE_FREE).any(), f"{key}: no sphere-free tile beside which the class could be missing"


def test_packed_gray8(pair):
    """The packed depth-1 instance reads the bit: GRAY8 frames (first, calibration, cached) equal the oracle's R channel
    as bytes (floor(clamp(c, 0, 1) * 255 + 0.5), the RGBA8 definition) and the R channel of the twin's RGBA8."""
    case, W, H = "c2", 321, 203
    name, depth = CASES[case]
    for t in pair:
        t.set_scene(sk.scene_named(name))
    cam = sk.camera(W, H)
    ref = _render(pair[1], cam, W, H, depth)["rgba8"][..., :1].clone()
    want = np.floor(np.clip(_oracle(case, W, H)[0][..., :1], 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    st = torch.cuda.current_stream()
    for k in range(5):
        g = torch.empty((H, W, 1), dtype=torch.uint8, device="cuda")
        _fill(g)
        abi.check(abi.lib().rt_render_dev_packed(pair[0]._ctx, ctypes.byref(cam), W, H, depth, None,
                                                 abi.RT_PIXEL_RGBA32F, None, abi.RT_PIXEL_GRAY8,
                                                 ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(st.cuda_stream)),
                  "rt_render_dev_packed")
        torch.cuda.synchronize()
        assert np.array_equal(g.cpu().numpy(), want), f"GRAY8 render {k} against the oracle"
        assert torch.equal(g, ref), f"GRAY8 render {k}"
    assert fc.flat_counts(pair[0])[1] >= 1


@pytest.mark.parametrize("rank", [0, 1])
def test_banded_rows(pair, rank):
    """A rank's rows of a two-rank frame, bands of 8 rows."""
    _, _, flat, _ = _static_view(pair, "c2", 320, 184, rows_key=(8, 2, rank))
    assert flat.any()


def test_two_streams(pair):
    """One context rendered alternately on two streams: 6 frames of one static view, every frame equal to the oracle and
    to the twin's."""
    case, W, H = "c2", 321, 203
    name, depth = CASES[case]
    on, off = pair
    for t in pair:
        t.set_scene(sk.scene_named(name))
    cam = sk.camera(W, H)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    frames = [_render(on, cam, W, H, depth, stream=streams[k % 2]) for k in range(6)]
    twin = _render(off, cam, W, H, depth)
    torch.cuda.synchronize()
    for k, f in enumerate(frames):
        _check(f, twin, _oracle(case, W, H), f"two streams, frame {k}")
    assert fc.flat_counts(on)[1] >= 1


def test_moved_eye_and_back(pair):
    """Cached renders, two renders of a moved eye (their records are not this view's: no class), cached again."""
    case, W, H = "c2", 321, 203
    cam, want, flat, _ = _static_view(pair, case, W, H)
    assert flat.any()
    eyes = sk.orbit_eyes()
    for k in (3, 11):
        a, b = _render_both(pair, sk.camera(W, H, eyes[k]), W, H, CASES[case][1])
        _check(a, b, _oracle(case, W, H, eyes[k]), f"moved eye {k}")
    for k in range(3):
        a, b = _render_both(pair, cam, W, H, CASES[case][1])
        _check(a, b, want, f"cached again {k}")


def test_scene_swap(pair):
    """c2 calibrated, then the `rise` scene under the same camera, then c2 again: each view gets its own verdicts."""
    W, H = 321, 203
    _static_view(pair, "c2", W, H, cached=1)
    _, _, flat, _ = _static_view(pair, "rise", W, H)
    assert flat.any()
    _static_view(pair, "c2", W, H, cached=1)


def test_supersampled_view_takes_no_class(pair):
    """The supersampled instances read no class bit: their view holds no verdicts, and its frames equal the twin's."""
    case, W, H, S = "c2", 160, 92, 2
    _static_view(pair, case, W * S, H * S, cached=1)
    cam = sk.camera(W, H)
    for k in range(4):
        out = []
        for t in pair:
            bufs = t.alloc_ss(W, H, None, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
            for key in OUTS:
                _fill(bufs[key])
            out.append(t.render_ss_into(cam, W, H, CASES[case][1], S, bufs))
        torch.cuda.synchronize()
        for key in OUTS:
            assert torch.equal(out[0][key], out[1][key]), f"supersampled render {k}: {key}"
        assert not (out[0]["rgba8"] == SENTINEL).all(dim=-1).any(), "a pixel no wave wrote"
    assert fc.flat_counts(pair[0]) == (0, 0)


def test_eye_beyond_the_origin_skip_gate(pair):
    """An eye at twice the board's origin-skip height: all-board tiles exist (and half that height has flat ones), but
    none is flat, and the frames match."""
    case, W, H = "c2", 321, 203
    y = _board_skip_y("c2")
    _, _, flat, cls = _static_view(pair, case, W, H, eye=(0.0, 0.5 * y, 200.0))
    assert flat.any(), "an eye inside the gate, as far away: flat tiles"
    eye = (0.0, 2.0 * y, 200.0)
    _, _, flat, cls = _static_view(pair, case, W, H, eye=eye)
    assert not flat.any()
    assert ((cls == SPHERE_FREE) & fc.oracle_truth("c2", W, H, eye)["board"]).any(), \
        "no sphere-free all-board tile: the gate decided nothing"


def test_eye_without_hits_ok(pair):
    """An eye so far away that the hit points' bounding-sphere shortcut is off.  In these scenes that happens only beyond
    the origin-skip gate (test_flat_tiles.py::test_gates_on_the_host shows both on the host), so what the device can
    show is that such a view has no flat tile and still matches."""
    assert fc.flat_gates("c2", (0.0, 1e10, 200.0))[:2] == (0, 0)
    _, _, flat, _ = _static_view(pair, "c2", 321, 203, eye=(0.0, 1e10, 200.0))
    assert not flat.any()


@pytest.mark.parametrize("eye", [(0.0, -100.0, 200.0), (0.0, -300.0, 100.0)], ids=["y-100", "y-300"])
def test_eye_below_the_board(pair, eye):
    _static_view(pair, "c2", 321, 203, eye=eye)
