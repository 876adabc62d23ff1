"""GPU tests of the tile classes (rt_render.hpp render_body, rt_plain.hip rt_class_kernel): the calibration of a static
view of a fast-kernel scene marks the tracing tiles whose cone mask and level masks keep no sphere, and the cached
renders trace those tiles without the sphere code.  Every frame equals the oracle bit for bit and the frame of a twin
context created under RT_TILE_CLASSES=0 byte for byte, with the output buffers filled with a sentinel before every
render; every tile the class grid marks is sphere-free in the oracle, ray by ray and level by level; and the class really
occurs beside tracing tiles outside it, so both paths ran.

Sphere-free tiles the calibration reported on an MI355X, against the exact counts of tiles with no sphere involvement
(EXACT below, which bound them from above): c2 321x203 80 of 170, c2 320x184 74 of 161, c3 321x203 44 of 122, c2 64x40
1 of 3, noboard 320x184 0 of 0 (profiles/tileclass/README.md)."""
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
from .tile_classes_common import SKY, SPHERE_FREE, TRACE, class_counts, class_grid, tiles_any  # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("rgba32f", "rgba8", "rgb64f", "raycount")
SENTINEL = 0xA5
DEPTH = {"c2": 1, "c3": 2, "noboard": 1, "rise": 1}
PARITY = [("c2", 321, 203), ("c2", 64, 40), ("c3", 321, 203), ("noboard", 320, 184)]
# tiles in which no primary, reflected or shadow ray of any pixel touches a sphere (the oracle, on the CPU), of the
# tracing tiles: the kernel's conservative masks classify at most these
EXACT = {("c2", 321, 203): (170, 406), ("c2", 320, 184): (161, 396), ("c3", 321, 203): (122, 406),
         ("c2", 64, 40): (3, 22), ("noboard", 320, 184): (0, None)}
MUST_OCCUR = {("c2", 321, 203), ("c2", 320, 184), ("c3", 321, 203)}


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
    """(on, off): a context with tile classes and its RT_TILE_CLASSES=0 twin."""
    on, off = _tracer(RT_TILE_CLASSES=1), _tracer(RT_TILE_CLASSES=0)
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
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs from the RT_TILE_CLASSES=0 twin"


def _check_counts(on, name, W, H, rows=None):
    """The classes the calibration decided, against the exact counts: -> the class grid."""
    nl = scenes.local_rows(H, rows)
    ty, tx = (nl + 7) // 8, (W + 7) // 8
    tiles, sky, free = class_counts(on)
    grid = class_grid(on, ty, tx)
    assert tiles == ty * tx and sky == int((grid == SKY).sum()) and free == int((grid == SPHERE_FREE).sum())
    print(f"tile classes {name} {W}x{H} rows={rows is not None}: {tiles} tiles, {sky} sky, {free} sphere-free, "
          f"{tiles - sky - free} other tracing tiles")
    key = (name, W, H)
    if key in EXACT and rows is None:
        exact = EXACT[key][0]
        assert free <= exact, f"{key}: {free} sphere-free tiles, but only {exact} are exactly sphere-free"
    if key in MUST_OCCUR:
        assert free >= 1, f"{key}: the class does not occur"
    assert (grid == TRACE).any(), f"{key}: every tracing tile is in the class: the general path never ran"
    return grid


def _static_view(pair, name, W, H, rows_key=None, cached=3):
    """First render, calibration, `cached` cached renders of the canonical view on both contexts, each checked against
    the oracle and the twin; then the class counts."""
    sc = sk.scene_named(name)
    for t in pair:
        t.set_scene(sc)
    rows = scenes.rows(*rows_key) if rows_key else None
    cam = sk.camera(W, H)
    want = _oracle(name, W, H, None, rows_key)
    for what in ["first", "calibration"] + [f"cached {k}" for k in range(cached)]:
        a, b = _render_both(pair, cam, W, H, DEPTH[name], rows)
        _check(a, b, want, f"{name} {W}x{H} {what}")
    grid = _check_counts(pair[0], name, W, H, rows)
    return cam, want, grid


@pytest.mark.parametrize("name,W,H", PARITY, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in PARITY])
def test_static_view_equals_oracle_and_twin(pair, name, W, H):
    _static_view(pair, name, W, H)


def _touched_tiles(name, W, H):
    """bool [tile rows, tiles_x]: some pixel of the tile has a primary, reflected or shadow ray, level by level up to the
    depth, that hits a sphere in po.intersect — tested on the scene without its board, so a sphere counts wherever it
    lies along the ray (the masks are geometric: they know nothing of the board in front)."""
    sc = sk.scene_named(name)
    full = sc.to_abi()
    bare_sc = sk.scene_named(name)
    bare_sc.has_board = False
    bare = bare_sc.to_abi()
    cam = sk.camera(W, H)
    lights = [np.array(lt.position(), np.float64) for lt in sc.lights]
    ends = po.screen_points(cam, W, H).reshape(-1, 3)
    starts = np.broadcast_to(np.array(cam.eye[:], np.float64), ends.shape).copy()
    pix = np.arange(W * H)
    touched = np.zeros(W * H, bool)
    for lvl in range(DEPTH[name] + 1):
        if pix.size == 0:
            break
        touched[pix[po.intersect(bare, starts, ends)["hit"] != 0]] = True
        h = po.intersect(full, starts, ends)
        hit = h["hit"] != 0
        pix, p, nxt = pix[hit], h["point"][hit], h["reflected_end"][hit]
        for L in lights:
            if pix.size:
                blocked = po.intersect(bare, p, np.broadcast_to(L, p.shape).copy())["hit"] != 0
                touched[pix[blocked]] = True
        starts, ends = p, nxt
    return tiles_any(touched.reshape(H, W))


@pytest.mark.parametrize("name,W,H", [("c2", 321, 203), ("c3", 321, 203), ("c2", 64, 40)],
                         ids=["c2-321x203", "c3-321x203", "c2-64x40"])
def test_marked_tiles_are_sphere_free_in_the_oracle(pair, name, W, H):
    on = pair[0]
    on.set_scene(sk.scene_named(name))
    cam = sk.camera(W, H)
    for _ in range(3):
        _render(on, cam, W, H, DEPTH[name])
    torch.cuda.synchronize()
    grid = _check_counts(on, name, W, H)
    touched = _touched_tiles(name, W, H)
    bad = np.argwhere((grid == SPHERE_FREE) & touched)
    assert bad.size == 0, f"{name} {W}x{H}: tiles marked sphere-free whose rays hit a sphere: {bad[:8].tolist()}"
    exact = int((~touched & (grid != SKY)).sum())
    print(f"{name} {W}x{H}: {int((grid == SPHERE_FREE).sum())} marked, {exact} tracing tiles untouched in the oracle")


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_packed_gray8(pair, name):
    """The packed instances: GRAY8 frames (first, calibration, cached) equal the R channel of the twin's RGBA8.  (At
    depth 2 the packed instances do not read the class bit, so their views' records must not carry it.)"""
    W, H = 321, 203
    sc = sk.scene_named(name)
    for t in pair:
        t.set_scene(sc)
    cam = sk.camera(W, H)
    ref = _render(pair[1], cam, W, H, DEPTH[name])["rgba8"][..., :1].clone()
    st = torch.cuda.current_stream()
    for k in range(5):
        g = torch.empty((H, W, 1), dtype=torch.uint8, device="cuda")
        _fill(g)
        abi.check(abi.lib().rt_render_dev_packed(pair[0]._ctx, ctypes.byref(cam), W, H, DEPTH[name], None,
                                                 abi.RT_PIXEL_RGBA32F, None, abi.RT_PIXEL_GRAY8,
                                                 ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(st.cuda_stream)),
                  "rt_render_dev_packed")
        torch.cuda.synchronize()
        assert torch.equal(g, ref), f"GRAY8 render {k}"
    assert class_counts(pair[0])[2] >= 1


@pytest.mark.parametrize("rank", [0, 1])
def test_banded_rows(pair, rank):
    """A rank's rows of a two-rank frame, bands of 8 rows."""
    _, _, grid = _static_view(pair, "c2", 320, 184, rows_key=(8, 2, rank), cached=2)
    assert (grid == SPHERE_FREE).any()


def test_supersampled_view(pair):
    """A supersampled render whose sample grid has the calibrated size: the supersampled instances do not read the class
    bit, so their view's records must not carry it.  First, calibration and two cached renders equal the twin's."""
    name, W, H, S = "c2", 160, 92, 2
    _static_view(pair, name, W * S, H * S, cached=1)
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


def test_full_frame_320x184(pair):
    _static_view(pair, "c2", 320, 184, cached=1)


def test_two_streams(pair):
    """One context rendered alternately on two streams: 6 frames of one static view, every frame equal to the oracle and
    to the twin's."""
    name, W, H = "c2", 321, 203
    on, off = pair
    for t in pair:
        t.set_scene(sk.scene_named(name))
    cam = sk.camera(W, H)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    frames = [_render(on, cam, W, H, DEPTH[name], stream=streams[k % 2]) for k in range(6)]
    twin = _render(off, cam, W, H, DEPTH[name])
    torch.cuda.synchronize()
    for k, f in enumerate(frames):
        _check(f, twin, _oracle(name, W, H), f"two streams, frame {k}")
    assert class_counts(on)[2] >= 1


def test_mixed_sequence(pair):
    """Cached renders, two renders of a moving camera (no class: their records are not this view's), cached again."""
    name, W, H = "c2", 321, 203
    cam, want, _ = _static_view(pair, name, W, H, cached=2)
    eyes = sk.orbit_eyes()
    for k in (3, 11):
        a, b = _render_both(pair, sk.camera(W, H, eyes[k]), W, H, DEPTH[name])
        _check(a, b, _oracle(name, W, H, eyes[k]), f"moving {k}")
    for k in range(3):
        a, b = _render_both(pair, cam, W, H, DEPTH[name])
        _check(a, b, want, f"cached again {k}")


def test_scene_change_on_a_calibrated_context(pair):
    """c2 calibrated, then c2 with sphere 3 replaced by one that rises against the sky, same camera: the new sphere's
    tiles must not inherit the old view's class."""
    W, H = 321, 203
    _static_view(pair, "c2", W, H, cached=1)
    cam, _, grid = _static_view(pair, "rise", W, H, cached=2)
    assert (grid == SPHERE_FREE).any()
    _static_view(pair, "c2", W, H, cached=1)
