"""GPU parity: the HIP path (lib/librt_amd.so through the C ABI) against the reference-generated golden
fixtures and the CPU oracle, on the same inputs.

Tolerance: the north-star bar is L-infinity <= 1e-4 per channel (TOL below).  The kernel keeps the
reference's FP64 operation order (-ffp-contract=off, IEEE div/sqrt), so these tests also require
bit-exact equality; a single flipped hit/shadow/checker decision would show up as an error near 1.
"""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer, decode_hits, unshuffle  # noqa: E402

from . import golden  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
CAM = np.array([0.0, 100.0, 200.0])


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    t = Tracer(0)
    yield t
    t.close()


def _render64(tr, scene, cam, W, H, depth, rows=None):
    tr.set_scene(scene)
    b = tr.render(cam, W, H, depth, rows=rows, rgba32f=False, rgb64f=True, raycount=True)
    torch.cuda.synchronize()
    return b["rgb64f"].cpu().numpy(), b["raycount"].cpu().numpy().view(np.uint32)


def _assert_parity(got, want):
    # NaN appears only where the reference itself yields NaN (total internal reflection -> Line(p, p))
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    fin = ~np.isnan(want)
    err = np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
    assert err <= TOL, f"L-inf {err}"
    assert np.array_equal(got, want, equal_nan=True), \
        f"not bit-exact: {(got != want).any(axis=-1).sum()} pixels differ"


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c5", "demo"])
def test_small_frame_vs_reference(tr, name):
    cfg = scenes.CONFIGS[name]
    g = golden.frames(name)
    W, H = (int(x) for x in g["small_wh"])
    rgb, _ = _render64(tr, cfg.scene(), cfg.camera(W, H), W, H, cfg.depth)
    _assert_parity(rgb, g["small"])


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c5", "demo"])
def test_sampled_full_res_pixels_vs_reference(tr, name):
    cfg = scenes.CONFIGS[name]
    g = golden.frames(name)
    tr.set_scene(cfg.scene())
    sp = po.screen_points(cfg.camera(), cfg.width, cfg.height)[g["pj"], g["pi"]]
    starts = torch.tensor(np.tile(CAM, (len(sp), 1)), device="cuda")
    ends = torch.tensor(np.ascontiguousarray(sp), device="cuda")
    rgb, _ = tr.trace_rays(starts, ends, cfg.depth)
    _assert_parity(rgb.cpu().numpy(), g["samples"])


@pytest.mark.parametrize("name", ["c1", "c2", "demo"])
def test_full_frame_vs_oracle(tr, name):
    cfg = scenes.CONFIGS[name]
    sc = cfg.scene()
    rgb, rc = _render64(tr, sc, cfg.camera(), cfg.width, cfg.height, cfg.depth)
    want, want_rc = po.render(sc.to_abi(), cfg.camera(), cfg.width, cfg.height, cfg.depth)
    _assert_parity(rgb, want)
    assert np.array_equal(rc, want_rc)
    assert int((rc & 0xFFFF).sum()) + int((rc >> 16).sum()) == scenes.PINNED_RAYS[name]


@pytest.mark.parametrize("name", ["c3", "c5"])
def test_full_frame_hash_vs_reference(tr, name):
    """Full-size frames: size-independent checks — FNV-1a of the whole float64 frame equals the hash of
    the reference's own frame, and the traced-ray total equals the reference's."""
    cfg = scenes.CONFIGS[name]
    rgb, rc = _render64(tr, cfg.scene(), cfg.camera(), cfg.width, cfg.height, cfg.depth)
    assert f"{po.fnv1a64(rgb):016x}" == golden.manifest()["frames"][name]["fnv1a64"]
    assert int((rc & 0xFFFF).sum()) + int((rc >> 16).sum()) == scenes.PINNED_RAYS[name]


@pytest.mark.parametrize("name", ["c3", "c5", "demo"])
def test_intersection_kat(tr, name):
    cfg = scenes.CONFIGS[name]
    k = golden.kat(name)
    tr.set_scene(cfg.scene())
    raw = tr.intersect(torch.tensor(k["starts"], device="cuda"), torch.tensor(k["ends"], device="cuda"))
    got = decode_hits(raw)
    assert np.array_equal(got["hit"], k["hit"])
    assert np.array_equal(got["material"], k["material"])
    for f in ("point", "normal", "reflected_end", "transmitted_end"):
        assert np.array_equal(got[f], k[f]), f


def _board_edge_rays():
    """Rays whose board-plane hit points sit at chosen offsets around the board's edges and its diagonal — both sides
    of the position shortcut's margin delta = L 2^-19 (board_hit) — and far beyond the board (|w| up to 2^24 L and
    past it), from the eye, from above the board and from grazing origins."""
    L, v0 = 320.0, np.array([-160.0, 0.0, -320.0])
    delta = L * 2.0 ** -19
    offs = [0.0, 1e-13, -1e-13, 1e-7, -1e-7, delta / 2, -delta / 2, delta, -delta, 2 * delta, -2 * delta, 1e-2, -1e-2,
            5.0, -5.0]
    pts = []
    for e in offs:
        for a in (0.0, L):                                  # edges wx = 0, L and wz = 0, L
            for b in (37.0, 160.0 + e / 3, L - 11.0):
                pts += [(a + e, b), (b, a + e)]
        for b in (1.0, 100.0, 250.0, L - 1.0):              # the diagonal wx = wz
            pts += [(b + e, b), (b, b + e)]
    for far in (1e6, 2.0 ** 24 * L * 0.999, 2.0 ** 24 * L * 1.001, 1e12):
        pts += [(far, 100.0), (100.0, -far), (-far, -far)]
    q = v0 + np.array([[wx, 0.0, wz] for wx, wz in pts])
    starts, ends = [], []
    for o in ((0.0, 100.0, 200.0), (10.0, 50.0, -100.0), (0.0, 3e6, -160.0), (-500.0, 0.5, -160.0)):
        o = np.array(o)
        for t in q:
            starts.append(o)
            ends.append(o + (t - o) * 0.5)                 # the plane is crossed at m = 2
    return np.array(starts), np.array(ends)


@pytest.mark.parametrize("name", ["c3", "c5"])
def test_board_position_shortcut_edges(tr, name):
    """The board decided by its hit point's position (board_hit) equals the reference's barycentric
    tests on both sides of the margin, on the diagonal and far away: hits, points and colours, bit for bit."""
    cfg = scenes.CONFIGS[name]
    tr.set_scene(cfg.scene())
    s, e = _board_edge_rays()
    got = decode_hits(tr.intersect(torch.tensor(s, device="cuda"), torch.tensor(e, device="cuda")))
    want = po.intersect(cfg.scene().to_abi(), s, e)
    assert np.array_equal(got["hit"], want["hit"])
    assert np.array_equal(got["material"], want["material"])
    assert np.array_equal(got["point"], want["point"])
    for depth in (0, 2):
        rgb, _ = tr.trace_rays(torch.tensor(s, device="cuda"), torch.tensor(e, device="cuda"), depth)
        want_rgb, _ = po.trace_rays(cfg.scene().to_abi(), s, e, depth)
        assert np.array_equal(rgb.cpu().numpy(), want_rgb)
    # both outcomes occur near every edge: the test exercises the exact fallback and the shortcut
    assert 0 < int(np.sum(want["hit"])) < len(s)


@pytest.mark.parametrize("name", ["c3", "c5", "demo"])
def test_trace_rays_kat(tr, name):
    cfg = scenes.CONFIGS[name]
    k = golden.kat(name)
    tr.set_scene(cfg.scene())
    s = torch.tensor(k["starts"], device="cuda")
    e = torch.tensor(k["ends"], device="cuda")
    for depth in range(6):
        rgb, _ = tr.trace_rays(s, e, depth)
        _assert_parity(rgb.cpu().numpy(), k["colors"][depth])


def test_output_formats_consistent(tr):
    cfg = scenes.CONFIGS["c2"]
    W, H = 321, 203
    tr.set_scene(cfg.scene())
    b = tr.render(cfg.camera(W, H), W, H, cfg.depth, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    torch.cuda.synchronize()
    c64 = b["rgb64f"].cpu().numpy()
    c32 = b["rgba32f"].cpu().numpy()
    c8 = b["rgba8"].cpu().numpy()
    assert np.array_equal(c32[..., :3], c64.astype(np.float32))
    assert np.all(c32[..., 3] == 1.0)
    want8 = np.floor(np.clip(c64, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(c8[..., :3], want8)
    assert np.all(c8[..., 3] == 255)


@pytest.mark.parametrize("env", ["RT_SCENE_IN_LDS", "RT_WG_STAGING"])
@pytest.mark.parametrize("name", ["c2", "c5"])
def test_workgroup_variants_agree(env, name):
    """The 256-thread A/B variants (scene copied into LDS; LDS-staged row stores) equal the default
    one-wave-workgroup kernel and the oracle bit for bit — on every render of a view: the first (identity
    order), the calibration and the later renders in calibrated order (which never read the one-wave kernels'
    per-tile cone-mask cache)."""
    cfg = scenes.CONFIGS[name]
    W, H = 200, 150
    out = []
    for mode in ("1", "0"):
        os.environ[env] = mode
        t = Tracer(0)
        out.append([_render64(t, cfg.scene(), cfg.camera(W, H), W, H, cfg.depth)[0] for _ in range(4)])
        t.close()
    os.environ.pop(env)
    want, _ = po.render(cfg.scene().to_abi(), cfg.camera(W, H), W, H, cfg.depth)
    for k in range(4):
        assert np.array_equal(out[0][k], want), f"{env}=1 render {k}"
        assert np.array_equal(out[1][k], want), f"{env}=0 render {k}"


@pytest.mark.parametrize("env", ["RT_SCENE_IN_LDS", "RT_WG_STAGING"])
@pytest.mark.parametrize("name", ["demo", "tree_demo"])
def test_workgroup_knobs_leave_one_wave_scenes_whole(env, name):
    """Transparent and ray-tree scenes have no 256-thread instance: under the A/B knobs they run their one-wave
    kernels, and the frame's tiles are that instance's 8 x 8 (cut by the knob's 32 x 8 the one-wave kernel would trace a
    quarter of the columns).  Every pixel and counter equals the frame without the knob, on each render of the view."""
    scene = scenes.tree_case(name)[0] if name == "tree_demo" else scenes.CONFIGS[name].scene()
    W, H, depth = 200, 150, 3
    cam = scenes.CONFIGS["demo"].camera(W, H)
    out = []
    for mode in ("1", "0"):
        os.environ[env] = mode
        t = Tracer(0)
        t.set_scene(scene)
        frames = []
        for _ in range(3):
            b = t.alloc(W, H, None, rgba32f=False, rgb64f=True, raycount=True)
            b["rgb64f"].fill_(-7.0)
            b["raycount"].fill_(-7)
            t.render_into(cam, W, H, depth, b)
            torch.cuda.synchronize()
            frames.append((b["rgb64f"].cpu().numpy(), b["raycount"].cpu().numpy()))
        out.append(frames)
        t.close()
    os.environ.pop(env)
    for k in range(3):
        assert np.array_equal(out[0][k][0], out[1][k][0]), f"{env}=1 render {k}"
        assert np.array_equal(out[0][k][1], out[1][k][1]), f"{env}=1 render {k}"
        assert (out[1][k][1] != -7).all()


@pytest.mark.parametrize("G,hb", [(2, 8), (3, 5), (8, 16), (4, 1)])
def test_row_bands_and_unshuffle(tr, G, hb):
    cfg = scenes.CONFIGS["c2"]
    W, H = 250, 133
    full, _ = _render64(tr, cfg.scene(), cfg.camera(W, H), W, H, cfg.depth)
    slab = max(scenes.local_rows(H, scenes.rows(hb, G, r)) for r in range(G))
    gathered = torch.zeros((G, slab, W, 3), dtype=torch.float64, device="cuda")
    for r in range(G):
        part, _ = _render64(tr, cfg.scene(), cfg.camera(W, H), W, H, cfg.depth, rows=scenes.rows(hb, G, r))
        gathered[r, : part.shape[0]] = torch.tensor(part, device="cuda")
    img = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
    unshuffle(gathered, img, W, H, hb, G, slab)
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy(), full)


@pytest.mark.parametrize("W,H", [(1, 1), (33, 17), (31, 9), (64, 8), (7, 300)])
@pytest.mark.parametrize("depth", [0, 3, 7])
def test_odd_sizes_and_depths(tr, W, H, depth):
    cfg = scenes.CONFIGS["c3"]
    sc = cfg.scene()
    rgb, rc = _render64(tr, sc, cfg.camera(W, H), W, H, depth)
    want, want_rc = po.render(sc.to_abi(), cfg.camera(W, H), W, H, depth)
    _assert_parity(rgb, want)
    assert np.array_equal(rc, want_rc)


def _random_scene(rng, n_spheres, n_lights, board=True):
    sq = [chr(ord("a") + int(rng.integers(0, 8))) + chr(ord("1") + int(rng.integers(0, 8)))
          for _ in range(n_spheres)]
    sph = [scenes.SphereSpec(s, float(rng.uniform(2, 45)), float(rng.uniform(-70, 90))) for s in sq]
    lts = [scenes.LightSpec(chr(ord("a") + int(rng.integers(0, 8))) + chr(ord("1") + int(rng.integers(0, 8))),
                            tuple(float(x) for x in rng.uniform(0, 1, 3))) for _ in range(n_lights)]
    return scenes.Scene(spheres=sph, lights=lts, has_board=board)


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_random_scenes_vs_oracle(tr, seed):
    rng = np.random.default_rng(seed)
    sc = _random_scene(rng, int(rng.integers(0, 40)), int(rng.integers(0, 5)), board=bool(seed % 3))
    W, H = 160, 120
    cam = scenes.make_camera(W, H, float(rng.uniform(0.5, 4.0)))
    depth = int(rng.integers(0, 8))
    rgb, rc = _render64(tr, sc, cam, W, H, depth)
    want, want_rc = po.render(sc.to_abi(), cam, W, H, depth)
    _assert_parity(rgb, want)
    assert np.array_equal(rc, want_rc)
    # random rays from random origins through the same scene
    s = rng.uniform(-300, 300, (4096, 3))
    e = s + rng.normal(size=(4096, 3)) * rng.uniform(0.1, 100, (4096, 1))
    g, _ = tr.trace_rays(torch.tensor(s, device="cuda"), torch.tensor(e, device="cuda"), depth)
    w, _ = po.trace_rays(sc.to_abi(), s, e, depth)
    _assert_parity(g.cpu().numpy(), w)


def test_max_spheres_and_empty_scene(tr):
    rng = np.random.default_rng(7)
    big = _random_scene(rng, abi.RT_MAX_SPHERES, 2)
    W, H = 64, 48
    cam = scenes.make_camera(W, H, 500.0 / W)
    rgb, _ = _render64(tr, big, cam, W, H, 2)
    want, _ = po.render(big.to_abi(), cam, W, H, 2)
    _assert_parity(rgb, want)
    empty = scenes.Scene(spheres=[], lights=[], has_board=False)
    rgb, rc = _render64(tr, empty, cam, W, H, 3)
    assert not rgb.any()
    assert np.all(rc == 1)


def test_errors_are_loud(tr):
    L = abi.lib()
    cfg = scenes.CONFIGS["c1"]
    sc = cfg.scene()
    s = sc.to_abi()
    s.n_spheres = abi.RT_MAX_SPHERES + 1
    assert L.rt_set_scene(tr._ctx, ctypes.byref(s)) == abi.RT_EINVAL
    tr.set_scene(sc)
    cam = cfg.camera(8, 8)
    assert L.rt_render_dev(tr._ctx, ctypes.byref(cam), 8, 8, 8, None, None, None, None, None, None) == abi.RT_EINVAL
    assert L.rt_render_dev(tr._ctx, ctypes.byref(cam), 0, 8, 1, None, None, None, None, None, None) == abi.RT_EINVAL
    assert "depth" in abi.last_error() or "size" in abi.last_error()


def test_host_buffer_render_and_stats(tr):
    cfg = scenes.CONFIGS["c2"]
    sc = cfg.scene()
    rgb, st = tr.render_host(sc.to_abi(), cfg.camera(), cfg.width, cfg.height, cfg.depth)
    want, _ = po.render(sc.to_abi(), cfg.camera(), cfg.width, cfg.height, cfg.depth)
    _assert_parity(rgb, want)
    assert st.primary_rays + st.reflect_rays + st.shadow_rays == scenes.PINNED_RAYS["c2"]
    assert st.primary_rays == cfg.width * cfg.height
    assert st.kernel_ms > 0


def _ppm_expect(rgb64):
    q = np.floor(np.clip(rgb64, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    return q[::-1]                       # writePpmScreenshot writes the bottom-up image top-down


def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 1)
    hdr = parts[0].split()
    assert hdr[0] == b"P6" and hdr[3] == b"255"
    W, H = int(hdr[1]), int(hdr[2])
    return np.frombuffer(parts[1], np.uint8).reshape(H, W, 3)


def test_cli_canonical_scene_ppm(tmp_path):
    import subprocess
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "c1.ppm"
    r = subprocess.run([exe, "--config", "c1", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"rays {scenes.PINNED_RAYS['c1']}" in r.stdout
    cfg = scenes.CONFIGS["c1"]
    want, _ = po.render(cfg.scene().to_abi(), cfg.camera(), cfg.width, cfg.height, cfg.depth)
    assert np.array_equal(_read_ppm(out), _ppm_expect(want))


def test_cli_initscene2_dialogue_ppm(tmp_path):
    """initScene2's stdin dialogue (MySdlApplication.cpp:1430-1493) -> loadScene -> draw() at the
    reference's own window (500x500, unit pitch, MAX_DEPTH 5)."""
    import subprocess
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    answers = "d\nd7\ny\nzz\nd\nb2\nyes\na\nb6\nmaybe\nn\n"
    out = tmp_path / "app.ppm"
    r = subprocess.run([exe, "--stdin", "--out", str(out)], input=answers, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    sc = scenes.load_scene([("d7", scenes.SPHERE), ("b2", scenes.SPHERE), ("b6", scenes.LIGHT)])
    cam = scenes.make_camera(500, 500, 1.0)
    want, _ = po.render(sc.to_abi(), cam, 500, 500, 5)
    assert np.array_equal(_read_ppm(out), _ppm_expect(want))


def _random_mesh_scene(rng):
    entries = []
    for _ in range(int(rng.integers(1, 14))):
        sq = chr(ord("a") + int(rng.integers(0, 8))) + chr(ord("1") + int(rng.integers(0, 8)))
        entries.append((sq, int(rng.choice([scenes.SPHERE, scenes.TETRAHEDRON, scenes.CUBE]))))
    entries.append((chr(ord("a") + int(rng.integers(0, 8))) + chr(ord("1") + int(rng.integers(0, 8))), scenes.LIGHT))
    return scenes.load_scene(entries)


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_mesh_scenes_vs_oracle(tr, seed):
    """loadScene boards with tetrahedra (transparent, refracting), cubes and spheres: frames and random rays."""
    rng = np.random.default_rng(1000 + seed)
    sc = _random_mesh_scene(rng)
    W, H = 128, 96
    cam = scenes.make_camera(W, H, float(rng.uniform(0.8, 4.0)))
    depth = int(rng.integers(0, 8))
    rgb, rc = _render64(tr, sc, cam, W, H, depth)
    want, want_rc = po.render(sc.to_abi(), cam, W, H, depth)
    _assert_parity(rgb, want)
    assert np.array_equal(rc, want_rc)
    s = rng.uniform(-250, 250, (2048, 3))
    e = s + rng.normal(size=(2048, 3)) * rng.uniform(0.1, 100, (2048, 1))
    g, _ = tr.trace_rays(torch.tensor(s, device="cuda"), torch.tensor(e, device="cuda"), depth)
    w, _ = po.trace_rays(sc.to_abi(), s, e, depth)
    _assert_parity(g.cpu().numpy(), w)
    raw = tr.intersect(torch.tensor(s, device="cuda"), torch.tensor(e, device="cuda"))
    got = decode_hits(raw)
    want_h = po.intersect(sc.to_abi(), s, e)
    for f in ("hit", "material", "point", "normal", "reflected_end", "transmitted_end"):
        assert np.array_equal(got[f], want_h[f], equal_nan=True), f


def test_cli_demo_ppm(tmp_path):
    import subprocess
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "demo.ppm"
    r = subprocess.run([exe, "--config", "demo", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"rays {scenes.PINNED_RAYS['demo']}" in r.stdout
    cfg = scenes.CONFIGS["demo"]
    want, _ = po.render(cfg.scene().to_abi(), cfg.camera(), cfg.width, cfg.height, cfg.depth)
    assert np.array_equal(_read_ppm(out), _ppm_expect(want))


@pytest.mark.parametrize("G,frames", [(2, 2), (4, 4), (3, 2)])
def test_stacked_frames_frame_major(tr, G, frames):
    """rt_rows.frames: a rank's bands of several frames in one launch, frame-major (the bench's frame
    streams); every frame's rows equal the single-frame render's."""
    from ray_tracer_fragment_shader_amd.distributed import BandPlan
    cfg = scenes.CONFIGS["c2"]
    W, H = 96, 72
    full, _ = _render64(tr, cfg.scene(), cfg.camera(W, H), W, H, cfg.depth)
    plan = BandPlan(H, G, frames=frames)
    for r in range(G):
        part, rc = _render64(tr, cfg.scene(), cfg.camera(W, H), W, H, cfg.depth, rows=plan.rows(r))
        want, want_rc = po.render(cfg.scene().to_abi(), cfg.camera(W, H), W, H, cfg.depth, rows=plan.rows(r))
        _assert_parity(part, want)
        fl = plan.frame_local[r]
        js = [j for j in range(H) if (j // plan.band_height) % G == r]
        for f in range(frames):
            assert np.array_equal(part[f * fl:(f + 1) * fl], full[js])


def _math_operands(rng):
    """Vectors around every threshold of the sqrt / division fast paths (rt_device.hpp)."""
    vals = [0.0, -0.0, 1.0, -1.0, 3.0, 1e-300, -1e-300, 5e-324, -5e-324, 2.2250738585072014e-308,
            2.0 ** -500, -(2.0 ** -500), 2.0 ** -501, 2.0 ** -499, 2.0 ** -350, 2.0 ** -351, 2.0 ** -349,
            2.0 ** 350, 2.0 ** 349.5, 2.0 ** 351, 1e200, 1e300, -1e300, np.inf, -np.inf, np.nan,
            40.0, 0.1, 1e-14, 160.0, -320.0, 277.12812921102034]
    vals = np.array(vals)
    rows = [rng.choice(vals, size=3) for _ in range(4000)]
    with np.errstate(over="ignore"):
        big = [(np.ldexp(1.0, e), np.exp2(e / 2)) for e in range(-1100, 1100, 7)]
    for p, h in big:                                     # one component across the exponent range
        rows.append(np.array([p, 1.0, 0.0]))
        rows.append(np.array([h, h * 0.7, -h * 0.3]))
    rows += list(rng.normal(size=(4000, 3)) * 10.0 ** rng.uniform(-20, 20, size=(4000, 1)))
    rows += list(rng.uniform(-400, 400, size=(4000, 3)))
    rows += list(np.where(rng.random((2000, 3)) < 0.3, 0.0, rng.normal(size=(2000, 3))))
    return np.ascontiguousarray(np.array(rows, dtype=np.float64))


def _same_bits(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)
    return (ia == ib) | (np.isnan(a) & np.isnan(b))


def test_math_fast_paths(tr):
    """unit()/len_fast() (exact fast paths of the render kernel) return the bits of the compiler's IEEE
    sqrt and division, which are the binary64 results numpy computes on the host."""
    import torch
    v = _math_operands(np.random.default_rng(7))
    n = len(v)
    dv = torch.from_numpy(v).cuda()
    out = torch.empty((n, 9), dtype=torch.float64, device="cuda")
    abi.check(abi.lib().rt_probe_math_dev(0, ctypes.c_void_p(dv.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                          None), "rt_probe_math_dev")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    with np.errstate(all="ignore"):
        s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        l = np.sqrt(s)
        u = v / l[:, None]
    assert _same_bits(o[:, 3], l).all()
    assert _same_bits(o[:, 0:3], u).all()
    assert _same_bits(o[:, 4:8], o[:, 0:4]).all()
    assert _same_bits(o[:, 8], o[:, 3]).all()
    fast = (s >= 2.0 ** -700) & (s <= 2.0 ** 700)
    assert fast.sum() > n // 2 and (~fast).sum() > 100        # both paths exercised


@pytest.mark.parametrize("G,hb,frames", [(1, 8, 1), (3, 5, 2), (2, 3, 3)])
def test_primary_cone_culling_bands_frames(tr, G, hb, frames):
    """64 spheres (>= kConeMin: per-wave primary culling) under row bands and stacked frames, where a
    wave's 8 rows may straddle bands or frames."""
    cfg = scenes.CONFIGS["c5"]
    W, H = 203, 97
    cam = cfg.camera(W, H)
    for r in range(G):
        rows = scenes.rows(hb, G, r, frames)
        got, rc = _render64(tr, cfg.scene(), cam, W, H, 2, rows=rows)
        want, want_rc = po.render(cfg.scene().to_abi(), cam, W, H, 2, rows=rows)
        _assert_parity(got, want)
        assert np.array_equal(rc, want_rc)


@pytest.mark.parametrize("seed", range(6))
def test_primary_cone_culling_random_cameras(tr, seed):
    """Many spheres seen from random eyes (close up, inside a sphere, far away) and pitches."""
    rng = np.random.default_rng(300 + seed)
    sc = _random_scene(rng, int(rng.integers(16, 120)), int(rng.integers(1, 3)))
    W, H = 120, 88
    cam = scenes.make_camera(W, H, float(rng.choice([0.05, 0.5, 2.0, 9.0])))
    if seed % 3 == 1:                                 # eye among (possibly inside) the spheres
        sp = sc.spheres[int(rng.integers(0, len(sc.spheres)))]
        c = np.array(sp.center()) + np.array([0.0, 0.0, -160.0])
        eye = c + rng.normal(size=3) * sp.radius * float(rng.choice([0.5, 1.5]))
        cam.eye = abi.vec3(eye)
    elif seed % 3 == 2:                               # far away
        cam.eye = abi.vec3((0.0, 3000.0, 9000.0))
    got, rc = _render64(tr, sc, cam, W, H, 1)
    want, want_rc = po.render(sc.to_abi(), cam, W, H, 1)
    _assert_parity(got, want)
    assert np.array_equal(rc, want_rc)


def _render_screen(tr, scene, W, H, depth, rng, seed, bx=None, by=None):
    from ray_tracer_fragment_shader_amd import scenes as S
    cam = S.make_camera(W, H, 1.0)
    if bx is not None:
        cam.bottom_x, cam.bottom_y = bx, by
    rgb = np.zeros((H, W, 3), np.float64)
    rgba8 = np.zeros((H, W, 4), np.uint8)
    ns = np.zeros((H, W), np.uint8)
    calls = ctypes.c_uint64()
    abi.check(abi.lib().rt_render_screen(tr._ctx, ctypes.byref(scene.to_abi()), ctypes.byref(cam), W, H, depth, rng,
                                         seed, rgb.ctypes.data, rgba8.ctypes.data, ns.ctypes.data,
                                         ctypes.byref(calls)), "rt_render_screen")
    return rgb, rgba8, ns, int(calls.value)


@pytest.mark.parametrize("name,W,H,rng,seed", [("c1", 48, 36, 0, 1), ("c2", 64, 36, 1, 1), ("demo", 50, 50, 0, 1),
                                               ("c2", 40, 30, 0, 7), ("c5", 37, 23, 1, 99), ("demo", 23, 61, 1, 5)])
def test_render_screen_faithful_vs_oracle(tr, name, W, H, rng, seed):
    """rt_render_screen (speculative GPU chunks + in-order resolution) equals the serial restatement bit for
    bit: colours, per-pixel sample counts and rand() consumption; glibc cases also equal the reference's
    own rand() consumption (tests/golden/screen.json)."""
    sc = scenes.CONFIGS[name].scene()
    rgb, rgba8, ns, calls = _render_screen(tr, sc, W, H, 5, rng, seed)
    want_rgb, want_ns, want_calls = po.render_screen(sc.to_abi(), W, H, 5, rng, seed)
    assert np.array_equal(ns, want_ns)
    assert calls == want_calls
    assert np.array_equal(rgb, want_rgb)
    q = np.floor(np.clip(want_rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(rgba8[..., :3], q) and (rgba8[..., 3] == 255).all()
    for g in golden.screen()["cases"]:
        if (g["scene"], g["width"], g["height"], g["seed"], rng) == (name, W, H, seed, 0):
            assert calls == g["calls"]


def test_render_screen_on_another_device_than_current():
    """rt_render_screen on a context of device 1 while device 0 is current: its workspace (streams, events, mapped
    buffers) and launches belong to the context's device, the frame equals the restatement, and the caller's current
    device is unchanged afterwards."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    t1 = Tracer(1)
    try:
        sc = scenes.CONFIGS["demo"].scene()
        for _ in range(2):                                  # the second call reuses the cached workspace
            torch.cuda.set_device(0)
            rgb, _, ns, calls = _render_screen(t1, sc, 64, 48, 5, 0, 1)
            assert torch.cuda.current_device() == 0
            want_rgb, want_ns, want_calls = po.render_screen(sc.to_abi(), 64, 48, 5, 0, 1)
            assert np.array_equal(ns, want_ns) and calls == want_calls and np.array_equal(rgb, want_rgb)
    finally:
        t1.close()


@pytest.mark.parametrize("env", [{"RT_SCREEN_NEXT_MIN": "0"}, {"RT_SCREEN_NEXT_MIN": "0", "RT_SCREEN_AHEAD": "2"},
                                 {"RT_SCREEN_NEXT": "0"}, {"RT_SCREEN_NEXT_MIN": "0", "RT_SCREEN_PROGRESSIVE": "1"}],
                         ids=["every_chunk", "ahead2", "next0", "progressive"])
def test_render_screen_pipelines_vs_oracle(tr, monkeypatch, env):
    """The chunk pipelines the default rarely takes on small frames (continuations behind every chunk, two of them,
    none), read from the environment at each call: the same frame, bit for bit, as the serial restatement."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = scenes.CONFIGS["demo"].scene()
    for rng, seed, W, H in ((0, 1, 160, 120), (1, 4, 97, 61)):
        rgb, _, ns, calls = _render_screen(tr, sc, W, H, 5, rng, seed)
        want_rgb, want_ns, want_calls = po.render_screen(sc.to_abi(), W, H, 5, rng, seed)
        assert np.array_equal(ns, want_ns) and calls == want_calls
        assert np.array_equal(rgb, want_rgb)


def test_cli_faithful_screen_ppm(tmp_path):
    """`rt_render --config demo --faithful msvc`: the app's rayTraceScreen frame through rt_render_screen."""
    import subprocess
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    out = tmp_path / "demo_faithful.ppm"
    r = subprocess.run([exe, "--config", "demo", "--faithful", "msvc", "--seed", "3", "--width", "64", "--height",
                        "48", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want, ns, calls = po.render_screen(scenes.CONFIGS["demo"].scene().to_abi(), 64, 48, 5, po.MSVC, 3)
    assert f"{int(ns.sum())} samples, {calls} rand() calls" in r.stdout
    assert np.array_equal(_read_ppm(out), _ppm_expect(want))


def test_render_dev_graph_capture(tr):
    """rt_render_dev is asynchronous and allocation-free: it can be captured in a HIP graph and replayed."""
    import torch
    cfg = scenes.CONFIGS["c1"]
    W, H = 200, 150
    cam = cfg.camera(W, H)
    tr.set_scene(cfg.scene())
    bufs = tr.alloc(W, H, rgba32f=False, rgba8=True, rgb64f=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tr.render_into(cam, W, H, cfg.depth, bufs, stream=s)   # warm-up: per-eye data prepared outside
    s.synchronize()
    for b in bufs.values():
        if b is not None:
            b.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        tr.render_into(cam, W, H, cfg.depth, bufs, stream=s)
    g.replay()
    torch.cuda.synchronize()
    want, _ = po.render(cfg.scene().to_abi(), cam, W, H, cfg.depth)
    assert np.array_equal(bufs["rgb64f"].cpu().numpy(), want)
    bufs["rgb64f"].zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bufs["rgb64f"].cpu().numpy(), want)


def test_checker_division_fast_path(tr):
    """div_core(a, b, rcp_core(b)) (the checker's quotients) equals IEEE a / b bit for bit for normal
    b and |a| in [2^-969, 2^500] (and truncates to the same int everywhere on a board)."""
    import torch
    rng = np.random.default_rng(11)
    a = np.concatenate([rng.uniform(-400, 400, 20000), rng.uniform(-1, 1, 5000) * 40.0,
                        np.arange(-400, 401, 40, dtype=np.float64), np.arange(-400, 401, 40) + 1e-13,
                        np.arange(-400, 401, 40) - 1e-13, np.ldexp(1.0, np.arange(-960, 490, 3)),
                        -np.ldexp(1.0, np.arange(-960, 490, 3)) * 1.37, [0.0, -0.0, 1e-300, -1e-310]])
    b = np.concatenate([np.full(len(a) - 40, 40.0), rng.uniform(0.5, 1e3, 40)])
    pairs = np.ascontiguousarray(np.stack([a, b], axis=1))
    d = torch.from_numpy(pairs).cuda()
    out = torch.empty_like(d)
    abi.check(abi.lib().rt_probe_math_dev(1, ctypes.c_void_p(d.data_ptr()), len(a), ctypes.c_void_p(out.data_ptr()),
                                          None), "rt_probe_math_dev")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    ieee = a / b
    assert np.array_equal(o[:, 0], ieee)
    regular = (np.abs(a) >= 2.0 ** -969) & (np.abs(a) <= 2.0 ** 500)
    assert _same_bits(o[regular, 1], ieee[regular]).all()
    board = np.abs(a) <= 1e4
    assert np.array_equal(np.trunc(o[board, 1]), np.trunc(ieee[board]))


@pytest.mark.parametrize("name,W,H,rows", [("c2", 480, 270, None), ("c5", 640, 360, None),
                                           ("c3", 400, 300, (4, 3, 1, 2))])
def test_tile_order_adaptive(tr, name, W, H, rows):
    """The adaptive tile-row order (a calibration render times its tile rows, later renders dispatch them
    longest first, rt_order_kernel) only reorders work: every render is bit-identical to the bottom-to-top
    order and to the oracle."""
    cfg = scenes.CONFIGS[name]
    sc, cam = cfg.scene(), cfg.camera(W, H)
    rr = abi.rt_rows(*rows) if rows else None
    lib = abi.lib()
    try:
        abi.check(lib.rt_diag_tile_order(tr._ctx, 1), "rt_diag_tile_order")
        base, base_rc = _render64(tr, sc, cam, W, H, cfg.depth, rows=rr)
        abi.check(lib.rt_diag_tile_order(tr._ctx, 0), "rt_diag_tile_order")
        tr.set_scene(sc)
        for k in range(3):                       # calibration render, then two ordered renders
            b = tr.render(cam, W, H, cfg.depth, rows=rr, rgba32f=False, rgb64f=True, raycount=True)
            torch.cuda.synchronize()
            assert np.array_equal(b["rgb64f"].cpu().numpy(), base, equal_nan=True), f"render {k} differs"
            assert np.array_equal(b["raycount"].cpu().numpy().view(np.uint32), base_rc)
    finally:
        lib.rt_diag_tile_order(tr._ctx, 0)
    if rows is None and name != "c5":
        want, _ = po.render(sc.to_abi(), cam, W, H, cfg.depth)
        _assert_parity(base, want)
    with pytest.raises(abi.RtError):
        abi.check(lib.rt_diag_tile_order(tr._ctx, 7), "rt_diag_tile_order")


def test_tall_frame_grid_slices(tr):
    """More than 32,768 tile rows: the launch splits its rows over grid.z slices (rt_render_dev)."""
    cfg = scenes.CONFIGS["c1"]
    W, H = 2, 8 * 32768 + 20
    sc, cam = cfg.scene(), cfg.camera(W, H)
    rgb, rc = _render64(tr, sc, cam, W, H, 1)
    want, want_rc = po.render(sc.to_abi(), cam, W, H, 1)
    _assert_parity(rgb, want)
    assert np.array_equal(rc, want_rc)


# ---------------------------------------------------------------------------------------------- ray trees
# Materials that transmit AND reflect (scenes.TREE_CASES): the trace_tree kernels (per-lane node stack)
# against the reference-generated fixtures and the oracle; NaN positions must agree, payloads are free.
TREES = list(scenes.TREE_CASES)


@pytest.mark.parametrize("name", TREES)
def test_tree_small_frame_vs_reference(tr, name):
    sc, cfg, depth, _ = scenes.tree_case(name)
    g = golden.tree(name)
    W, H = (int(x) for x in g["small_wh"])
    rgb, _ = _render64(tr, sc, cfg.camera(W, H), W, H, depth)
    _assert_parity(rgb, g["small"])


@pytest.mark.parametrize("name", TREES)
def test_tree_samples_and_kat_vs_reference(tr, name):
    sc, cfg, depth, (W, H) = scenes.tree_case(name)
    g = golden.tree(name)
    tr.set_scene(sc)
    sp = po.screen_points(scenes.make_camera(W, H, 500.0 / W), W, H)[g["pj"], g["pi"]]
    starts = torch.tensor(np.tile(CAM, (len(sp), 1)), device="cuda")
    rgb, _ = tr.trace_rays(starts, torch.tensor(np.ascontiguousarray(sp), device="cuda"), depth)
    _assert_parity(rgb.cpu().numpy(), g["samples"])
    s = torch.tensor(g["starts"], device="cuda")
    e = torch.tensor(g["ends"], device="cuda")
    for d in range(depth + 1):
        rgb, rc = tr.trace_rays(s, e, d)
        _assert_parity(rgb.cpu().numpy(), g["colors"][d])
        _, want_rc = po.trace_rays(sc.to_abi(), g["starts"], g["ends"], d)
        assert np.array_equal(rc.cpu().numpy().view(np.uint32), want_rc), d


@pytest.mark.parametrize("name", TREES)
def test_tree_full_frame_vs_reference_hash(tr, name):
    """Full-size tree frame: FNV-1a (NaNs canonical) equals the reference's; ray counts equal the oracle's
    per pixel; RGBA32F / RGBA8 agree with the FP64 frame."""
    sc, cfg, depth, (W, H) = scenes.tree_case(name)
    cam = scenes.make_camera(W, H, 500.0 / W)
    tr.set_scene(sc)
    b = tr.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    torch.cuda.synchronize()
    rgb = b["rgb64f"].cpu().numpy()
    man = golden.manifest()["tree"][name]
    assert f"{po.fnv1a64(golden.canonical_nan(rgb)):016x}" == man["fnv1a64_canonical_nan"]
    _, want_rc = po.render(sc.to_abi(), cam, W, H, depth)
    assert np.array_equal(b["raycount"].cpu().numpy().view(np.uint32), want_rc)
    f32 = b["rgba32f"].cpu().numpy()
    assert np.array_equal(f32[..., :3], rgb.astype(np.float32), equal_nan=True)
    want8 = np.floor(np.clip(np.nan_to_num(rgb, nan=0.0), 0, 1) * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(b["rgba8"].cpu().numpy()[..., :3], want8)


def test_tree_depth_range_and_graph(tr):
    """Ray trees at every depth 0..7 (the node stack's full size) vs the oracle on a 64 x 48 frame, and a
    captured tree render replays bit-exact."""
    sc, cfg, _, _ = scenes.tree_case("tree_c2")
    W, H = 64, 48
    cam = cfg.camera(W, H)
    for depth in range(8):
        rgb, rc = _render64(tr, sc, cam, W, H, depth)
        want, want_rc = po.render(sc.to_abi(), cam, W, H, depth)
        _assert_parity(rgb, want)
        assert np.array_equal(rc, want_rc), depth
    tr.set_scene(sc)
    bufs = tr.alloc(W, H, rgb64f=True)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        tr.render_into(cam, W, H, 7, bufs, stream=s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        tr.render_into(cam, W, H, 7, bufs, stream=s)
    bufs["rgb64f"].zero_()
    g.replay()
    torch.cuda.synchronize()
    _assert_parity(bufs["rgb64f"].cpu().numpy(), want)


def test_origin_skips_edge_cases(tr):
    """The exact skips for rays that start at a hit (origin_skip: the board test after a board hit, a sphere's
    own test after a hit on it) at their thresholds: rays from far above the board (|p0.y| past
    board_skip_y, so the board is tested again), tiny / huge / distant spheres (the self-test bound fails and
    the sphere is tested again), grazing and inward rays; every colour and ray count equals the oracle's."""
    rng = np.random.default_rng(7)
    sc = scenes.Scene(spheres=[scenes.SphereSpec("d4", 1e-3), scenes.SphereSpec("e5", 20.0, 1e-9),
                               scenes.SphereSpec("c3", 5e3, -5e3 - 60.0), scenes.SphereSpec("f6", 20.0, 3e6),
                               scenes.SphereSpec("b2", 0.5, 30.0)],
                      lights=[scenes.LightSpec("b6", scenes.WHITE), scenes.LightSpec("g3", scenes.GREY)])
    tr.set_scene(sc)
    n = 6144
    heights = np.concatenate([np.full(n // 6, h) for h in (50.0, 1e3, 5e6, 6e6, 1e9, 1e15)])
    starts = np.stack([rng.uniform(-150, 150, n), heights, rng.uniform(-310, -10, n)], axis=1)
    ends = np.stack([rng.uniform(-150, 150, n), np.zeros(n), rng.uniform(-310, -10, n)], axis=1)
    # rays at the spheres' surfaces, from outside and inside
    cs = np.array([sp.center() for sp in sc.spheres]) + np.array([0.0, 0.0, -160.0])
    k = rng.integers(0, len(cs), n)
    dirs = rng.normal(size=(n, 3))
    starts2 = cs[k] + dirs * rng.uniform(0.5, 3.0, (n, 1)) * np.array([sp.radius for sp in sc.spheres])[k, None]
    ends2 = cs[k] + rng.normal(size=(n, 3)) * 0.1
    s = np.concatenate([starts, starts2])
    e = np.concatenate([ends, ends2])
    S, E = torch.tensor(s, device="cuda"), torch.tensor(e, device="cuda")
    for depth in (1, 3):
        rgb, rc = tr.trace_rays(S, E, depth)
        want, want_rc = po.trace_rays(sc.to_abi(), s, e, depth)
        _assert_parity(rgb.cpu().numpy(), want)
        assert np.array_equal(rc.cpu().numpy().view(np.uint32), want_rc), depth


@pytest.mark.parametrize("name", ["c3", "c5", "demo"])
@pytest.mark.parametrize("eps", [0.49, 1.0, 1.5, 12.0])
def test_large_small_number_vs_oracle(tr, name, eps):
    """SMALL_NUMBER (MSA:50) of 0.49 and at or above 1: the reference then culls bounding-sphere roots with
    |s| < eps (:754) that the exact shortcuts prove to be >= 1 (inner2 for origins inside the bound, prim_bound_ok for
    primary hits from an eye outside it), and misses sphere / board hits nearer than eps.  The shortcuts must stand
    down above 0.5; frames and ray counts equal the oracle's bit for bit."""
    cfg = scenes.CONFIGS[name]
    W, H = 96, 72
    sc = cfg.scene().to_abi()
    sc.small_number = eps
    rgb, rc = _render64(tr, sc, cfg.camera(W, H), W, H, cfg.depth)
    want, want_rc = po.render(sc, cfg.camera(W, H), W, H, cfg.depth)
    _assert_parity(rgb, want)
    assert np.array_equal(rc, want_rc)
    # rays from points inside the bounding sphere (the inner2 shortcut's domain) and from hit points
    rng = np.random.default_rng(int(eps * 100))
    n = 2048
    s = np.stack([rng.uniform(-120, 120, n), rng.uniform(0.5, 60, n), rng.uniform(-300, -20, n)], axis=1)
    e = s + rng.normal(size=(n, 3)) * 40.0
    got, grc = tr.trace_rays(torch.tensor(s, device="cuda"), torch.tensor(e, device="cuda"), cfg.depth)
    want, want_rc = po.trace_rays(sc, s, e, cfg.depth)
    _assert_parity(got.cpu().numpy(), want)
    assert np.array_equal(grc.cpu().numpy().view(np.uint32), want_rc)


def test_render_kernels_do_not_spill(tr):
    """The render kernels the benchmark configs launch keep everything in registers (private scratch would
    be written back to HBM: PMC showed 1.2x the algorithmic write bytes when the r02 bounce loop spilled 36 B/lane),
    and the depth <= 2 fast kernels fit 6 waves per SIMD (<= 80 VGPRs), the culling kernels of depth 0, 1 and 3
    seven (<= 72 VGPRs, r04).  rt_diag_kernel_resources reads the instances' hipFuncGetAttributes."""
    L = abi.lib()
    regs, scratch = ctypes.c_int(), ctypes.c_int()
    table = {}
    for variant in (0, 1, 2, 3, 4, 5):
        for depth in range(8 if variant < 4 else 4):  # (the achromatic instances 4 / 5: depths 0..3)
            abi.check(L.rt_diag_kernel_resources(depth, variant, ctypes.byref(regs), ctypes.byref(scratch)),
                      "rt_diag_kernel_resources")
            table[(variant, depth)] = (regs.value, scratch.value)
    print(table)
    for depth in range(4):                           # c1..c5: spheres + board, and the culling variant
        for fast, cull in ((0, 1), (4, 5)):          # three-channel and achromatic instances
            assert table[(fast, depth)][1] == 0, (depth, table[(fast, depth)])
            assert table[(cull, depth)][1] == 0, (depth, table[(cull, depth)])
            if depth != 2:
                assert table[(cull, depth)][0] <= 72, (depth, table[(cull, depth)])   # 7 waves per SIMD
    for depth in range(3):
        assert table[(0, depth)][0] <= 80, (depth, table[(0, depth)])
        assert table[(4, depth)][0] <= 80, (depth, table[(4, depth)])
    assert L.rt_diag_kernel_resources(4, 4, ctypes.byref(regs), ctypes.byref(scratch)) == abi.RT_EINVAL
    assert table[(3, 3)][1] > 0                     # the ray-tree node stack lives in scratch by design
    assert L.rt_diag_kernel_resources(8, 0, ctypes.byref(regs), ctypes.byref(scratch)) == abi.RT_EINVAL
