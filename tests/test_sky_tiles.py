"""The sky-tile verdict on the CPU (rt_diag_sky_tiles: the host evaluation of the proof the render kernel's waves make,
rt_cone.hpp) against the oracle's ray counters.

Soundness: a tile the verdict proves has the miss counter (one ray segment, no shadow ray) in every valid pixel — no
exception, whatever the eye: canonical, bench.py's orbit, below the board, steep, in and next to the board plane, and a
seeded set of random eyes; at sizes with whole tiles (320x184, 64x40) and partial ones (321x203).

Not vacuous: on the eight views the bound was prototyped on it proves at least 0.90 of the tiles that truly all miss
(0.95 of them at c2's 1920x1080 frame)."""
import numpy as np
import pytest

from ray_tracer_fragment_shader_amd import scenes

from . import sky_common as sk

SCENES = ["c2", "c3", "c5", "noboard", "rise"]
SIZES = [(320, 184), (321, 203), (64, 40)]
BELOW = (0.0, -50.0, 200.0)
STEEP = (0.0, 300.0, 10.0)


def _named_eyes(scene_abi):
    by = sk.board_y(scene_abi)
    eyes = [None] + sk.orbit_eyes() + [BELOW, STEEP]
    eyes += [(0.0, by + dh, 200.0) for dh in (1e-9, -1e-9, 1e-3, -1e-3, 0.0)]
    return eyes


def _check_sound(scene_abi, W, H, eye, rows=None):
    cam = sk.camera(W, H, eye)
    proved = sk.host_verdict(scene_abi, cam, W, H, rows).astype(bool)
    truth = sk.tiles_all_miss(sk.oracle_rc(scene_abi, cam, W, H, 1, rows))
    bad = np.argwhere(proved & ~truth)
    assert bad.size == 0, f"eye {eye}, {W}x{H}: proved tiles with a hit: {bad[:8].tolist()}"
    return int(proved.sum()), int(truth.sum())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_proved_tiles_all_miss_named_eyes(name, size):
    sa = sk.scene_named(name).to_abi()
    proved = 0
    for eye in _named_eyes(sa):
        proved += _check_sound(sa, size[0], size[1], eye)[0]
    assert proved > 0                                      # (the canonical view alone proves tiles in every scene)


@pytest.mark.parametrize("name", SCENES)
def test_proved_tiles_all_miss_random_eyes(name):
    """240 seeded eyes in a box around the board (side 320, centred on (0, 0, -160)): above and below it, inside and
    outside the scene's bound, some inside a sphere; the sizes in turn."""
    sa = sk.scene_named(name).to_abi()
    rng = np.random.default_rng(20240 + SCENES.index(name))
    proved = 0
    for k in range(240):
        eye = (float(rng.uniform(-300, 300)), float(rng.uniform(-150, 400)), float(rng.uniform(-400, 400)))
        W, H = SIZES[k % 3]
        proved += _check_sound(sa, W, H, eye)[0]
    assert proved > 0


def test_banded_rows_and_frames():
    """A rank's rows of a banded frame (band height 8: every tile is 8 consecutive image rows; band height 4: none
    is, and nothing may be proved) and a two-frame row plan."""
    sa = sk.scene_named("c2").to_abi()
    W, H = 320, 184
    for rank in (0, 1):
        p, t = _check_sound(sa, W, H, None, scenes.rows(8, 2, rank))
        assert 0 < p <= t
    assert _check_sound(sa, W, H, None, scenes.rows(4, 2, 0))[0] == 0
    p, t = _check_sound(sa, W, H, None, scenes.rows(1, 1, 0, frames=2))
    assert 0 < p <= t


def test_scenes_outside_the_early_out_prove_nothing():
    """Fewer than 8 spheres (no primary cone mask), a mesh scene: all zeros."""
    for sc in (scenes.CONFIGS["c1"].scene(), scenes.CONFIGS["demo"].scene()):
        sa = sc.to_abi()
        assert sk.host_verdict(sa, sk.camera(320, 184), 320, 184).sum() == 0


# the eight views the edge-plane bound was prototyped on (FP64, no FP32 margins: shares 0.972 .. 0.998)
PROTOTYPE_VIEWS = [("c2", 1920, 1080, None, 0.95), ("c3", 1920, 1080, None, 0.90), ("c5", 1920, 1080, None, 0.90),
                   ("c2", 320, 184, None, 0.90), ("c2", 321, 203, None, 0.90),
                   ("c2", 320, 184, (150.0, 40.0, 120.0), 0.90), ("c2", 320, 184, BELOW, 0.90),
                   ("c2", 320, 184, STEEP, 0.90)]


@pytest.mark.parametrize("name,W,H,eye,floor", PROTOTYPE_VIEWS,
                         ids=[f"{v[0]}-{v[1]}x{v[2]}-{'canonical' if v[3] is None else v[3]}" for v in PROTOTYPE_VIEWS])
def test_catch_share(name, W, H, eye, floor):
    sa = sk.scene_named(name).to_abi()
    proved, truth = _check_sound(sa, W, H, eye)
    assert truth > 0
    share = proved / truth
    print(f"{name} {W}x{H} eye {eye}: proved {proved} of {truth} all-miss tiles = {share:.4f}")
    assert share >= floor
