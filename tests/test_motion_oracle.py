"""Motion blur on the CPU: the three new symbols (the ABI version stays 10), the rules and pins of the contract on
its numpy restatement (tests/motion_common.py), the fixtures made from the reference build (tests/golden/motion.npz),
the conditions that make the GPU tests sensitive to every use of a sphere centre, and the CLI's usage errors.
No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes

from . import dof_common as dc
from . import motion_common as mc
from . import soft_common as so
from . import ssaa_common as sc

W, H = 37, 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVES = mc.MOVES


def test_symbols_and_abi_version():
    L = abi.lib()
    assert L.rt_abi_version() == 10 and abi.ABI_VERSION == 10
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_api.h")).read(), flags=re.S)
    for name in ("rt_set_motion", "rt_render_motion_dev", "rt_render_motion"):
        assert hasattr(L, name), name
        assert name in abi.SIGNATURES
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    assert len(abi.SIGNATURES["rt_set_motion"][1]) == 3
    assert len(abi.SIGNATURES["rt_render_motion_dev"][1]) == 14 and len(abi.SIGNATURES["rt_render_motion"][1]) == 15


# rules 2-3 ---------------------------------------------------------------------------------------------------
def test_times_and_centres_by_hand():
    """S = 2, F = 0.5: u = -3/4, -1/4, 1/4, 3/4 in the order (0, 0), (1, 0), (0, 1), (1, 1); c2's sphere 4 stands on
    c4, scene-local (-20, 60, 60), and moves by d = (320, 8, 0)."""
    assert [float(mc.time_of(2, 0.5, a, b)) for b in range(2) for a in range(2)] == [-0.375, -0.125, 0.125, 0.375]
    assert [float(mc.time_of(4, 1.0, a, b)) for a, b in ((0, 0), (3, 0), (0, 1), (3, 3))] == \
        [-15 / 16, -9 / 16, -7 / 16, 15 / 16]
    assert float(mc.time_of(1, 1.0, 0, 0)) == 0.0 and not np.signbit(mc.time_of(1, 1.0, 0, 0))
    scene, _ = sc.scene_of("c2")
    assert mc.local_centres(scene)[4].tolist() == [-20.0, 60.0, 60.0]
    d = mc.displacement(scene, ((4, (320.0, 8.0, 0.0)),))
    got = [mc.displaced_centres(scene, d, 2, 0.5, a, b)[4].tolist() for b in range(2) for a in range(2)]
    assert got == [[-140.0, 57.0, 60.0], [-60.0, 59.0, 60.0], [20.0, 61.0, 60.0], [100.0, 63.0, 60.0]]
    for b in range(2):
        for a in range(2):
            c = mc.displaced_centres(scene, d, 2, 0.5, a, b)
            assert np.array_equal(np.delete(c, 4, axis=0), np.delete(mc.local_centres(scene), 4, axis=0))
    assert mc.sphere_spec_of((100.0, 63.0, 60.0), 20.0) == scenes.SphereSpec("c7", 20.0, 3.0)


def test_no_centre_has_a_negative_zero():
    """The pins assume it (rule 6): c + (+-0) is c only then."""
    for name in ("c2", "c5", "demo", "tree_demo", "tree_c2"):
        scene, _ = sc.scene_of(name)
        c = mc.local_centres(scene)
        assert not ((c == 0.0) & np.signbit(c)).any(), name


# pins of the contract on the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("name,S", [("c2", 2), ("c5", 4), ("demo", 8), ("tree_demo", 2), ("tree_c2", 2)])
def test_shutter_zero_and_no_displacement_are_the_soft_frame(name, S):
    want = so.expected(name, W, H, S, 8.0, 40.0)
    for F, moves in ((0.0, MOVES[name]), (1.0, ())):
        e = mc.expected(name, W, H, S, 8.0, 40.0, F, moves)
        sc.assert_same_bits(e["hi"], want["hi"], f"{name} S={S} F={F} samples")
        assert np.array_equal(e["hi_rc"], want["hi_rc"])
        sc.assert_same_bits(e["rgb"], want["rgb"], f"{name} S={S} F={F}")
        assert np.array_equal(e["rc2"], want["rc2"])


@pytest.mark.parametrize("name,S", dc.FIXTURES)
def test_frozen_frame_is_the_dof_fixture(name, S):
    e = mc.expected(name, dc.FIX_W, dc.FIX_H, S, dc.FIX_A, 0.0, 0.0, MOVES[name])
    sc.assert_same_bits(e["rgb"], dc.fixtures()[sc.fixture_key(name, S)], f"{name} S={S}")


@pytest.mark.parametrize("name,S", sc.FIXTURES)
def test_frozen_pinhole_frame_is_the_ssaa_fixture(name, S):
    e = mc.expected(name, sc.FIX_W, sc.FIX_H, S, 0.0, 0.0, 1.0, ())
    sc.assert_same_bits(e["rgb"], sc.fixtures()[sc.fixture_key(name, S)], f"{name} S={S}")


@pytest.mark.parametrize("name", ["c2", "demo"])
def test_one_sample_is_the_plain_render(name):
    e = mc.expected(name, W, H, 1, 8.0, 40.0, 1.0, MOVES[name])
    scene, depth = sc.scene_of(name)
    rgb, rc = po.render(scene.to_abi(), e["cam"], W, H, depth)
    sc.assert_same_bits(e["rgb"], rgb, name)
    assert np.array_equal(e["rc2"], sc.reduce_counts(rc, 1))


# fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,S,F,A,R,lights,moves", mc.FIXTURES)
def test_oracle_route_reproduces_fixture(key, name, S, F, A, R, lights, moves):
    fx = mc.fixtures()
    assert sorted(fx) == sorted(f[0] for f in mc.FIXTURES), "recorded colours only"
    want = fx[key]
    assert want.shape == (mc.FIX_H, mc.FIX_W, 3) and want.dtype == np.float64
    e = mc.expected(name, mc.FIX_W, mc.FIX_H, S, A, R, F, moves, lights)
    sc.assert_same_bits(e["rgb"], want, key)
    if name == "tree_c2":
        assert np.isnan(want).any(), "the NaN fixture has no NaN"


def test_half_shutter_with_doubled_motion_is_the_same_fixture():
    fx = mc.fixtures()
    sc.assert_same_bits(fx["c2_s2_half"], fx["c2_s2"], "F = 0.5, 2 d")


@pytest.mark.ref
@pytest.mark.parametrize("key,name,S,F,A,R,lights,moves", mc.FIXTURES)
def test_reference_build_reproduces_fixture(key, name, S, F, A, R, lights, moves):
    if not po.ref_available():
        pytest.skip("no reference build here")
    scene, depth = sc.scene_of(name)
    cam = scenes.make_camera(mc.FIX_W, mc.FIX_H, 500.0 / mc.FIX_W)
    got = mc.render_ref(scene, cam, mc.FIX_W, mc.FIX_H, depth, S, A, R, F, mc.displacement(scene, moves), lights)
    sc.assert_same_bits(got, mc.fixtures()[key], key)


# sensitivity: a kernel that ignores the motion cannot pass the GPU tests ---------------------------------------
@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_motion_changes_the_frame(name, S):
    """(Measured on the oracle when the contract was written, S = 2 / 4 / 8, share of the 37 x 21 pixels that differ
    from the frozen frame in rgb64f and in RGBA8: DESIGN.md 5h has the table.)"""
    e, e0 = mc.expected(name, W, H, S, 0.0, 0.0, 1.0, MOVES[name]), mc.expected(name, W, H, S, 0.0, 0.0, 1.0, ())
    f64 = dc.differ(e["rgb"], e0["rgb"]).mean()
    u8 = dc.differ(sc.to_rgba8(e["rgb"]), sc.to_rgba8(e0["rgb"])).mean()
    print(f"{name} S={S}: rgb64f differs in {100 * f64:.1f} % of the pixels, rgba8 in {100 * u8:.1f} %")
    assert f64 >= 0.04
    assert u8 >= 0.03


# the frames a kernel that moves only some uses of the centre cannot pass ----------------------------------------
def _frames(case, depth=None):
    scene, dcase, S, F, moves = case()
    depth = dcase if depth is None else depth
    cam = scenes.make_camera(W, H, 500.0 / W)
    d = mc.displacement(scene, moves)
    moving = mc.render(scene, cam, W, H, depth, S, 0.0, 0.0, F, d)
    frozen = mc.render(scene, cam, W, H, depth, S, 0.0, 0.0, 0.0, d)
    return scene, cam, S, F, d, moves[0][0], moving, frozen


def test_shadow_only_frame():
    """No primary ray of any sample meets the moving sphere, so a kernel that moved it for primary rays only would
    render the frozen frame; the frame differs from it because the shadow moves.  (Measured: 61 pixels.)"""
    scene, cam, S, F, d, k, moving, frozen = _frames(mc.shadow_only_case)
    assert not mc.primary_hits_sphere(scene, cam, W, H, S, F, d, k).any()
    assert np.array_equal(moving["hi_rc"], frozen["hi_rc"]), "depth 0: the same rays either way"
    n = int(dc.differ(sc.to_rgba8(moving["rgb"]), sc.to_rgba8(frozen["rgb"])).sum())
    flips = int((so.shadowed(moving) != so.shadowed(frozen)).sum())
    print(f"shadow only: {n} pixels differ from the frozen (= primary-only motion) frame, {flips} samples flip")
    assert n >= 20 and flips >= 20


def test_reflection_only_frame():
    """No primary ray meets the moving sphere; at depth 0 a pixel can change only through its shadow.  The pixels
    that change at depth 1 although their depth-0 value does not see the sphere in the reflection alone.
    (Measured: 69 pixels differ at depth 1, 7 of them with an unchanged depth-0 value.)"""
    scene, cam, S, F, d, k, moving, frozen = _frames(mc.reflection_only_case)
    assert not mc.primary_hits_sphere(scene, cam, W, H, S, F, d, k).any()
    _, _, _, _, _, _, moving0, frozen0 = _frames(mc.reflection_only_case, depth=0)
    changed = dc.differ(sc.to_rgba8(moving["rgb"]), sc.to_rgba8(frozen["rgb"]))
    by_reflection = dc.differ(moving["rgb"], frozen["rgb"]) & ~dc.differ(moving0["rgb"], frozen0["rgb"])
    print(f"reflection only: {int(changed.sum())} pixels differ from the frozen (= primary-only motion) frame, "
          f"{int(by_reflection.sum())} of them through the reflection alone")
    assert changed.sum() >= 20 and by_reflection.sum() >= 3


def test_fast_small_sphere_frame():
    """|d| = 8 r: most of the samples that hit the sphere hit it where the FP32 filter record of its stored centre
    rejects their ray by a wide margin, so a kernel that kept that record loses them.  (Measured: 30 samples hit the
    sphere, 23 of them rejected by the static record; 25 pixels differ from the frozen frame.)"""
    scene, cam, S, F, d, k, moving, frozen = _frames(mc.fast_small_case)
    assert np.linalg.norm(d[k]) >= 4 * scene.spheres[k].radius
    on = mc.primary_hits_sphere(scene, cam, W, H, S, F, d, k)
    starts, ends = dc.rays(cam, W, H, S, 0.0)
    rej = mc.static_filter_rejects(scene, starts.reshape(-1, 3), ends.reshape(-1, 3), k).reshape(S * H, S * W)
    n = int(dc.differ(sc.to_rgba8(moving["rgb"]), sc.to_rgba8(frozen["rgb"])).sum())
    print(f"fast small sphere: {int(on.sum())} samples hit it, {int((on & rej).sum())} where the static filter record "
          f"rejects them; {n} pixels differ from the frozen frame")
    assert (on & rej).sum() >= 10 and n >= 10
    # the frozen sphere is not rejected where it is hit: the restated filter is the kernel's
    on0 = mc.primary_hits_sphere(scene, cam, W, H, S, 0.0, d, k)
    assert on0.any() and not (on0 & rej).any()


@pytest.mark.parametrize("S", [2, 8])
def test_nan_frame_condition(S):
    e = mc.expected("tree_c2", W, H, S, 0.0, 0.0, 1.0, MOVES["tree_c2"])
    n = int(np.isnan(e["rgb"]).any(axis=2).sum())
    print(f"tree_c2 S={S}: {n} NaN pixels of {W * H}")
    assert e["depth"] == 3 and 0 < n <= 0.25 * W * H


# the CLI -----------------------------------------------------------------------------------------------------
def test_cli_usage_errors(tmp_path):
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    mv = ["--move", "0:40,0,0"]
    for args, word in ((["--shutter", "1"] + mv, "--shutter"),
                       (["--samples", "2", "--shutter", "1", "--adaptive", "32"], "--shutter"),
                       (["--samples", "2", "--shutter", "1", "--faithful", "glibc"], "--shutter"),
                       (["--samples", "2", "--shutter", "1", "--gpus", "2"], "--shutter"),
                       (["--samples", "2", "--shutter", "-0.5"], "--shutter"),
                       (["--samples", "2", "--shutter", "1.5"], "--shutter"),
                       (["--samples", "2", "--shutter", "open"], "--shutter"),
                       (["--samples", "2", "--shutter", "1x"], "--shutter"),
                       (["--samples", "2", "--shutter", "nan"], "--shutter"),
                       (["--samples", "2", "--shutter", "inf"], "--shutter"),
                       (["--samples", "2"] + mv, "--move"),
                       (["--samples", "2", "--shutter", "1", "--move", "0:40,0"], "--move"),
                       (["--samples", "2", "--shutter", "1", "--move", "40,0,0"], "--move"),
                       (["--samples", "2", "--shutter", "1", "--move", "0:40,0,0,0"], "--move"),
                       (["--samples", "2", "--shutter", "1", "--move", "0:40,nan,0"], "--move"),
                       (["--samples", "2", "--shutter", "1", "--move", "-1:40,0,0"], "--move"),
                       (["--samples", "2", "--shutter", "1", "--move", "8:40,0,0"], "--move")):
        r = subprocess.run([exe, "--config", "c2", "--out", str(tmp_path / "x.ppm")] + args, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert word in r.stderr, (args, r.stderr)
        assert not (tmp_path / "x.ppm").exists()
