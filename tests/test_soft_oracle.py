"""Soft shadows on the CPU: the two new symbols (the ABI version stays 10), the pins of the contract on its numpy
restatement (tests/soft_common.py), the fixtures made from the reference build (tests/golden/soft.npz), the
conditions that make the GPU tests sensitive to the light size and to the shadow test's filter, and the CLI's usage
errors.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from ray_tracer_fragment_shader_amd import abi, scenes

from . import dof_common as dc
from . import soft_common as so
from . import ssaa_common as sc

W, H = 37, 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_abi_version():
    L = abi.lib()
    assert L.rt_abi_version() == 10 and abi.ABI_VERSION == 10
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_api.h")).read(), flags=re.S)
    for name in ("rt_render_soft_dev", "rt_render_soft"):
        assert hasattr(L, name), name
        assert name in abi.SIGNATURES
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    assert len(abi.SIGNATURES["rt_render_soft_dev"][1]) == 13 and len(abi.SIGNATURES["rt_render_soft"][1]) == 13


# pins of the contract on the restatement ---------------------------------------------------------------------
def _negative_zero(v):
    return v == 0.0 and np.signbit(v)


def test_no_light_has_a_negative_zero():
    """The pins assume it (rule 5): L + (+-0) is L only then."""
    for name in ("c2", "c5", "demo", "tree_demo", "tree_c2"):
        scene, _ = sc.scene_of(name)
        assert not any(_negative_zero(v) for v in so.centres_of(scene).ravel()), name
    for name, S, R, A, centres in so.FIXTURES:
        assert not any(_negative_zero(v) for p in centres for v in p), name
        scene, _ = sc.scene_of(name)
        assert len(centres) == len(scene.lights)
        for b in range(S):
            for a in range(S):
                assert not any(_negative_zero(v) for v in so.displaced(centres, S, R, a, b).ravel()), (name, a, b)


def test_panel_points():
    """Rule 2 on a case worked by hand: S = 4, R = 80 around (40, 200, -80)."""
    c = ((40.0, 200.0, -80.0),)
    xs = [so.displaced(c, 4, 80.0, a, 0)[0, 0] for a in range(4)]
    zs = [so.displaced(c, 4, 80.0, 0, b)[0, 2] for b in range(4)]
    assert xs == [-20.0, 20.0, 60.0, 100.0] and zs == [-140.0, -100.0, -60.0, -20.0]
    assert all(so.displaced(c, 4, 80.0, a, b)[0, 1] == 200.0 for a in range(4) for b in range(4))
    assert so.displaced(c, 1, 80.0, 0, 0).tolist() == [[40.0, 200.0, -80.0]]
    assert so.square_of_light((60.0, 200.0, -60.0)) == "b6"


@pytest.mark.parametrize("name,S", [("c2", 2), ("c5", 4), ("demo", 8), ("tree_demo", 2), ("tree_c2", 2)])
def test_light_size_zero_is_the_lens_frame(name, S):
    e, want = so.expected(name, W, H, S, 8.0, 0.0), dc.expected(name, W, H, S, 8.0)
    sc.assert_same_bits(e["hi"], want["hi"], f"{name} S={S} samples")
    assert np.array_equal(e["hi_rc"], want["hi_rc"])
    sc.assert_same_bits(e["rgb"], want["rgb"], f"{name} S={S}")
    assert np.array_equal(e["rc2"], want["rc2"])


@pytest.mark.parametrize("name,S", [("c2", 2), ("c5", 4), ("demo", 8), ("tree_demo", 2), ("tree_c2", 2)])
def test_both_zero_is_the_supersampled_frame(name, S):
    e, want = so.expected(name, W, H, S, 0.0, 0.0), sc.expected(name, W, H, S)
    sc.assert_same_bits(e["hi"], want["hi"], f"{name} S={S} samples")
    assert np.array_equal(e["hi_rc"], want["hi_rc"])
    sc.assert_same_bits(e["rgb"], want["rgb"], f"{name} S={S}")
    assert np.array_equal(e["rc2"], want["rc2"])


@pytest.mark.parametrize("name,S", sc.FIXTURES)
def test_both_zero_is_the_ssaa_fixture(name, S):
    e = so.expected(name, sc.FIX_W, sc.FIX_H, S, 0.0, 0.0)
    sc.assert_same_bits(e["rgb"], sc.fixtures()[sc.fixture_key(name, S)], f"{name} S={S}")


@pytest.mark.parametrize("name,S", dc.FIXTURES)
def test_light_size_zero_is_the_dof_fixture(name, S):
    e = so.expected(name, dc.FIX_W, dc.FIX_H, S, dc.FIX_A, 0.0)
    sc.assert_same_bits(e["rgb"], dc.fixtures()[sc.fixture_key(name, S)], f"{name} S={S}")


@pytest.mark.parametrize("name", ["c2", "demo"])
def test_one_sample_is_the_plain_render(name):
    e = so.expected(name, W, H, 1, 8.0, 40.0)
    scene, depth = sc.scene_of(name)
    rgb, rc = po.render(scene.to_abi(), e["cam"], W, H, depth)
    sc.assert_same_bits(e["rgb"], rgb, name)
    assert np.array_equal(e["rc2"], sc.reduce_counts(rc, 1))


# fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,R,A,centres", so.FIXTURES)
def test_oracle_route_reproduces_fixture(name, S, R, A, centres):
    fx = so.fixtures()
    assert sorted(fx) == sorted(so.fixture_key(n, s) for n, s, _, _, _ in so.FIXTURES), "recorded colours only"
    want = fx[so.fixture_key(name, S)]
    assert want.shape == (so.FIX_H, so.FIX_W, 3) and want.dtype == np.float64
    e = so.expected(name, so.FIX_W, so.FIX_H, S, A, R, centres)
    sc.assert_same_bits(e["rgb"], want, f"{name} S={S}")
    if name == "tree_c2":
        assert np.isnan(want).any(), "the NaN fixture has no NaN"


@pytest.mark.ref
@pytest.mark.parametrize("name,S,R,A,centres", so.FIXTURES)
def test_reference_build_reproduces_fixture(name, S, R, A, centres):
    if not po.ref_available():
        pytest.skip("no reference build here")
    scene, depth = sc.scene_of(name)
    cam = scenes.make_camera(so.FIX_W, so.FIX_H, 500.0 / so.FIX_W)
    got = so.render_ref(scene, cam, so.FIX_W, so.FIX_H, depth, S, A, R, centres)
    sc.assert_same_bits(got, so.fixtures()[so.fixture_key(name, S)], f"{name} S={S}")


# sensitivity: a kernel that ignores the light size cannot pass the GPU tests -----------------------------------
@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("name", ["c2", "c5", "demo", "tree_demo"])
def test_light_size_changes_the_frame(name, S):
    """(Measured on the oracle when the contract was written: c2 37.1-43.8 % of the pixels in rgb64f and 27.8-33.5 %
    in RGBA8, c5 54.8-63.8 % / 45.4-53.9 %, demo and tree_demo 31.7-38.1 % / 22.8-28.1 %.)"""
    e, e0 = so.expected(name, W, H, S, 0.0, 40.0), so.expected(name, W, H, S, 0.0, 0.0)
    f64 = dc.differ(e["rgb"], e0["rgb"]).mean()
    u8 = dc.differ(sc.to_rgba8(e["rgb"]), sc.to_rgba8(e0["rgb"])).mean()
    print(f"{name} S={S}: rgb64f differs in {100 * f64:.1f} % of the pixels, rgba8 in {100 * u8:.1f} %")
    assert f64 >= 0.25
    assert u8 >= 0.18


# penumbra: a kernel that moves the light but keeps the point light's cone filter cannot pass --------------------
@pytest.mark.parametrize("S", [2, 4, 8])
def test_penumbra_samples(S):
    """c2's scene at depth 0: the samples whose shadowed state differs between R = 40 and R = 0 are the ones whose
    shadow ray meets another set of blockers than the ray to the stored light position.  (Measured: 48 samples in
    33 pixels at S = 2, 215 in 62 at S = 4, 884 in 74 at S = 8.)"""
    e, e0 = so.expected("c2", W, H, S, 0.0, 40.0, None, 0), so.expected("c2", W, H, S, 0.0, 0.0, None, 0)
    assert np.array_equal(e["hi_rc"], e0["hi_rc"]), "depth 0: the rays traced do not depend on the light"
    flip = so.shadowed(e) != so.shadowed(e0)
    px = flip.reshape(H, S, W, S).any(axis=(1, 3))
    print(f"S={S}: {int(flip.sum())} samples in {int(px.sum())} pixels change their shadowed state")
    assert px.sum() >= 25


@pytest.mark.parametrize("S", [2, 8])
def test_nan_frame_condition(S):
    e = so.expected("tree_c2", W, H, S, 0.0, 40.0)
    n = int(np.isnan(e["rgb"]).any(axis=2).sum())
    print(f"tree_c2 S={S}: {n} NaN pixels of {W * H}")
    assert e["depth"] == 3 and 0 < n <= 0.25 * W * H


# the CLI -----------------------------------------------------------------------------------------------------
def test_cli_usage_errors(tmp_path):
    exe = os.path.join(os.path.dirname(abi.LIB_PATH), "rt_render")
    for args in (["--light-size", "40"], ["--samples", "2", "--light-size", "40", "--adaptive", "32"],
                 ["--samples", "2", "--light-size", "40", "--faithful", "glibc"],
                 ["--samples", "2", "--light-size", "40", "--gpus", "2"],
                 ["--samples", "2", "--light-size", "-1"], ["--samples", "2", "--light-size", "wide"],
                 ["--samples", "2", "--light-size", "40x"], ["--samples", "2", "--light-size", "nan"],
                 ["--samples", "2", "--light-size", "inf"]):
        r = subprocess.run([exe, "--config", "c2", "--out", str(tmp_path / "x.ppm")] + args, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert "--light-size" in r.stderr, args
        assert not (tmp_path / "x.ppm").exists()
