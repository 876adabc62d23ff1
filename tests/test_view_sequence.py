"""Conditions on the committed call sequences of tests/view_sequence_common.py (no GPU): they are deterministic and
pinned, they take every branch of the view cache often enough, every field of the view key is the one thing that keeps
a render from being a cached one often enough — for the fields that move geometry, on views where a stale sky verdict
would store the miss colour over a hit — and the comparison the GPU test makes rejects a single wrong bit.

The floors are conditions, not measurements: a sequence that misses one is lengthened or re-biased, the floor stays.
The census of every seed (branch counts, per-field counts, per-field discriminating counts) is printed: run with -s."""
import functools

import numpy as np
import pytest

from ray_tracer_fragment_shader_amd import scenes

from . import view_sequence_common as vs

ALL = [(name, seed) for name, seeds in vs.SEEDS.items() for seed in seeds]
IDS = [f"{name}-{seed}" for name, seed in ALL]

# a vocabulary or generator edit changes these: a conscious act
DIGESTS = {117: "2cabeda423d3f2b7", 219: "af70e6f8f5e0d597", 245: "6e44bc1384d852b3", 326: "9c389f7d0cfe0641",
           364: "5f7b41c2c32cc151", 372: "454fae63a61599db", 438: "aa84e810217723b0", 458: "43e3fe2929cd0f5b",
           360: "a784c78944e4afc9", 471: "55e9e167e5775982", 511: "2b6109048c2b0ff7"}


def _knobs(name):
    return vs.MOVING_KNOBS if name == "moving_order" else {}


@functools.lru_cache(maxsize=None)
def _census(name, seed):
    """-> (steps, branch counts, {field: steps only that field keeps from being cached}, {field: the discriminating
    ones of them}, {call kind: cached renders}, (set-scene no-ops, captures, replays))."""
    steps = vs.generate(seed)
    knobs = _knobs(name)
    fields = {f: vs.forgotten(steps, f, **knobs) for f in vs.KEY_FIELDS}
    discr = {f: [k for k, stale, new in fields[f] if vs.discriminating(steps[k], stale, new)]
             for f in vs.DISCRIMINATING_FIELDS}
    kinds = dict.fromkeys(vs.CALL_KINDS, 0)
    for s, r in zip(steps, vs.trace(steps, **knobs)):
        if r["branch"] == "cached":
            kinds[vs.call_kind(s)] += 1
    scene, noops = None, 0
    for s in steps:
        if s["op"] == "set_scene":
            noops += s["scene"] == scene
            scene = s["scene"]
    misc = (noops, sum(s["op"] == "capture" for s in steps), sum(s["op"] == "replay" for s in steps))
    return steps, vs.branch_counts(steps, **knobs), fields, discr, kinds, misc


def _total(pick):
    out = {}
    for name, seed in ALL:
        for k, v in pick(_census(name, seed)).items():
            out[k] = out.get(k, 0) + (v if isinstance(v, int) else len(v))
    return out


@pytest.mark.parametrize("name,seed", ALL, ids=IDS)
def test_sequences_are_deterministic_and_pinned(name, seed):
    a, b = vs.generate(seed), vs.generate(seed)
    assert a == b and len(a) == vs.STEPS
    assert vs.digest(a) == DIGESTS[seed], f"seed {seed}: the sequence changed (digest {vs.digest(a)})"
    assert a[0] == {"op": "set_scene", "scene": "c2"}
    for s in a:                                         # every step is in the vocabulary
        if "size" in s:
            assert tuple(s["size"]) in vs.SIZES and tuple(s["cam_size"]) in vs.SIZES and s["cam"] in vs.CAMS
            assert s["depth"] in vs.DEPTHS and s["outs"] in vs.OUTSETS and s["stream"] in (0, 1, 2)
            assert (tuple(s["rows"]) if s["rows"] else None) in vs.ROWS and s["scene"] in vs.SCENES


def test_replays_come_late_and_in_the_scene_of_their_capture():
    for name, seed in ALL:
        steps = vs.generate(seed)
        for k, s in enumerate(steps):
            if s["op"] != "replay":
                continue
            cap = [j for j in range(k) if steps[j]["op"] == "capture" and steps[j]["slot"] == s["slot"]]
            assert len(cap) == 1 and k - cap[0] >= vs.REPLAY_AFTER, (seed, k)
            assert dict(steps[cap[0]], op="replay") == s
            assert not any(t["op"] == "set_scene" and t["scene"] != s["scene"] for t in steps[cap[0]:k]), (seed, k)


@pytest.mark.parametrize("name,seed", ALL, ids=IDS)
def test_branch_floor_of_every_seed(name, seed):
    _, branches, fields, discr, kinds, misc = _census(name, seed)
    print(f"\nseed {seed} ({name}): branches {branches}\n  per field {({f: len(v) for f, v in fields.items()})}\n"
          f"  discriminating {({f: len(v) for f, v in discr.items()})}\n  cached renders per call {kinds}\n"
          f"  set-scene no-ops, captures, replays {misc}")
    for b in vs.BRANCHES:
        assert branches[b] >= 3, f"seed {seed}: {branches[b]} steps of branch {b}"


def test_branch_floor_of_all_seeds():
    tot = _total(lambda c: c[1])
    print(f"\nall seeds: branches {tot}")
    for b in vs.BRANCHES:
        assert tot[b] >= 30, f"{tot[b]} steps of branch {b}"


def test_every_call_is_rendered_from_the_cache():
    tot = _total(lambda c: c[4])
    print(f"\nall seeds: cached renders per call {tot}")
    for k in vs.CALL_KINDS:
        assert tot[k] >= 3, f"{k}: {tot[k]} cached renders"
    noops, captures, replays = (sum(_census(*a)[5][i] for a in ALL) for i in range(3))
    print(f"all seeds: {noops} set-scene no-ops, {captures} captures, {replays} replays")
    assert noops >= 3 and captures >= 3 and replays >= 3


def test_sampled_calls_and_streams_occur():
    ops = [s["op"] for a in ALL for s in vs.generate(a[1])]
    for op in vs.SAMPLED_OPS + ("tile_order",):
        assert ops.count(op) >= 3, op
    streams = {s["stream"] for a in ALL for s in vs.generate(a[1]) if "stream" in s}
    assert streams == {0, 1, 2}


def test_field_floors():
    tot = _total(lambda c: c[2])
    print(f"\nall seeds: steps only the field keeps from being cached {tot}")
    for f in vs.KEY_FIELDS:
        assert tot[f] >= 3, f"{f}: {tot[f]} steps where only it tells the new view from the calibrated one"


def test_discrimination_floors():
    tot = _total(lambda c: c[3])
    print(f"\nall seeds: discriminating steps {tot}")
    for f in vs.DISCRIMINATING_FIELDS:
        assert tot[f] >= 2, f"{f}: {tot[f]} steps where a stale sky verdict would show"


@pytest.mark.parametrize("cam", vs.EYE_FIXED + ("below", "steep"))
def test_camera_variants_discriminate_at_64x40(cam):
    """Every eye-fixed variant, and the two moved eyes chosen for it, renders c2 at 64 x 40 with a hit in a tile the
    canonical view proves sky: a stale verdict there stores the miss colour over geometry.  (Orbit eye 3, the eye the
    older cache tests move to, does not.)  The doubled pitch shows a wider view, with more sky: it discriminates on the
    way back."""
    base = {"op": "render", "scene": "c2", "size": [64, 40], "cam_size": [64, 40], "cam": "base", "depth": 1, "rows": None,
            "outs": "all", "fmt": "native", "stream": 0}
    stale = vs.plan(base)
    assert int(vs.sky_verdict(stale).sum()) == 15
    new = dict(base, cam=cam)
    if cam == "pitch_double":
        assert not vs.discriminating(new, stale, vs.plan(new)) and vs.discriminating(base, vs.plan(new), stale)
        return
    assert vs.discriminating(new, stale, vs.plan(new))
    assert not vs.discriminating(dict(base, cam="orbit3"), stale, vs.plan(dict(base, cam="orbit3")))


def test_the_true_model_forgets_nothing():
    """Every step some forgetful model calls cached while the true one does not is a step whose view differs from the
    calibrated one: its key differs from the true model's calibrated key."""
    for name, seed in ALL:
        steps = vs.generate(seed)
        for f in vs.KEY_FIELDS:
            for k, stale, new in vs.forgotten(steps, f, **_knobs(name)):
                assert stale is not None and new is not None


def test_model_on_the_documented_path():
    """First, calibration, cached; another camera and back; a scene swap; the same scene set again; RT_MOVING_ORDER=1
    with RT_RECALIBRATE=3."""
    base = {"op": "render", "scene": "c2", "size": [64, 40], "cam_size": [64, 40], "cam": "base", "depth": 1, "rows": None,
            "outs": "all", "fmt": "native", "stream": 0}
    set_c2 = {"op": "set_scene", "scene": "c2"}
    other = dict(base, cam="look_a")
    m = vs.Model()
    got = [m.step(s) for s in [set_c2, base, base, base, other, other, other, base, base, set_c2, base,
                               {"op": "set_scene", "scene": "c1"}, base | {"scene": "c1"}, base | {"scene": "c1"}]]
    assert [r["branch"] for r in got] == [None, "first", "calibration", "cached", "other", "calibration", "cached",
                                          "other", "calibration", None, "cached", None, "first", "calibration"]
    assert [r["prepare"] for r in got[1:9]] == [True] + [False] * 7            # look_a keeps the eye
    assert got[2]["cone"] and got[2]["lmask"] and not got[13]["cone"]           # c1: 3 spheres, no masks
    assert got[12]["prepare"] and not got[10]["prepare"]                         # a new scene; the same scene again
    m = vs.Model(**vs.MOVING_KNOBS)
    got = [m.step(s) for s in [set_c2, base, base, base, other, other, other, other, base]]
    assert [r["branch"] for r in got] == [None, "first", "calibration", "cached", "other", "other", "other", "cached",
                                          "other"]
    assert [r["calibrate"] for r in got[4:8]] == [False, False, True, False] and not got[6]["cone"]
    m = vs.Model()
    cap = dict(base, op="capture", slot=0, stream=1)
    got = [m.step(s) for s in [set_c2, base, base, cap, base, dict(cap, op="replay"), base]]
    assert [r["branch"] for r in got] == [None, "first", "calibration", "captured", "cached", None, "cached"]
    assert [r["prepare"] for r in got[1:]] == [True, False, True, True, False, True]


def _frame():
    s = {"op": "render", "scene": "c2", "size": [64, 40], "cam_size": [64, 40], "cam": "base", "depth": 1, "rows": None,
         "outs": "all", "fmt": "native", "stream": 0}
    want = vs.expected(s)
    return want, {k: want[k].copy() for k in vs.OUTS}


def test_check_step_accepts_the_expected_frame():
    want, got = _frame()
    vs.check_step(got, want, {k: v.copy() for k, v in got.items()}, "step 0 (first)")


@pytest.mark.parametrize("name", ["rgb64f", "rgba32f"])
def test_check_step_rejects_one_flipped_mantissa_bit(name):
    want, got = _frame()
    bits = got[name].view(np.uint64 if name == "rgb64f" else np.uint32)
    bits[17, 23, 1] ^= 1
    with pytest.raises(AssertionError, match=f"step 5 \\(cached\\): {name} differs from the oracle, first at row 17, column 23"):
        vs.check_step(got, want, None, "step 5 (cached)")


def test_check_step_rejects_one_wrong_counter_and_one_wrong_byte():
    want, got = _frame()
    got["raycount"][3, 60] += 1
    with pytest.raises(AssertionError, match="raycount differs from the oracle, first at row 3, column 60"):
        vs.check_step(got, want, None)
    want, got = _frame()
    got["rgba8"][39, 0, 2] ^= 1
    with pytest.raises(AssertionError, match="rgba8 differs from the oracle, first at row 39, column 0"):
        vs.check_step(got, want, None)


def test_check_step_rejects_one_sentinel_pixel_and_a_differing_twin():
    for name in vs.OUTS:
        want, got = _frame()
        got[name].view(np.uint8).reshape(40, 64, -1)[20, 31] = vs.SENTINEL
        with pytest.raises(AssertionError, match=f"{name}: pixels no wave wrote .*first at row 20, column 31"):
            vs.check_step(got, want, None)
    want, got = _frame()
    twin = {k: v.copy() for k, v in got.items()}
    twin["rgba8"][1, 2, 0] ^= 1
    with pytest.raises(AssertionError, match="rgba8 differs from the twin's bytes, first at row 1, column 2"):
        vs.check_step(got, want, twin)


def test_check_step_compares_nans_by_position():
    want, got = _frame()
    want = dict(want, rgb64f=want["rgb64f"].copy())
    want["rgb64f"][5, 5, 0] = np.nan
    got["rgb64f"][5, 5, 0] = -np.nan
    vs.check_step({"rgb64f": got["rgb64f"]}, want, None)
    got["rgb64f"][5, 6, 0] = np.nan
    with pytest.raises(AssertionError, match="row 5, column 6"):
        vs.check_step({"rgb64f": got["rgb64f"]}, want, None)


# (rt_render_ss_dev renders one frame per call)
BANDED = [(op, r) for op in ("render", "render_ss", "render_packed", "render_host") for r in vs.ROWS
          if r and not (op == "render_ss" and r[3] > 1)]


@pytest.mark.parametrize("op,rows", BANDED, ids=[f"{op}-{'-'.join(map(str, r))}" for op, r in BANDED])
def test_banded_expectation_is_the_rows_of_the_full_frame(op, rows):
    W, H = 61, 37
    s = {"op": op, "scene": "c5", "size": [W, H], "cam_size": [W, H], "cam": "look_b", "depth": 2, "rows": list(rows),
         "outs": "parity" if op == "render_host" else "bytes" if op == "render_packed" else "all", "fmt": "native",
         "stream": 0}
    band, full = vs.expected(s), vs.expected(dict(s, rows=None))
    band_h, n, rank, frames = rows
    mine = [r for r in range(H) if (r // band_h) % n == rank] * frames
    assert len(mine) == scenes.local_rows(H, vs.rows_of(rows))
    for k in band:
        if k != "grid_rc":
            assert np.array_equal(band[k], full[k][mine], equal_nan=True), k
