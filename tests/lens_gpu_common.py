"""What tests/test_gpu_dof.py, test_gpu_soft.py and test_gpu_motion.py share: the fixtures `tr` and `fresh` (imported
by name), the frame size, the comparison of every output with an expected frame, and the bodies of the checks that are
the same for the three renders but for the render call, which the test passes in.  Expected values come from the
callers (the CPU oracle and the fixtures), never from the code under test."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from ray_tracer_fragment_shader_amd import abi, scenes  # noqa: E402
from ray_tracer_fragment_shader_amd.tracer import Tracer  # noqa: E402

from . import ssaa_common as sc  # noqa: E402

W, H = 37, 21
OUTS = ("rgba32f", "rgba8", "rgb64f", "raycount")
BAD = (-1.0, -1e-300, float("nan"), float("inf"), -float("inf"))


def _tracer():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    t = Tracer(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def tr():
    yield from _tracer()


@pytest.fixture()
def fresh():
    """A context of its own: the tests of the context's and the per-view state."""
    yield from _tracer()


def _host(bufs):
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}
    if "raycount" in out:
        out["raycount"] = out["raycount"].view(np.uint32)
    return out


def _check_all(got, rgb, rc2, what):
    """Every output of a render against the expected float64 frame and counters."""
    sc.assert_same_bits(got["rgb64f"], rgb, what + " rgb64f")
    sc.assert_same_bits(got["rgba32f"], sc.to_rgba32f(rgb), what + " rgba32f")
    assert np.array_equal(got["rgba8"], sc.to_rgba8(rgb)), what + " rgba8"
    assert got["raycount"].shape == rc2.shape and np.array_equal(got["raycount"], rc2), what + " raycount"


def _read_ppm(path):
    hdr, body = open(path, "rb").read().split(b"\n", 1)
    assert hdr.split() == [b"P6", str(W).encode(), str(H).encode(), b"255"]
    return np.frombuffer(body, np.uint8).reshape(H, W, 3)


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check_one_sample_is_the_plain_render(t, name, render, set_motion=None):
    """render(cam, depth) -> the S = 1 frame of the scene set here, every output on the host; set_motion(scene) runs
    after the scene is set, before the plain render."""
    scene, depth = sc.scene_of(name)
    t.set_scene(scene)
    if set_motion:
        set_motion(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    want, want_rc = po.render(scene.to_abi(), cam, W, H, depth)
    plain = _host(t.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True))
    assert plain["rgb64f"].tobytes() == want.tobytes()
    got = render(cam, depth)
    for k in ("rgba32f", "rgba8", "rgb64f"):
        assert got[k].tobytes() == plain[k].tobytes(), k
    assert np.array_equal(got["raycount"], sc.reduce_counts(want_rc, 1))


def check_nan_frame(got, e, S):
    """The render `got` of tree_c2's expected frame `e`: NaNs where expected, and byte 0 there."""
    assert np.array_equal(np.isnan(got["rgb64f"]), np.isnan(e["rgb"]))
    _check_all(got, e["rgb"], e["rc2"], f"tree_c2 S={S}")
    assert (got["rgba8"][..., :3][np.isnan(e["rgb"])] == 0).all()


def check_nullable_output(only, e, render):
    """render(**flags) -> the buffers of a render of the expected frame `e` with the outputs `flags` ask for."""
    got = _host(render(**{k: k == only for k in OUTS}))
    assert list(got) == [only]
    want = {"rgba32f": sc.to_rgba32f(e["rgb"]), "rgba8": sc.to_rgba8(e["rgb"]), "rgb64f": e["rgb"],
            "raycount": e["rc2"]}[only]
    assert got[only].shape == want.shape and got[only].tobytes() == want.tobytes()


def check_no_outputs_is_a_no_op(t, symbol, *extra):
    """The _dev entry point `symbol` with its doubles `extra` and no output pointer."""
    scene, depth = sc.scene_of("c2")
    t.set_scene(scene)
    cam = scenes.make_camera(W, H, 500.0 / W)
    rc = getattr(abi.lib(), symbol)(t._ctx, ctypes.byref(cam), W, H, depth, 2, *extra, None, None, None, None,
                                    stream_ptr())
    assert rc == abi.RT_OK
    torch.cuda.synchronize()


def check_graph_capture(t, e, depth, render_into):
    """render_into(bufs, stream): the render of the expected frame `e` by the context `t`, whose scene is set."""
    bufs = t.alloc_ss(W, H, None, rgba32f=True, rgba8=True, rgb64f=True, raycount=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        render_into(bufs, s)                                                     # warm-up outside the capture
    s.synchronize()
    _check_all(_host(bufs), e["rgb"], e["rc2"], "direct")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        render_into(bufs, s)
    for k in range(2):
        for b in bufs.values():
            if b is not None:
                b.zero_()
        g.replay()
        _check_all(_host(bufs), e["rgb"], e["rc2"], f"replay {k}")
        plain = _host(t.render(e["cam"], W, H, depth, rgb64f=True))              # another render in between
        assert plain["rgb64f"].shape == (H, W, 3)


def check_host_buffers(e, S, what, call):
    """call(rgba32f, rgba8, rgb64f, stats) -> the status of the host entry point `what` on the expected frame `e`, its
    four pointers as given.  -> the rgb64f array, for a further call."""
    f32 = np.zeros((H, W, 4), np.float32)
    u8 = np.zeros((H, W, 4), np.uint8)
    f64 = np.zeros((H, W, 3), np.float64)
    st = abi.rt_stats()
    abi.check(call(ctypes.c_void_p(f32.ctypes.data), ctypes.c_void_p(u8.ctypes.data), ctypes.c_void_p(f64.ctypes.data),
                   ctypes.byref(st)), what)
    sc.assert_same_bits(f64, e["rgb"], what + " rgb64f")
    sc.assert_same_bits(f32, sc.to_rgba32f(e["rgb"]), what + " rgba32f")
    assert np.array_equal(u8, sc.to_rgba8(e["rgb"]))
    seg, sh = int(e["rc2"][..., 0].sum(dtype=np.uint64)), int(e["rc2"][..., 1].sum(dtype=np.uint64))
    assert st.primary_rays == W * H * S * S
    assert st.reflect_rays == seg - W * H * S * S and st.shadow_rays == sh
    return f64


def check_view_unchanged(frames, later):
    """`later`, a render of the view of `frames` after other work, appended: every frame equals the first."""
    frames.append(later)
    for k, f in enumerate(frames[1:]):
        for key in OUTS:
            assert f[key].tobytes() == frames[0][key].tobytes(), (k + 1, key)


def view_frames(t, scene, cam, depth):
    """A view's first, calibration and cached renders by the context `t`, the first checked against the oracle."""
    want, want_rc = po.render(scene.to_abi(), cam, W, H, depth)
    frames = [_host(t.render(cam, W, H, depth, rgba32f=True, rgba8=True, rgb64f=True, raycount=True))
              for _ in range(3)]
    assert frames[0]["rgb64f"].tobytes() == want.tobytes()
    assert np.array_equal(frames[0]["raycount"], want_rc)
    return frames
