"""The tile-class decision on the CPU (rt_diag_tile_class_plan: the host evaluation of rt_cone.hpp tile_sphere_free, the
function the device's class kernel runs): a tile is sphere-free when it is not sky and neither its primary cone mask nor
any of its level-mask slots keeps one of the scene's spheres."""
import numpy as np
import pytest

from ray_tracer_fragment_shader_amd import abi

from .tile_classes_common import class_plan


def test_bits_at_or_above_the_sphere_count_are_ignored():
    np_ = 8
    cone = np.array([1 << 8, 1 << 63, 0xFFFFFFFFFFFFFF00, 0], np.uint64)
    masks = np.array([[1 << 9, 1 << 40], [0, 1 << 8], [0xFF00, 0], [0, 0]], np.uint64)
    assert class_plan(cone, None, masks, np_).tolist() == [1, 1, 1, 1]
    # ... and the bit just below it is not
    cone[0] = 1 << 7
    masks[1, 1] = 1 << 7
    assert class_plan(cone, None, masks, np_).tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("np_", [8, 12, 64])
def test_a_sphere_bit_in_the_cone_or_in_any_single_slot_clears_the_class(np_):
    slots = 5
    for bit in (0, np_ - 1):
        cone = np.zeros(slots + 2, np.uint64)
        masks = np.zeros((slots + 2, slots), np.uint64)
        cone[0] = np.uint64(1) << np.uint64(bit)                 # tile 0: the cone mask
        for k in range(slots):                                   # tile 1 + k: slot k alone (first .. last)
            masks[1 + k, k] = np.uint64(1) << np.uint64(bit)
        want = [0] * (slots + 1) + [1]                           # the last tile keeps nothing
        assert class_plan(cone, None, masks, np_).tolist() == want, (np_, bit)


def test_a_sky_tile_is_never_in_the_class():
    cone = np.zeros(4, np.uint64)
    masks = np.zeros((4, 3), np.uint64)
    sky = np.array([0, 1, 255, 0], np.uint8)
    assert class_plan(cone, sky, masks, 8).tolist() == [1, 0, 0, 1]
    assert class_plan(cone, sky, None, 8).tolist() == [1, 0, 0, 1]


def test_no_slots():
    cone = np.array([0, 1, 1 << 8, 1 << 7], np.uint64)
    assert class_plan(cone, None, None, 8).tolist() == [1, 0, 1, 0]
    assert class_plan(cone, None, np.zeros((4, 0), np.uint64), 8).tolist() == [1, 0, 1, 0]
    assert class_plan(np.zeros(0, np.uint64), None, None, 8).tolist() == []
    # no sphere at all: every tracing tile is in the class
    assert class_plan(np.array([~np.uint64(0)], np.uint64), None, None, 0).tolist() == [1]


def test_bad_arguments():
    L = abi.lib()
    cone = np.zeros(2, np.uint64)
    masks = np.zeros((2, 2), np.uint64)
    out = np.zeros(2, np.uint8)
    ok = (cone.ctypes.data, None, masks.ctypes.data, 2, 2, 8, out.ctypes.data)
    assert L.rt_diag_tile_class_plan(*ok) == abi.RT_OK

    def call(**kw):
        names = ("cone", "sky", "masks", "tiles", "slots", "n", "out")
        a = dict(zip(names, ok))
        a.update(kw)
        return L.rt_diag_tile_class_plan(*(a[k] for k in names))

    assert call(cone=None) == abi.RT_EINVAL
    assert call(out=None) == abi.RT_EINVAL
    assert call(masks=None) == abi.RT_EINVAL              # slots > 0 without masks
    assert call(masks=None, slots=0) == abi.RT_OK
    assert call(tiles=-1) == abi.RT_EINVAL
    assert call(slots=-1) == abi.RT_EINVAL
    assert call(n=-1) == abi.RT_EINVAL
    assert call(n=65) == abi.RT_EINVAL
    assert L.rt_diag_tile_classes(None, None, None, None) == abi.RT_EINVAL
    assert L.rt_diag_tile_class_grid(None, None, 0) == abi.RT_EINVAL
