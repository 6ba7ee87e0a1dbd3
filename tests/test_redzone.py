"""The red-zone helper checked on the CPU: HostGuard must report a write one
byte past the payload, one byte before it, a write into an input, and leave an
untouched guard alone -- at every shift 0..7, with the offset it names counted
from the payload."""
import numpy as np
import pytest

import redzone as Z

SHIFTS = range(8)


def _raises(fn, *words):
    with pytest.raises(AssertionError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("shift", SHIFTS)
def test_layout_and_unchanged_band(shift):
    g = Z.HostGuard((5, 13), np.uint8, shift)
    assert g.raw.size == Z.BAND + shift + 65 + Z.BAND and g.offset == Z.BAND + shift
    assert g.ptr.value == g.raw.ctypes.data + Z.BAND + shift
    assert g.view.shape == (5, 13) and (g.view == Z.POISON).all()
    assert (g.raw[:g.offset] == Z.BAND_BYTE).all() and (g.raw[g.offset + 65:] == Z.BAND_BYTE).all()
    g.view[:] = 1  # the whole payload written: no finding
    g.check_bands()
    assert np.array_equal(g.payload(np.uint8, (5, 13)), np.ones((5, 13), np.uint8))


@pytest.mark.parametrize("shift", SHIFTS)
def test_one_byte_past_the_end(shift):
    g = Z.HostGuard(65, np.uint8, shift, name="hard")
    g.raw[g.offset + 65] = 0
    _raises(g.check_bands, "hard", "payload offset 65 ", "0 past")


@pytest.mark.parametrize("shift", SHIFTS)
def test_one_byte_before_the_start(shift):
    g = Z.HostGuard(65, np.uint8, shift, name="valid")
    g.raw[g.offset - 1] = 1
    _raises(g.check_bands, "valid", "payload offset -1 ")


@pytest.mark.parametrize("shift", SHIFTS)
def test_band_offsets_far_from_the_payload(shift):
    g = Z.HostGuard(7, np.int32, shift if shift % 4 == 0 else 4)
    g.raw[g.offset + 28 + 1000] = 9
    g.raw[g.offset + 28 + 2000] = 9  # the first one is named
    _raises(g.check_bands, "payload offset 1028 ", "1000 past")
    g = Z.HostGuard(7, np.uint8, shift)
    g.raw[0] = 9
    _raises(g.check_bands, f"payload offset {-(Z.BAND + shift)} ")
    g = Z.HostGuard(7, np.uint8, shift)
    g.raw[-1] = 9
    _raises(g.check_bands, f"payload offset {7 + Z.BAND - 1} ")


@pytest.mark.parametrize("shift", SHIFTS)
def test_changed_input(shift):
    x = np.arange(3 * 11, dtype=np.int8).reshape(3, 11)
    g = Z.HostGuard(x.shape, np.int8, shift, data=x, name="codes")
    assert np.array_equal(g.view, x)
    g.check_unchanged(x)
    g.view[2, 10] ^= 1
    _raises(lambda: g.check_unchanged(x), "codes", "payload offset 32 ")
    g.view[2, 10] ^= 1
    g.raw[g.offset + 33] = 0  # an input's band is checked with it
    _raises(lambda: g.check_unchanged(x), "payload offset 33 ")


@pytest.mark.parametrize("shift", SHIFTS)
def test_typed_views_and_poison(shift):
    g = Z.HostGuard(9, np.int32, shift)
    assert (g.view == Z.POISON_I32).all() and Z.POISON_I32 < 0
    g.check_poison()
    g.view[:4] = np.arange(4)
    g.check_poison(16)
    _raises(lambda: g.check_poison(12), "payload offset 12 ")
    assert np.array_equal(g.payload(np.int32)[:4], np.arange(4))
    d = Z.HostGuard((2, 3), np.float64, shift, data=np.arange(6.0).reshape(2, 3))
    assert np.array_equal(d.payload(np.float64, (2, 3)), np.arange(6.0).reshape(2, 3))
    d.fill()
    assert np.isnan(d.payload(np.float64)).sum() == 0 and (d.payload() == Z.POISON).all()


def test_nonconstant_and_first_difference():
    Z.nonconstant(np.array([0, 1, 1], np.uint8))
    _raises(lambda: Z.nonconstant(np.zeros(5, np.uint8), "hard"), "hard")
    _raises(lambda: Z.nonconstant(np.full(5, 2.5), "post"), "post")
    assert Z.first_difference(np.array([3, 3, 4], np.uint8), 3) == 2
    assert Z.first_difference(np.array([3, 3], np.uint8), np.array([3, 3], np.uint8)) == -1


def test_decoy_then_runs_the_decoy_first():
    seen = []

    def call(x):
        seen.append(int(x[0]))
        return x * 2

    out = Z.decoy_then(call, (np.array([5, 6]),), (np.array([1, 2]),))
    assert seen == [5, 1] and out.tolist() == [2, 4]
    _raises(lambda: Z.decoy_then(call, (np.array([1, 2]),), (np.array([1, 2]),)))  # the decoy must differ
