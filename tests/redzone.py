"""Red zones, poisoned outputs and decoy calls ("Sanitizers
on the device side").  Plain numpy plus ldpc_amd.DeviceBuffer.

A guard is one allocation laid out as  band | shift | payload | band.  Both
bands hold BAND_BYTE; the payload holds POISON (an output) or the caller's data
(an input).  After the call under test:
  check_bands()      every band byte is unchanged -- a store one element past
                     the payload, or one before it, lands in a band of the same
                     allocation and is named by its offset from the payload;
  check_unchanged(x) an input still holds x's bytes;
  check_poison(...)  a part of an output the call must not write still holds
                     POISON.
An output is poisoned with a byte pattern that is no legal value where the type
allows it (u8 bits and flags are 0 / 1, 0xA5A5A5A5 is a negative int32), so a
row the call never stored differs from every reference; for fp64 and int8 the
exact comparison with the reference does that work.

BAND is four times the largest single wave-wide store in the tree (64 lanes x
16 B = 1 KiB): a stray whole-wave store stays inside the allocation.

decoy_then() runs a call on other inputs of the same shapes first, so whatever
the library keeps between calls (staging halves, expanded priors, workspaces)
is wrong data for the checked call.
"""
import ctypes as C

import numpy as np

BAND = 4096
BAND_BYTE = 0x5C
POISON = 0xA5
POISON_I32 = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]  # negative: no iteration count


def first_difference(got, want):
    """Index of the first differing byte of two equal-length uint8 arrays, or -1."""
    d = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return int(d[0]) if d.size else -1


def nonconstant(a, what=""):
    """The expected output must not be constant: stale or poisoned data then differs visibly."""
    a = np.ascontiguousarray(a)
    assert a.size > 1 and len(np.unique(a.view(np.uint64) if a.dtype == np.float64 else a)) > 1, \
        f"{what}: the reference output is constant"


class _Guard:
    """Layout and checks shared by the host and the device guard; subclasses
    give _read(offset, nbytes) -> uint8 array and _write(offset, uint8 array)."""

    def _layout(self, nbytes, shift, name):
        assert nbytes >= 0 and 0 <= shift < BAND
        self.nbytes, self.shift, self.name = int(nbytes), int(shift), name
        self.offset = BAND + self.shift           # of the payload within the allocation
        self.total = self.offset + self.nbytes + BAND

    def _init(self, data):
        self._write(0, np.full(self.offset, BAND_BYTE, np.uint8))
        self._write(self.offset + self.nbytes, np.full(BAND, BAND_BYTE, np.uint8))
        self.fill(data)

    def fill(self, data=None):
        """Poison the payload, or load it with data's bytes."""
        if data is None:
            b = np.full(self.nbytes, POISON, np.uint8)
        else:
            b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            assert b.size == self.nbytes, (self.name, b.size, self.nbytes)
        if self.nbytes:
            self._write(self.offset, b)

    def payload(self, dtype=np.uint8, shape=None):
        """A copy of the payload as dtype / shape."""
        a = np.array(self._read(self.offset, self.nbytes), copy=True).view(dtype)
        return a if shape is None else a.reshape(shape)

    def check_bands(self):
        lo = self._read(0, self.offset)
        hi = self._read(self.offset + self.nbytes, BAND)
        k = first_difference(lo, BAND_BYTE)
        assert k < 0, (f"{self.name}: byte at payload offset {k - self.offset} (before the payload) changed "
                       f"from {BAND_BYTE:#x} to {int(lo[k]):#x}")
        k = first_difference(hi, BAND_BYTE)
        assert k < 0, (f"{self.name}: byte at payload offset {self.nbytes + k} ({k} past the payload's end) changed "
                       f"from {BAND_BYTE:#x} to {int(hi[k]):#x}")

    def check_unchanged(self, original):
        want = np.ascontiguousarray(original).reshape(-1).view(np.uint8)
        assert want.size == self.nbytes, (self.name, want.size, self.nbytes)
        k = first_difference(self.payload(), want)
        assert k < 0, f"{self.name}: input byte at payload offset {k} changed"
        self.check_bands()

    def check_poison(self, start=0, stop=None):
        """Payload bytes [start, stop) still hold POISON."""
        stop = self.nbytes if stop is None else stop
        k = first_difference(self.payload()[start:stop], POISON)
        assert k < 0, f"{self.name}: byte at payload offset {start + k} was written (poison expected)"


class HostGuard(_Guard):
    """A guarded numpy array: .view is the typed payload (for ctypes: .ptr)."""

    def __init__(self, shape, dtype, shift=0, pinned=False, data=None, name="host"):
        self.dtype = np.dtype(dtype)
        self.shape = tuple(np.atleast_1d(shape).tolist()) if not isinstance(shape, tuple) else shape
        self._layout(int(np.prod(self.shape)) * self.dtype.itemsize, shift, name)
        if pinned:
            import ldpc_amd
            self.raw = ldpc_amd.host_empty(self.total, np.uint8)
        else:
            self.raw = np.empty(self.total, np.uint8)
        self._init(data)

    def _read(self, offset, nbytes):
        return self.raw[offset:offset + nbytes]

    def _write(self, offset, b):
        self.raw[offset:offset + b.size] = b

    @property
    def view(self):
        """The payload in place, typed (unaligned when shift is no multiple of the item size)."""
        return self.raw[self.offset:self.offset + self.nbytes].view(self.dtype).reshape(self.shape)

    @property
    def ptr(self):
        return C.c_void_p(self.raw.ctypes.data + self.offset)


class DeviceGuard(_Guard):
    """One DeviceBuffer of BAND + shift + nbytes + BAND bytes; .ptr is the payload."""

    def __init__(self, L, device, nbytes, shift=0, data=None, name="device"):
        self._layout(nbytes, shift, name)
        self.buf = L.DeviceBuffer(device, self.total)
        self._init(data)

    def _read(self, offset, nbytes):
        return self.buf.download(np.empty(nbytes, np.uint8), offset)

    def _write(self, offset, b):
        self.buf.upload(b, offset)

    @property
    def ptr(self):
        return self.buf.at(self.offset)

    def free(self):
        self.buf.free()


def decoy_then(call, decoy_inputs, real_inputs):
    """call(*decoy_inputs) into its own guarded buffers, then call(*real_inputs):
    the checked call's result.  The decoy's inputs have the real ones' shapes
    and come from another seed."""
    assert len(decoy_inputs) == len(real_inputs)
    for d, r in zip(decoy_inputs, real_inputs):
        if isinstance(r, np.ndarray):
            assert d.shape == r.shape and d.dtype == r.dtype and not np.array_equal(d, r)
        else:  # a seed or a key that selects the input
            assert d != r
    call(*decoy_inputs)
    return call(*real_inputs)
