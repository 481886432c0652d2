"""Guard-banded buffers for tests that hand raw pointers to the C-ABI (TEST INFRASTRUCTURE ONLY).

A caching allocator rounds and pools allocations, so a kernel that writes one element, one row or one whole workspace
step past the end of `torch.empty(n)` lands in memory nobody looks at.  carve() puts the buffer in the middle of ONE
allocation whose other bytes hold a pattern, and check() proves the pattern is still there:

    [ band x 0xA5 | nbytes of payload | pad to `align` x 0xA5 | band x 0xA5 ]

The pad between the payload's end and the next multiple of `align` belongs to the guarded bytes, so an overrun of a
single element is seen even when the payload is not a multiple of `align`.  The band is 64 KiB: larger than any whole
workspace step of the shapes tests/test_gpu_bounds.py uses, so what these tests can detect stays inside the test's own
allocation.
"""
import numpy as np
import torch

PATTERN = 0xA5
BAND = 65536


def _round_up(n, a):
    return (int(n) + a - 1) // a * a


class Guarded:
    """One carve: `raw` is the uint8 view of exactly `nbytes` payload bytes, `t` the typed view (None for carve())."""

    def __init__(self, nbytes, device, band=BAND, align=256, name="buffer"):
        self.nbytes, self.band, self.name = int(nbytes), int(band), name
        self.padded = _round_up(self.nbytes, align)
        total = self.band + self.padded + self.band
        # `align` spare bytes so that the payload can start on a multiple of `align` wherever the allocation starts
        self._alloc = torch.empty(total + align, dtype=torch.uint8, device=device)
        skew = (-(self._alloc.data_ptr() + self.band)) % align
        self.whole = self._alloc[skew:skew + total]
        self.whole.fill_(PATTERN)
        self.raw = self.whole[self.band:self.band + self.nbytes]
        self.t = None
        assert self.data_ptr() % align == 0

    def data_ptr(self):
        """Address of the payload (valid and aligned also when the payload is empty)."""
        return self.whole.data_ptr() + self.band

    def fill(self, byte):
        self.raw.fill_(int(byte))
        return self

    def put(self, array):
        """Copies a numpy array's bytes into the payload (sizes must agree)."""
        src = np.ascontiguousarray(array)
        assert src.nbytes == self.nbytes, (self.name, src.nbytes, self.nbytes)
        if self.nbytes:
            self.raw.copy_(torch.from_numpy(src.reshape(-1).view(np.uint8).copy()))
        return self

    def bytes(self):
        return self.raw.cpu().numpy().copy()

    def numpy(self, dtype, shape=(-1,)):
        return self.bytes().view(dtype).reshape(shape)

    def check(self):
        """Both bands (and the pad) still hold the pattern everywhere; otherwise reports the first and the last damaged
        byte as offsets relative to the payload's first byte (negative: in front of it)."""
        lo = self.whole[:self.band].cpu().numpy()
        hi = self.whole[self.band + self.nbytes:].cpu().numpy()
        bad = np.concatenate([np.flatnonzero(lo != PATTERN) - self.band, np.flatnonzero(hi != PATTERN) + self.nbytes])
        assert bad.size == 0, ("%s: %d guard bytes damaged, first at offset %d, last at offset %d (payload is %d bytes)"
                               % (self.name, bad.size, int(bad[0]), int(bad[-1]), self.nbytes))


def carve(nbytes, device, band=BAND, align=256, name="buffer"):
    """(inner uint8 view of `nbytes` bytes with an `align`-aligned data_ptr(), check) inside one guarded allocation."""
    g = Guarded(nbytes, device, band, align, name)
    return g.raw, g.check


def carve_array(shape, dtype, device, band=BAND, align=256, name="array"):
    """A guarded array of a torch dtype: returns the Guarded, whose `t` is the typed view of `shape`."""
    shape = tuple(int(s) for s in np.atleast_1d(shape))
    item = torch.empty((), dtype=dtype).element_size()
    g = Guarded(int(np.prod(shape)) * item, device, band, align, name)
    g.t = g.raw.view(dtype).reshape(shape)
    return g


def carve_from(array, device, band=BAND, align=256, name="array"):
    """A guarded copy of a numpy array (same bytes, same shape)."""
    array = np.ascontiguousarray(array)
    g = carve_array(array.shape, torch.from_numpy(np.empty(0, array.dtype)).dtype, device, band, align, name)
    return g.put(array)
