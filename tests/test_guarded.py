"""The guard-band helper (tests/guarded.py) on CPU memory: its check() fails where it should, with the right offsets,
and passes where it should."""
import re

import numpy as np
import pytest
import torch

from tests import guarded


def _offsets(excinfo):
    m = re.search(r"first at offset (-?\d+), last at offset (-?\d+)", str(excinfo.value))
    assert m, str(excinfo.value)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("nbytes", [0, 1, 260, 256, 4096 + 8])
def test_carve_layout_and_alignment(nbytes):
    inner, check = guarded.carve(nbytes, "cpu")
    assert inner.dtype == torch.uint8 and inner.numel() == nbytes
    if nbytes:
        assert inner.data_ptr() % 256 == 0
    check()
    inner.fill_(0xFF)   # every payload byte may change
    check()


def test_check_fails_one_byte_before_and_one_byte_after():
    g = guarded.Guarded(260, "cpu", name="probe")
    assert g.whole.numel() == 2 * guarded.BAND + 512 and g.data_ptr() % 256 == 0
    assert (g.whole[:g.band] == guarded.PATTERN).all() and (g.whole[g.band + 260:] == guarded.PATTERN).all()
    g.check()
    g.raw[0] = 1
    g.raw[259] = 2
    g.check()                                   # writes inside are not damage
    g.whole[g.band - 1] = 0                     # one byte in front of the payload
    with pytest.raises(AssertionError) as e:
        g.check()
    assert _offsets(e) == (-1, -1) and "probe" in str(e.value)
    g.whole[g.band - 1] = guarded.PATTERN
    g.check()
    g.whole[g.band + 260] = 0                   # one byte behind it: inside the pad to 512, still guarded
    with pytest.raises(AssertionError) as e:
        g.check()
    assert _offsets(e) == (260, 260)
    g.whole[g.band - 1] = 7
    g.whole[-1] = 7                             # the last byte of the rear band
    with pytest.raises(AssertionError) as e:
        g.check()
    assert _offsets(e) == (-1, 512 + guarded.BAND - 1)
    assert "3 guard bytes" in str(e.value)


def test_a_write_that_restores_the_pattern_value_elsewhere_is_still_seen():
    """The far ends of both bands are checked, not only the bytes next to the payload."""
    g = guarded.Guarded(64, "cpu")
    g.whole[0] = 0
    with pytest.raises(AssertionError) as e:
        g.check()
    assert _offsets(e) == (-guarded.BAND, -guarded.BAND)


def test_typed_carves():
    g = guarded.carve_array((5, 3), torch.float32, "cpu", name="f32")
    assert g.t.shape == (5, 3) and g.t.dtype == torch.float32 and g.nbytes == 60
    g.fill(0xFF)
    assert torch.isnan(g.t).all()
    g.t[4, 2] = 1.0                             # the last element is inside
    g.check()
    flat = g.whole[g.band:].view(torch.float32)
    flat[15] = 1.0                              # one element past the end
    with pytest.raises(AssertionError) as e:
        g.check()
    assert _offsets(e) == (60, 63)
    src = np.arange(7, dtype=np.int64)
    h = guarded.carve_from(src, "cpu")
    assert h.t.dtype == torch.int64 and np.array_equal(h.t.numpy(), src) and np.array_equal(h.numpy(np.int64), src)
    h.check()
    empty = guarded.carve_array((0, 3), torch.float64, "cpu")
    assert empty.t.shape == (0, 3) and empty.data_ptr() % 256 == 0
    empty.check()
