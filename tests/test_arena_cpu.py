"""tests/arena.py on torch CPU tensors: the checker that tests/test_gpu_workspace_guard.py relies on reports what it should,
where it should, and nothing else."""
import numpy as np
import pytest
import torch

from tests.arena import GUARD, MIN_BAND, SENTINEL, Arena, Region, band_len

DTYPES = [torch.float64, torch.float32]


def _arena(dtype, m=0, offsets=(0, 1, 0)):
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    data = np.arange(37, dtype=np.float64 if dtype == torch.float64 else np.float32)
    return Arena(dtype, [Region("in", 37, offsets[0], "data", data), Region("work", 101, offsets[1] % vec, "poison"),
                         Region("out", 64, offsets[2], "sentinel")], m=m), data


@pytest.mark.parametrize("dtype", DTYPES)
def test_fills_and_a_clean_check(dtype):
    a, data = _arena(dtype)
    assert np.array_equal(a["in"].numpy(), data)
    assert torch.isnan(a["work"]).all() and a["work"].numel() == 101
    assert (a["out"] == SENTINEL).all() and a["out"].numel() == 64
    assert a.check() == []
    covered = sum(hi - lo for lo, hi, _, _ in a.bands()) + sum(a.bytes_of(n).numel() for n in a.names)
    assert covered == a.raw.numel()  # bands and regions tile the arena
    for lo, hi, _, _ in a.bands():
        assert (a.raw[lo:hi] == GUARD).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_offsets_land_where_asked(dtype):
    item = torch.empty((), dtype=dtype).element_size()
    vec = 16 // item
    for off in range(vec):
        a = Arena(dtype, [Region("a", 5, off), Region("b", 7, (off + 1) % vec), Region("c", 1, vec - 1 - off)])
        assert a["a"].data_ptr() % 16 == off * item
        assert a["b"].data_ptr() % 16 == (off + 1) % vec * item
        assert a["c"].data_ptr() % 16 == (vec - 1 - off) * item
        assert a.check() == []


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,want", [(0, MIN_BAND), (100, MIN_BAND), (2048, MIN_BAND), (4096, 8192), (16384, 32768)])
def test_bands_are_as_wide_as_stated(dtype, m, want):
    a, _ = _arena(dtype, m=m, offsets=(1, 3, 0))
    assert band_len(m) == want == a.band
    bands = a.bands()
    assert len(bands) == 4
    assert [(b, n) for _, _, b, n in bands] == [(None, "in"), ("in", "work"), ("work", "out"), ("out", None)]
    for lo, hi, _, _ in bands:
        elems = (hi - lo) // a.itemsize
        assert (hi - lo) % a.itemsize == 0 and want <= elems < want + a.vec, (lo, hi)
    # a band ends where its region begins and begins where the region before it ends
    for (_, hi, _, name), (lo, _, prev, _) in zip(bands[:-1], bands[1:]):
        assert name == prev
        first = a.bytes_of(name)
        assert first.data_ptr() - a.raw.data_ptr() == hi and hi + first.numel() == lo


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_flipped_band_byte_is_reported_with_its_region_and_side(dtype):
    a, _ = _arena(dtype, offsets=(0, 1, 3 % (16 // torch.empty((), dtype=dtype).element_size())))
    bands = a.bands()
    for lo, hi, before, after in bands:
        mid = lo if before is None else hi if after is None else (lo + hi) // 2
        spots = {lo, lo + 1, mid - 1, mid, hi - 2, hi - 1}  # first and last byte of the band and of either half
        for at in sorted(s for s in spots if lo <= s < hi):
            keep = int(a.raw[at])
            a.raw[at] = keep ^ 0x01
            want = (before, "after", at - lo, 1) if at < mid else (after, "before", at - hi, 1)
            assert a.check() == [want], (lo, hi, at)
            a.raw[at] = keep
            assert a.check() == []
    # both halves of a shared band, several bytes each: both regions, the first changed byte of each
    lo, hi, before, after = bands[1]
    a.raw[lo + 8:lo + 12] = 0
    a.raw[hi - 24:hi - 16] = 0
    assert a.check() == [(before, "after", 8, 4), (after, "before", -24, 8)]
    # every band at once, in address order
    a.raw[0] = 0
    a.raw[-1] = 0
    lo2, hi2, _, _ = bands[2]
    a.raw[lo2] = 0
    assert a.check() == [("in", "before", -bands[0][1], 1), ("in", "after", 8, 4), ("work", "before", -24, 8),
                         ("work", "after", 0, 1), ("out", "after", bands[3][1] - bands[3][0] - 1, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_written_into_a_band_is_seen(dtype):
    """the bands are compared as bytes: a NaN, which equals nothing as a number, is a change like any other"""
    a, _ = _arena(dtype)
    a.view("work", extra=1)[-1] = float("nan")
    assert a.check() == [("work", "after", 0, a.itemsize)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_writes_inside_regions_are_not_reported(dtype):
    a, _ = _arena(dtype)
    before = a.snapshot()
    for name in a.names:
        a[name].fill_(3.0)
        a[name][0], a[name][-1] = -1.0, float("inf")
    assert a.check() == []
    after = a.snapshot()
    assert not torch.equal(before, after)
    for lo, hi, _, _ in a.bands():
        assert torch.equal(before[lo:hi], after[lo:hi])
    # the element one past a region is the band's first: the overrun a short output region is there to show
    a.view("out", extra=1)[-1] = 1.0
    assert a.check() == [("out", "after", 0, a.itemsize)]
    assert a.view("in", extra=1).numel() == 38 and a["in"].numel() == 37


def test_a_bad_region_is_refused():
    with pytest.raises(AssertionError):
        Arena(torch.float64, [Region("a", 4, 2)])  # f64: offsets 0 and 1 only
    with pytest.raises(AssertionError):
        Arena(torch.float32, [Region("a", 4), Region("a", 4)])
    with pytest.raises(AssertionError):
        Arena(torch.float32, [Region("a", 4, 0, "data", np.zeros(5, np.float32))])
