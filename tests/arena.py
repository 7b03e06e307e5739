"""A packed, guarded arena for the tests of calls that work in caller-provided buffers (a plain helper, not a conftest).

One allocation per arena, laid out as

    band | region | band | region | ... | band

Every region has a name, a length in elements, an element offset from a 16-byte boundary and a fill:

    "data"      copied in from an array of the region's length (inputs; a zero-filled workspace is data of zeros)
    "sentinel"  a finite value (outputs: what the call does not write keeps it)
    "poison"    quiet NaN (workspaces: a value the call reads before it wrote it spreads into the result)

Bands hold the byte 0xA5 (the library's kGuardFill) and are compared through a uint8 view, so that no NaN comparison can hide
a change.  A band is max(4096, 2 M) elements wide, M being the largest inner convolution length of the planner under test
(0: none), plus the up to 16 / itemsize - 1 elements that bring the next region to its offset: a write one whole padded row
(re and im, 2 M elements) before or past a region still lands in a band.  A write further out than that is NOT caught -- it
lands in a neighbouring region (whose own checks may or may not notice) or outside the allocation.

check() reports, it asserts nothing: a list of (region, side, offset, count).  `side` is "before" or "after" the region,
`count` the bytes that changed there, `offset` the byte offset of the first changed byte from the region's edge: 0, 1, ...
from the first byte past the region's end for "after", -1, -2, ... back from the region's first byte for "before".  A band
between two regions is split in the middle: its first half is reported "after" the region it follows, its second half
"before" the region it precedes (an attribution by distance; both are reported when both halves changed).

Works on torch CPU tensors as on device tensors (tests/test_arena_cpu.py)."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

GUARD = 0xA5          # kGuardFill
MIN_BAND = 4096       # elements
SENTINEL = 9.0


@dataclasses.dataclass
class Region:
    name: str
    length: int                  # elements
    offset: int = 0              # elements past a 16-byte boundary: 0 .. 16 / itemsize - 1
    fill: str = "poison"         # "data" | "sentinel" | "poison"
    data: np.ndarray | None = None


def band_len(m: int = 0) -> int:
    return max(MIN_BAND, 2 * int(m))


class Arena:
    def __init__(self, dtype, regions, m: int = 0, device="cpu", sentinel: float = SENTINEL):
        regions = list(regions)
        self.dtype, self.device, self.sentinel = dtype, device, sentinel
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.vec = 16 // self.itemsize
        self.band = band_len(m)
        self.names = [r.name for r in regions]
        assert regions and len(set(self.names)) == len(self.names), self.names
        self._at = {}
        cursor = 0
        for r in regions:
            assert r.length >= 1 and 0 <= r.offset < self.vec and r.fill in ("data", "sentinel", "poison"), r
            start = cursor + self.band
            start += (r.offset - start) % self.vec
            self._at[r.name] = (start, r.length)
            cursor = start + r.length
        total = cursor + self.band
        whole = torch.empty(total + self.vec, dtype=dtype, device=device)
        lead = (-(whole.data_ptr() // self.itemsize)) % self.vec  # to the allocation's first 16-byte boundary
        self._buf = whole[lead:lead + total]
        self.raw = self._buf.view(torch.uint8)
        self.raw.fill_(GUARD)
        for r in regions:
            t = self[r.name]
            if r.fill == "data":
                src = np.array(r.data).reshape(-1)  # a copy: the source may be read-only
                assert src.size == r.length, (r.name, src.size, r.length)
                t.copy_(torch.from_numpy(src).to(dtype))
            else:
                t.fill_(sentinel if r.fill == "sentinel" else float("nan"))

    def __getitem__(self, name: str):
        return self.view(name)

    def view(self, name: str, extra: int = 0):
        """the region as a 1-D tensor; `extra` elements more reach into the band behind it (for a test of the checker)"""
        start, length = self._at[name]
        return self._buf[start:start + length + extra]

    def bytes_of(self, name: str):
        start, length = self._at[name]
        return self.raw[start * self.itemsize:(start + length) * self.itemsize]

    def snapshot(self):
        """every byte of the arena, bands included"""
        return self.raw.clone()

    def bands(self):
        """(first byte, end byte, region before or None, region after or None) of every band, in address order"""
        out, prev, at = [], None, 0
        for name in self.names:
            start, length = self._at[name]
            out.append((at * self.itemsize, start * self.itemsize, prev, name))
            prev, at = name, start + length
        out.append((at * self.itemsize, self.raw.numel(), prev, None))
        return out

    def check(self):
        found = []
        for lo, hi, before, after in self.bands():
            bad = self.raw[lo:hi] != GUARD
            if not bool(bad.any()):
                continue
            idx = bad.nonzero().reshape(-1).cpu().numpy() + lo
            split = lo if before is None else hi if after is None else (lo + hi) // 2
            first, second = idx[idx < split], idx[idx >= split]
            if first.size:
                found.append((before, "after", int(first[0] - lo), int(first.size)))
            if second.size:
                found.append((after, "before", int(second[0] - hi), int(second.size)))
        return found
