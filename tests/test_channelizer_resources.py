"""What the compiler made of the fold kernel of csrc/channelizer.hip (phastft_amd/lib/kernel_resources.json, written by the build
from hipcc's kernel-resource-usage remarks): both instantiations are there, neither uses scratch memory or spills a register,
and the static LDS and the occupancy are what DESIGN.md section 28 says: 4096 samples of the signal, 32 KiB in f64 and 16 KiB in
f32, at four waves per SIMD."""
import json
import os
import re

import pytest

from phastft_amd import build as B

FOLD = [f"chan_fold_kernelI{t}EE" for t in "df"]  # mangled template arguments: d / f the type


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "chan_fold_kernel" in k}


def test_every_instantiation_is_reported(resources):
    for want in FOLD:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == 2


def test_no_scratch_no_spills_and_the_lds_and_occupancy_of_the_design(resources):
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    section = design[design.index("## 28."):]
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        lds = 4096 * (8 if "Id" in k else 4)
        assert v["lds"] == lds, (k, v)
        assert f"{lds} bytes" in section, lds   # the figures the design section states
        m = re.search(r"occupancy (\d) waves per SIMD in f64 and (\d) in f32", section)
        assert m and v["occupancy"] == int(m.group(1 if "Id" in k else 2)), (k, v)
