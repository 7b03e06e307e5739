"""What the compiler made of the kernels of csrc/cwt.hip (phastft_amd/lib/kernel_resources.json, written by the build from hipcc's
kernel-resource-usage remarks): both instantiations of the bank kernel and of the pad / crop sweep are there, none uses scratch
memory or spills a register or has any LDS, and the bank's VGPR counts and occupancy are the ones DESIGN.md section 30 states."""
import json
import os
import re

import pytest

from phastft_amd import build as B

BANK = [f"cwt_bank_kernelI{t}EE" for t in "df"]  # mangled template arguments: d / f the type
COPY = [f"cwt_copy_kernelI{t}EE" for t in "df"]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "cwt_" in k}


def test_every_instantiation_is_reported(resources):
    for want in BANK + COPY:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == 4


def test_no_scratch_no_spills_and_the_lds_and_occupancy_of_the_design(resources):
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    section = design[design.index("## 30."):]
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["lds"] == 0, (k, v)
        if "cwt_bank" not in k:
            continue
        assert "0 bytes of LDS" in section   # the figures the design section states
        m = re.search(r"occupancy (\d) waves\s+per SIMD in f64 and (\d) in f32", section)
        assert m and v["occupancy"] == int(m.group(1 if "Id" in k else 2)), (k, v)
        m = re.search(r"(\d+) VGPRs in f64 and (\d+) in f32", section)
        assert m and v["vgprs"] == int(m.group(1 if "Id" in k else 2)), (k, v)
