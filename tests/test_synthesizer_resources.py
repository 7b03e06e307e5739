"""What the compiler made of the unfold kernel of csrc/synthesizer.hip (phastft_amd/lib/kernel_resources.json, written by the build
from hipcc's kernel-resource-usage remarks): both instantiations are there, neither uses scratch memory or spills a register,
and the static LDS and the occupancy are what DESIGN.md section 29 says: no LDS at all, at eight waves per SIMD.  The copy sweep
beside it is held to the same."""
import json
import os
import re

import pytest

from phastft_amd import build as B

UNFOLD = [f"synth_unfold_kernelI{t}EE" for t in "df"]  # mangled template arguments: d / f the type
COPY = [f"synth_copy_kernelI{t}EE" for t in "df"]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "synth_" in k}


def test_every_instantiation_is_reported(resources):
    for want in UNFOLD + COPY:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == 4


def test_no_scratch_no_spills_and_the_lds_and_occupancy_of_the_design(resources):
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    section = design[design.index("## 29."):]
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["lds"] == 0, (k, v)
        if "synth_unfold" not in k:
            continue
        assert "0 bytes of LDS" in section   # the figures the design section states
        m = re.search(r"occupancy (\d) waves\s+per SIMD in f64 and (\d) in f32", section)
        assert m and v["occupancy"] == int(m.group(1 if "Id" in k else 2)), (k, v)
        m = re.search(r"(\d+) VGPRs in f64 and (\d+) in f32", section)
        assert m and v["vgprs"] == int(m.group(1 if "Id" in k else 2)), (k, v)
