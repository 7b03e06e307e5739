"""What the compiler made of the kernels of csrc/dwt.hip (phastft_amd/lib/kernel_resources.json, written by the build from
hipcc's kernel-resource-usage remarks): every instantiation is there, none uses scratch memory or spills a register, and the
static LDS and the occupancy are what DESIGN.md section 31 says: two arrays of 1168 elements in either kernel (18688 bytes in
f64, 9344 in f32), eight waves per SIMD -- eight workgroups per CU, bound by the wave slots, not by LDS or registers."""
import json
import os

import pytest

from phastft_amd import build as B

# mangled template arguments: d / f the type
KERNELS = [f"dwt_{k}_kernelI{t}EE" for k in ("analysis", "synthesis") for t in "df"]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "dwt_" in k}


def test_every_instantiation_is_reported(resources):
    for want in KERNELS:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == 4


def test_no_scratch_no_spills_lds_and_occupancy(resources):
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    section = design.split("## 31.", 1)[1]
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        lds = 2 * 1168 * (8 if "Id" in k else 4)
        assert v["lds"] == lds, (k, v)
        assert f"{lds} bytes" in section, lds   # the figure the design section states
        assert v["occupancy"] == 8, (k, v)      # 8 waves per SIMD: 8 workgroups of 4 waves per CU
        assert 8 * lds <= 160 * 1024            # ... whose LDS fits the CU's 160 KiB together
        assert v["vgprs"] <= 64, (k, v)         # 512 / 8
    assert "eight workgroups per CU" in section
