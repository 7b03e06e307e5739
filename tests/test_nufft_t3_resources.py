"""What the compiler made of the kernels of csrc/nufft_t3.hip (phastft_amd/lib/kernel_resources.json, written by the build from
hipcc's kernel-resource-usage remarks): every instantiation is there, and none uses scratch memory, spills a register or has
static LDS -- the gather sums in registers and stores once."""
import json
import os

import pytest

from phastft_amd import build as B

# mangled template arguments: d / f the type, Lb0E / Lb1E a false / true flag
WANT = [f"nufft_t3_spread_kernelI{t}Lb{r}EE" for t in "df" for r in "01"] + [f"nufft_t3_post_kernelI{t}Lb{v}EE" for t in "df" for v in "01"]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "nufft_t3_" in k}


def test_every_instantiation_is_reported(resources):
    for want in WANT:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == len(WANT) == 8


def test_no_scratch_no_spills_no_lds(resources):
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)
