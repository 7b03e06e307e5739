"""What the compiler made of the kernels of csrc/resample.hip (phastft_amd/lib/kernel_resources.json, written by the build from
hipcc's kernel-resource-usage remarks): every instantiation is there, none uses scratch memory or spills a register, and the
static LDS is what DESIGN.md section 27 says: the tap chunk with its padding and the run of the signal in the polyphase kernel
(4096 + 512 + 4096 elements: 68 KiB in f64, 34 KiB in f32), none in the spectrum sweep."""
import json
import os

import pytest

from phastft_amd import build as B

# mangled template arguments: d / f the type
UPFIRDN = [f"upfirdn_kernelI{t}EE" for t in "df"]
SPECTRUM = [f"resample_spectrum_kernelI{t}EE" for t in "df"]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "upfirdn_kernel" in k or "resample_spectrum_kernel" in k}


def test_every_instantiation_is_reported(resources):
    for want in UPFIRDN + SPECTRUM:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == 4


def test_no_scratch_no_spills_and_the_lds_of_the_kernels(resources):
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        item = 8 if "Id" in k else 4
        lds = (4096 + 512 + 4096) * item if "upfirdn" in k else 0
        assert v["lds"] == lds, (k, v)
        if lds:
            assert f"{lds} bytes" in design, lds   # the figure the design section states
    # two f64 and four f32 workgroups share a CU's 160 KiB
    for k, v in resources.items():
        if "upfirdn" in k:
            assert v["occupancy"] == (2 if "Id" in k else 4), (k, v)
