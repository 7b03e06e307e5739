"""What the compiler made of the kernels of csrc/lomb.hip (phastft_amd/lib/kernel_resources.json, written by the build from
hipcc's kernel-resource-usage remarks): every instantiation is there, none uses scratch memory or spills a register, and the
static LDS is what the sweeps say: the 256 doubles of the slab sweeps' tree, the 1024 partials of the final sweep, none in
the post sweep."""
import json
import os

import pytest

from phastft_amd import build as B

# mangled template arguments: d / f the type, Lb0E / Lb1E a false / true flag
SLAB = [f"lomb_slab_kernelI{t}Lb{s}EE" for t in "df" for s in "01"]
POST = [f"lomb_post_kernelI{t}Lb{v}EE" for t in "df" for v in "01"]
FINAL = ["lomb_final_kernelE"]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "lomb_" in k}


def test_every_instantiation_is_reported(resources):
    for want in SLAB + POST + FINAL:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == 9


def test_no_scratch_no_spills_and_the_lds_of_the_sweeps(resources):
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        lds = 256 * 8 if "lomb_slab" in k else 1024 * 8 if "lomb_final" in k else 0
        assert v["lds"] == lds, (k, v)
