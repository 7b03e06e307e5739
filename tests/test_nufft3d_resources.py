"""What the compiler made of the kernels of csrc/nufft3d.hip (phastft_amd/lib/kernel_resources.json, written by the build from
hipcc's kernel-resource-usage remarks): every instantiation is there, none uses scratch memory or spills a register, and the
tiled spread kernel's static LDS stays within 64 KiB, so that two workgroups and more fit a compute unit."""
import json
import os

import pytest

from phastft_amd import build as B

# mangled template arguments: d / f the type, Lb0E / Lb1E a false / true flag
WANT = ([f"nufft3d_spread_kernelI{t}Lb{r}EE" for t in "df" for r in "01"] + [f"nufft3d_interp_kernelI{t}EE" for t in "df"]
        + [f"nufft3d_pre_kernelI{t}Lb{v}ELb{r}EE" for t in "df" for v in "01" for r in "01"]
        + [f"nufft3d_deconv_kernelI{t}Lb{v}EE" for t in "df" for v in "01"])


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "nufft3d_" in k}


def test_every_instantiation_is_reported(resources):
    for want in WANT:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == len(WANT) == 18


def test_no_scratch_no_spills(resources):
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)


def test_static_lds_of_the_spread_kernel(resources):
    for k, v in resources.items():
        if "nufft3d_spread_kernel" in k:
            assert 0 < v["lds"] <= 64 * 1024, (k, v)
        else:
            assert v["lds"] == 0, (k, v)
