"""What the compiler made of the kernels of csrc/nufft_nd.hip (phastft_amd/lib/kernel_resources.json, written by the build from
hipcc's kernel-resource-usage remarks): every instantiation of rank 2 and of rank 3 is there, none uses scratch memory or spills
a register, and the tiled spread kernel of rank 3 is the only one with static LDS, within 64 KiB, so that two workgroups and more
fit a compute unit."""
import json
import os

import pytest

from phastft_amd import build as B


def want(rank):
    """mangled template arguments: d / f the type, Lm2E / Lm3E the rank, Lb0E / Lb1E a false / true flag"""
    d = f"Lm{rank}E"
    return ([f"nufft_nd_spread_kernelI{t}{d}Lb{r}EE" for t in "df" for r in "01"] + [f"nufft_nd_interp_kernelI{t}{d}EE" for t in "df"]
            + [f"nufft_nd_pre_kernelI{t}{d}Lb{v}ELb{r}EE" for t in "df" for v in "01" for r in "01"]
            + [f"nufft_nd_deconv_kernelI{t}{d}Lb{v}EE" for t in "df" for v in "01"])


WANT = want(3)
WANT_2D = want(2)


@pytest.fixture(scope="module")
def all_resources():
    if not os.path.exists(B.RESOURCES):
        B.build()
    return {k: v for k, v in json.load(open(B.RESOURCES)).items() if "nufft_nd_" in k}


@pytest.fixture(scope="module")
def resources(all_resources):
    return {k: v for k, v in all_resources.items() if any(w in k for w in WANT)}


@pytest.fixture(scope="module")
def resources_2d(all_resources):
    return {k: v for k, v in all_resources.items() if any(w in k for w in WANT_2D)}


def test_every_instantiation_is_reported(resources, all_resources):
    for want in WANT:
        assert sum(want in k for k in resources) == 1, want
    assert len(resources) == len(WANT) == 18
    assert len(all_resources) == 36  # the unit holds ranks 2 and 3 and nothing else


def test_no_scratch_no_spills(resources):
    for k, v in resources.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)


def test_static_lds_of_the_spread_kernel(resources):
    for k, v in resources.items():
        if "nufft_nd_spread_kernel" in k:
            assert 0 < v["lds"] <= 64 * 1024, (k, v)
        else:
            assert v["lds"] == 0, (k, v)


def test_every_instantiation_of_rank_2_is_reported(resources_2d):
    for want in WANT_2D:
        assert sum(want in k for k in resources_2d) == 1, want
    assert len(resources_2d) == len(WANT_2D) == 18


def test_rank_2_no_scratch_no_spills_no_lds(resources_2d):
    for k, v in resources_2d.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)
