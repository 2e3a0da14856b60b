"""Head training's native output stage, the parts that need no GPU: the closed form of the adjoint (include/athd.h,
csrc/head_grad.hip) against torch autograd of the output stage's own ops, the bound the GPU kernel is held to, and the ABI.

  * float64: the closed form equals autograd of `head_output_refs.torch_stage` to 1e-12 of each item's largest
    |gradient|, on every shape of the GPU kernel tests;
  * float32: the closed form evaluated in float32 in the kernel's order of operations lies within ALLOW = 4 times `a`, the
    gap of torch's own float32 autograd to float64 on the same case.  So the allowance the GPU test uses is within reach
    of a correct f32 evaluation; two planted defects (c_kb = 1 on the interior bins; a DC bin that keeps an imaginary
    part) exceed it on every case, so it is not vacuous;
  * the header and `native.EXPORTED` name the three entries and the workspace query.
"""
import os
import re

import numpy as np
import pytest
import torch

import head_output_refs as R
from conftest import REPO

IDS = ["%d-%d-%d" % c for c in R.CASES]


_refs = R.refs


@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_closed_form_equals_autograd_float64(shape):
    c, g64, _ = _refs(shape)
    dxd, dxt = R.closed_form(c)
    gap = max(R.item_gap(dxd, g64[0]) + R.item_gap(dxt, g64[1]))
    print(shape, "closed form vs float64 autograd:", gap)
    assert gap <= 1e-12, gap


@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_float32_closed_form_within_allowance(shape):
    c, g64, a = _refs(shape)
    dxd, dxt = R.closed_form(c, f32=True)
    ratio = [g / ai for g, ai in zip(R.item_gap(dxd, g64[0]), a)]
    print(shape, "f32 closed form / a:", ratio, "a:", a)
    assert max(ratio) <= R.ALLOW, (ratio, a)
    assert np.array_equal(dxt, g64[1])                           # g * stdt: one exact product of float32 values


@pytest.mark.parametrize("mut", ["c1", "dc_imag"])
@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_planted_defects_exceed_allowance(shape, mut):
    c, g64, a = _refs(shape)
    dxd, _ = R.closed_form(c, f32=True, mut=mut)
    ratio = [g / ai for g, ai in zip(R.item_gap(dxd, g64[0]), a)]
    print(shape, mut, ratio)
    assert min(ratio) > R.ALLOW, (mut, ratio)


def test_time_branch_resize_in_front():
    """a head that emits xtd of another length: the torch resize in front of the stage, its gradient by autograd"""
    c, _, _ = _refs((3, 3072, 2))
    short = c["xtd"][..., :3000].contiguous()
    _, dx = R.autograd(c, torch.float64, xtd=short)
    assert dx.shape == (2, 2, 3000)
    want = torch.autograd.functional.vjp(
        lambda x: torch.nn.functional.interpolate(x, size=3072, mode="linear", align_corners=False), short,
        c["g"] * c["stdt"])[1]
    assert float((torch.as_tensor(dx) - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_abi_names_the_new_entries():
    from athd import native
    names = ["athd_pack_spectrum", "athd_head_output_workspace_bytes", "athd_head_output", "athd_head_output_backward"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "athd.h")).read(), flags=re.S)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in native.EXPORTED and hasattr(native.lib, n), n
    # the workspace is the forward's boundary-partials buffer; shapes out of range have none
    assert native.lib.athd_head_output_workspace_bytes(2, 33297) == 2 * 2 * 12288 * 4
    assert native.lib.athd_head_output_workspace_bytes(1, 2049 * 1024) == 0
    assert native.lib.athd_head_output_workspace_bytes(0, 4096) == 0
