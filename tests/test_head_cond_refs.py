"""Head training's native text-conditioning stage, the parts that need no GPU: the closed form of include/athd.h
(csrc/head_cond.hip) against torch autograd of `_TextAttention.rows`, the bound the GPU kernels are held to, and the ABI.

  * float64: the closed form equals autograd of `head_cond_refs.torch_stage` to 1e-12 of each tensor's largest value, for
    the output and all seven gradients (the six parameters and the attention vector), on every shape of the GPU tests;
  * float32: the closed form evaluated in float32 lies within ALLOW = 4 times torch-CPU's own float32-against-float64 gap
    on every case and tensor, so the allowance the GPU test uses is within reach of a correct f32 evaluation; two planted
    defects (tanh-GELU in place of erf; a LayerNorm backward without the Vh mean(D Vh) term) exceed it on every case, so
    it is not vacuous;
  * the header and `native.EXPORTED` name the three entries.
"""
import os
import re

import numpy as np
import pytest

import head_cond_refs as R
from conftest import REPO

IDS = ["%d-%d" % c for c in R.CASES]


@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_closed_form_equals_autograd_float64(shape):
    c, g64, _ = R.refs(shape)
    g = R.gaps(R.closed_form(c), g64)
    print(shape, "closed form vs float64 autograd:", g)
    assert max(g.values()) <= 1e-12, g


@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_float32_closed_form_within_allowance(shape):
    c, g64, a = R.refs(shape)
    g = R.gaps(R.closed_form(c, np.float32), g64)
    ratio = {k: (g[k] / a[k] if a[k] > 0 else (0.0 if g[k] == 0 else float("inf"))) for k in R.NAMES}
    print(shape, "f32 closed form / a:", ratio, "a:", a)
    assert max(ratio.values()) <= R.ALLOW, (ratio, a)


@pytest.mark.parametrize("mut", ["tanh_gelu", "ln_no_proj"])
@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_planted_defects_exceed_allowance(shape, mut):
    c, g64, a = R.refs(shape)
    g = R.gaps(R.closed_form(c, np.float32, mut=mut), g64)
    ratio = {k: g[k] / a[k] for k in R.NAMES if a[k] > 0}
    print(shape, mut, ratio)
    assert max(ratio.values()) > R.ALLOW, (mut, ratio)


def test_abi_names_the_new_entries():
    from athd import native
    names = ["athd_head_cond_workspace_bytes", "athd_head_cond", "athd_head_cond_backward"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "athd.h")).read(), flags=re.S)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in native.EXPORTED and hasattr(native.lib, n), n
    # four tile tensors, W2 transposed, the per-tile and per-item row sums and 14 weight-gradient slices; none for a
    # shape out of range
    ws = lambda B, N: native.lib.athd_head_cond_workspace_bytes(B, N)
    tiles = 3 * 2
    assert ws(3, 70) == 4 * (4 * tiles * 384 * 64 + 384 * 384 + tiles * 4 * 384 + 3 * 4 * 384 + 14 * 2 * 384 * 384)
    assert ws(8, 16384) > 0 and ws(1, 1 << 20) > 0
    assert ws(0, 64) == 0 and ws(65536, 64) == 0 and ws(1, 0) == 0 and ws(1, (1 << 20) + 1) == 0
