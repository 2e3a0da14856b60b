"""The references of tests/head_proj_refs.py, on the CPU: what tests/test_gpu_head_proj.py holds the kernels to.

  * the float64 closed forms of both primitives are torch's float64 autograd of `nn.Conv2d(4, 2, 1)` / `nn.Conv1d(4, 2, 1)`
    and of `_TextAttention.attn_vector` (to 1e-12);
  * a float32 evaluation of the closed form stays within ALLOW = 4 units of the float64 reference on every case, the unit
    per tensor being max(torch's own f32-against-f64 gap, the derived rounding bound);
  * every planted defect leaves that allowance, on at least one of the tensors it shows in, on every case that can see it;
  * the header and `native.EXPORTED` name the five entries; the workspace query's host arithmetic and limits.
"""
import os
import re

import numpy as np
import pytest

import head_proj_refs as R

PROJ_IDS = ["-".join(str(int(v)) for v in c) for c in R.PROJ_CASES]


@pytest.mark.parametrize("shape", R.PROJ_CASES, ids=PROJ_IDS)
def test_proj_closed_form_is_torch_float64(shape):
    c, g64, _, _ = R.proj_refs(shape)
    got = R.proj_closed_form(c)
    for k in R.PROJ_NAMES:
        assert got[k].shape == g64[k].shape, k
        assert R.gap(got[k], g64[k]) <= 1e-12, k


@pytest.mark.parametrize("shape", R.PROJ_CASES, ids=PROJ_IDS)
def test_proj_float32_reaches_the_bound_and_defects_do_not(shape):
    c, g64, a, floor = R.proj_refs(shape)
    unit = R.units(a, floor)
    f32 = R.proj_closed_form(c, np.float32)
    ratio = R.ratios({k: R.gap(f32[k], g64[k]) for k in R.PROJ_NAMES}, unit)
    print(shape, "float32 gap / unit:", ratio, "a:", a, "floor:", floor)
    assert max(ratio.values()) <= R.ALLOW, ratio
    for mut in R.PROJ_MUTS:
        bad = R.proj_closed_form(c, np.float32, mut)
        r = R.ratios({k: R.gap(bad[k], g64[k]) for k in R.PROJ_NAMES}, unit)
        if R.proj_blind(shape, mut):
            assert max(r.values()) <= R.ALLOW, (mut, r)               # blind means blind: the defect changes nothing
        else:
            assert max(r[k] for k in R.proj_sees(mut)) > R.ALLOW, (mut, r)


def test_every_proj_defect_is_seen_by_some_case():
    for mut in R.PROJ_MUTS:
        assert any(not R.proj_blind(s, mut) for s in R.PROJ_CASES), mut


@pytest.mark.parametrize("B", R.ATTN_CASES)
def test_attn_closed_form_is_torch_float64(B):
    c, g64, _, _ = R.attn_refs(B)
    g = R.attn_gaps(R.attn_closed_form(c), g64)
    assert max(g.values()) <= 1e-12, g
    assert not g64["w_in_dead"].any() and not g64["b_in_dead"].any()


@pytest.mark.parametrize("B", R.ATTN_CASES)
def test_attn_float32_reaches_the_bound_and_defects_do_not(B):
    c, g64, a, floor = R.attn_refs(B)
    unit = R.units(a, floor)
    ratio = R.ratios(R.attn_gaps(R.attn_closed_form(c, np.float32), g64), unit)
    print(B, "float32 gap / unit:", ratio)
    assert max(ratio.values()) <= R.ALLOW, ratio
    r = R.ratios(R.attn_gaps(R.attn_closed_form(c, np.float32, "k_third"), g64), unit)
    assert min(r[k] for k in ("a", "wv", "bv", "w_in", "b_in", "wo")) > R.ALLOW, r
    r = R.ratios(R.attn_gaps(R.attn_closed_form(c, np.float32, "dead_nonzero"), g64), unit)
    assert r["w_in_dead"] > R.ALLOW and r["b_in_dead"] > R.ALLOW, r


def test_header_and_bindings_name_the_entries():
    from athd import native
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "athd.h")).read()
    for n in ("athd_head_proj_workspace_bytes", "athd_head_proj", "athd_head_proj_backward", "athd_head_attn_vec",
              "athd_head_attn_vec_backward"):
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in native.EXPORTED and hasattr(native.lib, n), n


def test_workspace_bytes_and_limits():
    """host arithmetic of athd_head_proj_workspace_bytes: ten doubles per workgroup of the larger of the backward's two
    grids (chunks of 4096 positions per item; 32 x 32 tiles per item); 0 outside the limits"""
    from athd import native
    ws = native.Context.head_proj_workspace_bytes
    assert ws(1, 1, 1) == 80
    assert ws(2, 1, 4096) == 2 * 80 and ws(2, 1, 4097) == 4 * 80
    assert ws(3, 33, 37) == 3 * 4 * 80                                 # 4 tiles against 1 chunk
    assert ws(1, 2048, 2048) == 80 * 64 * 64                           # a 2048 x 2048 grid: the tiles
    assert ws(8, 1, 47 * 44100) == 8 * 80 * -(-47 * 44100 // 4096)     # 47 s with R = 1
    assert ws(65535, 1, 1) == 65535 * 80 and ws(1, 1, 1 << 22) == 80 * 1024 and ws(1, 4096, 1024) > 0
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (1, 4097, 1), (1, 1, (1 << 22) + 1), (1, 2, 1 << 22),
                (1, 4096, 1025), (-1, 1, 1)):
        assert ws(*bad) == 0, bad
