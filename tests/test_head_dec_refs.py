"""Head training's native decoder level, the parts that need no GPU: the closed form of include/athd.h (csrc/head_dec.hip)
against torch autograd of one `_Decoder` level, the bound the GPU kernels are held to, and the ABI.

  * float64: the closed form equals autograd of `head_dec_refs.torch_level` to 1e-12 of each tensor's largest value, for
    the output and every gradient (input, weight, bias, GroupNorm weight and bias), on every shape of the GPU tests;
  * float32: the closed form evaluated in float32 lies within ALLOW = 4 times torch-CPU's own float32-against-float64 gap
    on every case and tensor, so the allowance the GPU test uses is within reach of a correct f32 evaluation; five planted
    defects (tanh-GELU in place of erf; a GroupNorm backward without the ch mean(D ch) term; align_corners=True; an
    unscaled skip; the two taps k1 / k1 + 4 exchanged) exceed it in at least one tensor of every case that can see them
    (`head_dec_refs.blind` names the cases that cannot), so it is not vacuous;
  * the frequency decoder's ops with one column are the time decoder's ops;
  * `native_decoders` is off by default and, without a bound model, raises instead of running torch's ops;
  * the header and `native.EXPORTED` name the three entries, and the workspace formula is the header's.
"""
import os
import re

import numpy as np
import pytest
import torch

import head_dec_refs as R
from conftest import REPO

IDS = ["-".join(str(v) for v in c) for c in R.CASES]


@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_closed_form_equals_autograd_float64(shape):
    c, g64, _ = R.refs(shape)
    g = R.gaps(R.closed_form(c), g64)
    print(shape, "closed form vs float64 autograd:", g)
    assert set(g) == set(R.names(shape[0]))
    assert max(g.values()) <= 1e-12, g


@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_float32_closed_form_within_allowance(shape):
    c, g64, a = R.refs(shape)
    ratio = R.ratios(R.gaps(R.closed_form(c, np.float32), g64), a)
    print(shape, "f32 closed form / a:", ratio, "a:", a)
    assert max(ratio.values()) <= R.ALLOW, (ratio, a)


@pytest.mark.parametrize("mut", R.MUTS)
@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_planted_defects_exceed_allowance(shape, mut):
    c, g64, a = R.refs(shape)
    g = R.gaps(R.closed_form(c, np.float32, mut=mut), g64)
    ratio = {k: g[k] / a[k] for k in a if a[k] > 0}
    print(shape, mut, ratio)
    if R.blind(shape, mut):
        assert max(ratio.values()) <= R.ALLOW, (mut, ratio)       # the case cannot see it: the same values as without it
    else:
        assert max(ratio.values()) > R.ALLOW, (mut, ratio)


def test_every_defect_is_seen_by_some_case():
    for mut in R.MUTS:
        assert any(not R.blind(s, mut) for s in R.CASES), mut


def test_time_decoder_is_the_frequency_decoder_with_one_column():
    from athd.head import _Decoder
    c = R.case(1, 2, 63, 1, 250, 63)
    ft, tt = _Decoder(True).double(), _Decoder(False).double()
    tt.load_state_dict({k: v.squeeze(-1) if v.dim() == 4 else v for k, v in ft.state_dict().items()})
    want = R.torch_level(tt, 1, c["x"].squeeze(-1), c["skip"].squeeze(-1), c["Lt"])
    got = R.torch_level(ft, 1, c["x"], c["skip"], c["Lt"]).squeeze(-1)
    assert torch.equal(got, want) or float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())


def test_option_is_off_by_default_and_never_falls_back():
    import head_refs as H
    from athd.head import NativeDecoderLevel, TrainableHead
    assert issubclass(NativeDecoderLevel, torch.autograd.Function)
    assert not TrainableHead().native_decoders
    head = TrainableHead(native_decoders=True).float()
    feats, text = H.seeded_features(torch.float32), H.seeded_text(torch.float32)
    with pytest.raises(RuntimeError, match="native_decoders.*bind"):
        head(feats, text)                                             # no model bound, no GPU: an error, not torch's ops


def test_abi_names_the_new_entries():
    from athd import native
    names = ["athd_head_dec_workspace_bytes", "athd_head_dec_level", "athd_head_dec_level_backward"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "athd.h")).read(), flags=re.S)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in native.EXPORTED and hasattr(native.lib, n), n
    ws = native.lib.athd_head_dec_workspace_bytes
    up4 = lambda v: (v + 3) // 4 * 4
    for level, B, M, inner, Lt, _ in R.CASES:
        Ci, Co = R.LEVELS[level]
        P = 4 * M * inner
        n, q, slices = Co * P, -(-P // 1024), [8, 16, 32, 64][level]
        want = (2 * up4(B * n) + up4(B * -(-n // 8192)) + 2 * up4(2 * B) + up4(2 * B * Co * q) + up4(B * Co * q)
                + up4(2 * B * Co) + up4(slices * Ci * Co * 8))
        assert ws(level, B, M, inner, Lt) == 4 * want, (level, B, M, inner, Lt)
    # 2048 frames: the time decoder's last level, the frequency decoder's widest; none for a shape out of range
    assert ws(3, 1, 524288, 1, 2097152) > 0 and ws(1, 1, 2048, 2048, 2048) > 0
    for bad in [(4, 1, 8, 1, 32), (-1, 1, 8, 1, 32), (0, 0, 8, 1, 32), (0, 65536, 8, 1, 32), (0, 1, 0, 1, 32),
                (0, 1, (1 << 20) + 1, 1, 32), (0, 1, 8, 0, 32), (0, 1, 8, 4097, 32), (0, 1, 8, 1, 0),
                (0, 1, 8, 1, (1 << 22) + 1), (0, 1, 1 << 20, 128, 32), (0, 1, 8, 4096, 1 << 20)]:
        assert ws(*bad) == 0, bad
