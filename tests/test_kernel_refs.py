"""CPU checks of tests/kernel_refs.py: the references are right, their tolerances hold for an honest low-precision
evaluation, and every deliberate mutation (the kind of bug a kernel can have) lands more than 10x outside the
tolerance on every swept shape, so the GPU comparisons of tests/test_gpu_kernels.py have teeth."""
import numpy as np
import pytest

import kernel_refs as kr
import test_gpu_kernels as tg

LN2 = tg.LN2


def _exceeds(R, Rm, tol, factor=10.0):
    return bool((np.abs(Rm - R) > factor * tol).any())


# ------------------------------------------------------------------------------------------------ bf16 helpers
def test_bf16_round_to_nearest_even():
    x = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0x00008000, 0x00018000, 0x80000000],
                 dtype=np.uint32).view(np.float32)
    assert [int(v) for v in kr.bf16_bits(x)] == [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0x7F80, 0x0000, 0x0002, 0x8000]
    import torch
    y = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    t = torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(kr.bf16_bits(y), t)


def test_bf16_round_amb_flags_ties_only():
    a = np.array([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 1e-9, 1.0 + 2.0 ** -10, 0.0, -3.0 - 2.0 ** -7])
    r, amb = kr.bf16_round_amb(a)
    assert list(amb > 0) == [True, True, False, False, True]
    assert amb[0] == 2.0 ** -7 and amb[4] == 2.0 ** -6


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("Nq,Nk", tg.ATTN_PAIRS)
def test_attn_mutations_detected(Nq, Nk):
    rng = np.random.default_rng(Nq * 7 + Nk)
    for mode, scale in ((1, LN2), (0, 0.125)):
        for mult, place in tg.ATTN_VARIANTS:
            if place == "kzero":
                continue
            q, k, v = tg._attn_inputs(rng, Nq, Nk, mult, place, mode == 1)
            if Nq > 16:          # (queries are independent: the first and last 8 of the shape's inputs)
                q = np.concatenate([q[:, :, :8], q[:, :, -8:]], axis=2)
            R, tol = kr.attn_ref(q, k, v, scale, mode)
            # one head's V used for another
            Rm, _ = kr.attn_ref(q, k, np.roll(v, 1, axis=1), scale, mode)
            assert _exceeds(R, Rm, tol), ("head", mode, mult, place)
            if Nk < 2:
                continue          # (one key: nothing to drop or swap)
            if place != "last":
                continue          # (elsewhere the last key's weight is ~1 / Nk or underflows: no error to see.  The
                                  # 'last' placement gives it the largest logit at every scale)
            # last key dropped
            Rm, _ = kr.attn_ref(q, k[:, :, :-1], v[:, :, :-1], scale, mode)
            assert _exceeds(R, Rm, tol), ("drop", mode, mult, place)
            # two V rows of one key tile swapped (the last tile's first and last keys)
            a, b = (Nk - 1) // 64 * 64, Nk - 1
            if a == b:
                a = b - 1
            vs = v.copy()
            vs[:, :, [a, b]] = vs[:, :, [b, a]]
            Rm, _ = kr.attn_ref(q, k, vs, scale, mode)
            assert _exceeds(R, Rm, tol), ("swap", mode, mult, place)


@pytest.mark.parametrize("Nq,Nk", [(5, 1), (33, 63), (17, 64), (9, 65), (40, 200), (8, 2072)])
@pytest.mark.parametrize("mult", [1, 36, 400])
def test_attn_bf16_emulation_within_tolerance(Nq, Nk, mult):
    """64-key online softmax, P rounded to bf16 once, f32 accumulation, bf16 output: inside 4u (P|V|) + 2u |R|"""
    rng = np.random.default_rng(Nk + mult)
    worst = 0.0
    for place in ("rand", "first", "last"):
        q, k, v = tg._attn_inputs(rng, Nq, Nk, mult, place, True)
        R, tol = kr.attn_ref(q, k, v, LN2, 1)
        o = kr.attn_emulate_bf16(q, k, v, LN2)
        worst = max(worst, float((np.abs(o - R) / tol).max()))
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ GEMM
def test_gemm_ref_plain_is_matmul():
    rng = np.random.default_rng(3)
    g = tg.build_gemm(3, 0, nb=2, H_in=37, C_in=40, N=24, Kp=64, bias=False, a_bf16=0)
    ref = kr.gemm_ref(g, 0)
    A = g.A.reshape(74, 40)
    exp = A @ g.Wp[:24, :40].T
    assert np.array_equal(ref.idx, np.arange(74 * 24))
    assert np.abs(ref.R.reshape(74, 24) - exp).max() <= 1e-13 * np.abs(exp).max()
    assert (ref.tol > 0).all()


def test_gemm_ref_conv_matches_torch():
    """the implicit-conv indexing (taps, stride, dilation, zero padding per batch) against torch conv1d in float64"""
    import torch
    for dil, stride, ntaps, off in ((1, 1, 3, -1), (2, 1, 3, -2), (1, 4, 8, -2)):
        H_in = 44
        H_out = H_in if stride == 1 else H_in // 4
        g = tg.build_gemm(9, 0, nb=3, H_in=H_in, H_out=H_out, C_in=8, N=12, ntaps=ntaps, in_stride=stride, in_off=off,
                          dil=dil, a_bf16=0, Kp=_ru(ntaps * 8, 32))
        ref = kr.gemm_ref(g, 0)
        x = torch.from_numpy(g.A.reshape(3, H_in, 8)).permute(0, 2, 1)
        w = torch.from_numpy(g.Wp[:12, :ntaps * 8].reshape(12, ntaps, 8)).permute(0, 2, 1).contiguous()
        y = torch.nn.functional.conv1d(x, w, torch.from_numpy(g.bias), stride=stride, padding=-off, dilation=dil)
        exp = y.permute(0, 2, 1).numpy()[:, :H_out]
        assert np.abs(ref.v.reshape(3, H_out, 12) - exp).max() < 1e-12


def _ru(a, b):
    return (a + b - 1) // b * b


def test_gemm_ref_glu_pair_order_and_routing():
    """GLU over packed pairs [a(16) | gate(16)] per 32 columns; col_split routes group g to row + g hi_row_off"""
    g = tg.build_gemm(4, 0, nb=1, H_in=5, C_in=8, N=64, act=kr.ACT_GLU, a_bf16=0, Kp=32)
    ref = kr.gemm_ref(g, 0)
    v = g.A.reshape(5, 8) @ g.Wp[:64, :8].T + g.bias
    exp = np.concatenate([v[:, 0:16] * kr.sigmoid(v[:, 16:32]), v[:, 32:48] * kr.sigmoid(v[:, 48:64])], axis=1)
    assert np.abs(ref.R.reshape(5, 32) - exp).max() < 1e-13
    g = tg.build_gemm(4, 0, nb=2, H_in=3, W=2, C_in=8, N=16, ntaps=3, in_off=-1, a_bf16=0, Kp=32, convt=("quad", 0))
    ref = kr.gemm_ref(g, 0)
    out = np.zeros(g.c_elems)
    out[ref.idx] = ref.R
    out = out.reshape(2, 12, 2, 4)
    for rho in range(4):
        assert np.allclose(out[:, rho::4], ref.v[..., 4 * rho:4 * rho + 4])


CONV_CASES = sorted(n for n, (m, e, kw) in tg.GEMM_CASES.items() if kw.get("ntaps", 1) > 1 and e != "REFUSED")
STAT_CASES = sorted(n for n, (m, e, kw) in tg.GEMM_CASES.items() if kw.get("stats") and kw["nb"] > 1 and
                    kw.get("C_in", 0) <= 512)


@pytest.mark.parametrize("name", CONV_CASES)
def test_gemm_conv_mutations_detected(name):
    mode, _, kw = tg.GEMM_CASES[name]
    g = tg.build_gemm(sum(map(ord, name)), mode, **kw)
    ref = kr.gemm_ref(g, mode)
    # a conv tap shifted by one row
    m = kr.gemm_ref(g, mode, tap_shift=1)
    assert _exceeds(ref.v, m.v, ref.v_tol), "tap shift"
    if kw["nb"] > 1 or kw.get("flat"):
        # a batch boundary's zero padding replaced by the neighbour's row
        m = kr.gemm_ref(g, mode, pad_neighbour=True)
        assert _exceeds(ref.v, m.v, ref.v_tol), "neighbour padding"


@pytest.mark.parametrize("name", STAT_CASES)
def test_gemm_stats_mutation_detected(name):
    mode, _, kw = tg.GEMM_CASES[name]
    g = tg.build_gemm(sum(map(ord, name)), mode, **kw)
    ref = kr.gemm_ref(g, mode)
    m = kr.gemm_ref(g, mode, stats_shift=True)       # one row's statistics credited to the batch before
    assert _exceeds(ref.stats, m.stats, ref.stats_tol), (ref.stats, m.stats, ref.stats_tol)


def test_gemm_f32_emulation_within_tolerance():
    """an honest f32 evaluation (sequential f32 accumulation over K in 32-wide steps) stays inside (K + 16) e S"""
    g = tg.build_gemm(21, 1, nb=2, H_in=33, C_in=512, N=64)
    ref = kr.gemm_ref(g, 1)
    A = g.A.reshape(66, 512).astype(np.float32)
    W = g.Wp[:64, :512].astype(np.float32)
    acc = np.zeros((66, 64), dtype=np.float32)
    for k0 in range(0, 512, 32):
        acc = (acc + (A[:, k0:k0 + 32] @ W[:, k0:k0 + 32].T).astype(np.float32)).astype(np.float32)
    out = (acc + g.bias.astype(np.float32)).astype(np.float32)
    assert (np.abs(out.ravel() - ref.R) <= ref.tol).all()


# ------------------------------------------------------------------------------------------------ ConvTranspose
def test_convt_ref_matches_conv_transpose2d():
    import torch
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 7, 3, 12))
    wt = rng.standard_normal((12, 5, 8))
    bias = rng.standard_normal(5)
    R, tol, S, _ = kr.convt_ref(x, kr.convt_pack(wt), bias)
    y = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt)[..., None],
                                             torch.from_numpy(bias), stride=(4, 1), padding=(2, 0))
    exp = y.permute(0, 2, 3, 1).numpy()
    assert exp.shape == R.shape and np.abs(R - exp).max() < 1e-12
    Rd, Sd = kr.convt_ref_direct(x, wt, bias)
    assert np.abs(R - Rd).max() < 1e-12 and np.abs(S - Sd).max() < 1e-12


@pytest.mark.parametrize("nb,H,W", tg.CT_UNIT + tg.CT_WALK)
def test_convt_mutations_detected(nb, H, W):
    rng = np.random.default_rng(H * 100 + W)
    wt = kr.bf16_round(rng.standard_normal((96, 48, 8)) / np.sqrt(192.0))
    bias = 0.5 * rng.standard_normal(48)
    x = kr.bf16_round(rng.standard_normal((nb, H, W, 96)) * tg._bscale(nb, (1, 1, 1)))
    wp = kr.convt_pack(wt)
    R, tol, _, tol_acc = kr.convt_ref(x, wp, bias)
    for rho in range(4):                     # one residue's two taps swapped
        wm = wp.copy()
        wm[rho * 48:(rho + 1) * 48] = np.concatenate([wp[rho * 48:(rho + 1) * 48, 96:], wp[rho * 48:(rho + 1) * 48, :96]], 1)
        Rm = kr.convt_ref(x, wm, bias)[0]
        assert _exceeds(R[:, rho::4], Rm[:, rho::4], tol[:, rho::4])
    # a residue reading one input row off
    Rm = kr.convt_ref(x, wp, bias, res_off=(-1, -1, 0, -1))[0]
    assert _exceeds(R, Rm, tol)
    if nb > 1:                               # one row's statistics credited to the next item
        st, stt = kr.stats_of(R, tol_acc)
        row = R[0, -1]
        sm = st.copy()
        sm[0] -= [row.sum(), (row * row).sum()]
        sm[1] += [row.sum(), (row * row).sum()]
        assert _exceeds(st, sm, stt)


def test_convt_bf16_emulation_within_tolerance():
    """f32 accumulation of exact bf16 products, bf16 output: inside (192 + 16) e S + half a bf16 ulp (a flat u |R| with
    u = 2^-9 is exceeded by this honest evaluation: kernel_refs' docstring)"""
    rng = np.random.default_rng(2)
    wt = kr.bf16_round(rng.standard_normal((96, 48, 8)) / np.sqrt(192.0))
    bias = np.float32(0.5) * rng.standard_normal(48).astype(np.float32)
    x = kr.bf16_round(rng.standard_normal((2, 9, 3, 96)))
    wp = kr.convt_pack(wt)
    R, tol, _, _ = kr.convt_ref(x, wp, bias.astype(np.float64))
    xp = np.zeros((2, 11, 3, 96), dtype=np.float32)
    xp[:, 1:10] = x
    out = np.zeros_like(R)
    for rho in range(4):
        a = np.concatenate([xp[:, 1 + kr.RES_OFF[rho]:10 + kr.RES_OFF[rho]], xp[:, 2 + kr.RES_OFF[rho]:11 + kr.RES_OFF[rho]]], -1)
        acc = np.zeros(a.shape[:-1] + (48,), dtype=np.float32)
        w = wp[rho * 48:(rho + 1) * 48].astype(np.float32)
        for k0 in range(0, 192, 32):
            acc = (acc + a[..., k0:k0 + 32] @ w[:, k0:k0 + 32].T).astype(np.float32)
        out[:, rho::4] = kr.bf16_round((acc + bias).astype(np.float32))
    assert (np.abs(out - R) <= tol).all()


# ------------------------------------------------------------------------------------------------ LayerNorm
def test_layernorm_f32_emulation_within_tolerance():
    rng = np.random.default_rng(6)
    f = np.float32
    for C in (384, 512):
        x = rng.standard_normal((9, C)).astype(f)
        x[0] = 0.75
        x[1] = (1e3 + rng.standard_normal(C)).astype(f)
        w, b = (1 + 0.25 * rng.standard_normal(C)).astype(f), (0.1 * rng.standard_normal(C)).astype(f)
        y, tol = kr.layernorm_ref(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64))
        m = (x.sum(-1, keepdims=True, dtype=f) * f(1.0 / C)).astype(f)
        t = (x - m).astype(f)
        r = (f(1) / np.sqrt((t * t).sum(-1, keepdims=True, dtype=f) * f(1.0 / C) + f(1e-5))).astype(f)
        out = (t * r * w + b).astype(f)
        assert (np.abs(out - y) <= tol).all()


def test_bf16_output_term_is_half_an_ulp():
    """round to nearest reaches hulp16 at the bottom of a binade and u |R| = 2^-9 |R| would not cover it"""
    x = np.array([1.0 + 2.0 ** -8 - 1e-9, 0.7168, 3.99], dtype=np.float64)
    err = np.abs(kr.bf16_round(x) - x)
    assert (err <= kr.hulp16(x)).all() and (err[:2] > kr.U16 * x[:2]).all()
    assert list(kr.hulp16(np.array([1.0, 1.99, 2.0, 0.0, -0.75]))) == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0, 2.0 ** -9]
