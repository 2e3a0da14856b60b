"""Kernel-level parity: the launchers of csrc/gemm.h, attn.h and kernels.h against the float64 references and derived
tolerances of tests/kernel_refs.py, called through libathd_ktest.so (the exact objects libathd.so ships, plus the
ping-pong attention kernel of csrc/attn_pp.hip, which is built into the test library only).

Common rules: every device buffer has guard bands (operands: a large finite value, outputs: a sentinel) of at least a
tile of rows, untouched output elements must keep their sentinel, batches and heads are scaled by different powers
of two, and every shape is either computed within tolerance or refused with a nonzero code and an untouched output.
Each case records max(err / tol) in $ATHD_OUT/kernel_parity_report.json (default bench_out/).
"""
import os

import numpy as np
import pytest

import kernel_refs as kr

pytestmark = pytest.mark.gpu

LN2 = 0.6931471805599453
Q_PRESCALE = 0.125 * 1.4426950408889634


@pytest.fixture(scope="module")
def kt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    import ktest
    for name, (a, b) in ktest.sizes_match().items():
        assert a == b, (name, a, b)
    return ktest


def _bits_or_f32(vals, bf16):
    return kr.bf16_bits(np.asarray(vals, dtype=np.float32)) if bf16 else np.asarray(vals, dtype=np.float32)


def _vals(arr, bf16):
    return kr.bf16_value(arr).astype(np.float64) if bf16 else arr.astype(np.float64)


def _ratio(got, R, tol):
    bad = ~np.isfinite(got)
    r = np.abs(got - R) / np.maximum(tol, 1e-300)
    r[bad] = np.inf
    return float(r.max()) if r.size else 0.0


def _check_output(buf, init, idx, R, tol, bf16):
    """max err/tol over the stored elements; every other element and the bands must be untouched"""
    got_raw, bands = buf.host()
    assert bands, "guard band overwritten"
    touched = np.zeros(got_raw.size, dtype=bool)
    touched[idx] = True
    assert touched.sum() == idx.size, "reference stores an element twice"
    same = got_raw[~touched] == init[~touched]
    assert same.all(), "%d elements outside the kernel's output were written" % int((~same).sum())
    return _ratio(_vals(got_raw, bf16)[idx], R, tol)


# =====================================================================================================  attention
ATTN_PAIRS = [(1, 1), (33, 1), (31, 8), (127, 63), (128, 64), (129, 65), (128, 127), (257, 129), (257, 200), (1, 64),
              (16, 65), (64, 128), (65, 192), (130, 193), (200, 257), (255, 130), (256, 64), (257, 66),
              # many key tiles (attn_pp_kernel's 4-slot rings wrap twice): 10 tiles with a 1-key tail and two 256-query
              # blocks; 8 full tiles, no tail, a third 256-query block holding a single query
              (300, 577), (513, 512)]
NB, HEADS = 2, 8


def _attn_inputs(rng, Nq, Nk, mult, place, bf16):
    q = rng.standard_normal((NB, HEADS, Nq, 64))
    k = rng.standard_normal((NB, HEADS, Nk, 64))
    v = rng.standard_normal((NB, HEADS, Nk, 64))
    if place == "first" or place == "last":     # every query's largest logit at one key of the first / last tile
        j = 0 if place == "first" else Nk - 1
        q[..., 0] = np.abs(q[..., 0]) + 2.0
        k[:, :, j, :] = 0.0
        k[:, :, j, 0] = 12.0
    if place == "kzero":
        k[:] = 0.0
    q = q * mult * (Q_PRESCALE if bf16 else 1.0)
    # batches and heads at different powers of two: another head's or batch's V is a gross error
    v = v * (2.0 ** (np.arange(NB * HEADS).reshape(NB, HEADS, 1, 1) - 8))
    return kr.bf16_round(q), kr.bf16_round(k), kr.bf16_round(v)


def _attn_run(kt, q, k, v, layout, bf16, mode, pp_prio=None):
    """-> (O [nb][H][Nq][64] float64, O bits/raw); pp_prio: attn_pp_kernel<pp_prio> instead of attn_launch(mode)"""
    Nq, Nk = q.shape[2], k.shape[2]
    tok = lambda x: np.transpose(x, (0, 2, 1, 3)).reshape(NB, x.shape[2], 512)     # [nb][N][512]
    big = 3.0e38
    if layout == "qkv":
        N = max(Nq, Nk)
        h = np.full((NB, N, 1536), big)
        h[:, :Nq, 0:512] = tok(q)
        h[:, :Nk, 512:1024] = tok(k)
        h[:, :Nk, 1024:1536] = tok(v)
        bq = bk = kt.Buf(_bits_or_f32(h, bf16), "bf16" if bf16 else "f32", 128 * 1536)
        lay = dict(Q=bq.ptr, q_bs=N * 1536, q_ld=1536, q_off=0, K=bq.ptr, k_bs=N * 1536, k_ld=1536, k_off=512,
                   V=bq.ptr, v_bs=N * 1536, v_ld=1536, v_off=1024)
    else:
        hk = np.full((NB, Nk, 1024), big)
        hk[:, :, 0:512] = tok(k)
        hk[:, :, 512:1024] = tok(v)
        bq = kt.Buf(_bits_or_f32(tok(q), bf16), "bf16" if bf16 else "f32", 128 * 512)
        bk = kt.Buf(_bits_or_f32(hk, bf16), "bf16" if bf16 else "f32", 128 * 1024)
        lay = dict(Q=bq.ptr, q_bs=Nq * 512, q_ld=512, q_off=0, K=bk.ptr, k_bs=Nk * 1024, k_ld=1024, k_off=0,
                   V=bk.ptr, v_bs=Nk * 1024, v_ld=1024, v_off=512)
    o_init = np.zeros(NB * Nq * 512)
    bo = kt.Buf(o_init, "bf16" if bf16 else "f32", 128 * 512, output=True)
    b = int(bool(bf16))
    d = kt.fill(kt.KtAttn, q_bf16=b, k_bf16=b, v_bf16=b, o_bf16=b, O=bo.ptr, o_bs=Nq * 512, o_ld=512, nb=NB, Nq=Nq,
                Nk=Nk, heads=HEADS, scale_bits=kt.f32_bits(LN2 if bf16 else 0.125), **lay)
    import ctypes
    rc = kt.lib.kt_attn(ctypes.byref(d), mode, None) if pp_prio is None else kt.lib.kt_attn_pp(ctypes.byref(d), pp_prio, None)
    kt.sync()
    assert rc == 0, rc
    raw, bands = bo.host()
    assert bands, "guard band of O overwritten"
    o = _vals(raw, bf16).reshape(NB, Nq, HEADS, 64).transpose(0, 2, 1, 3)
    return o, raw


ATTN_VARIANTS = [(1, "rand"), (36, "rand"), (400, "rand"), (1, "first"), (36, "first"), (400, "first"), (1, "last"),
                 (36, "last"), (400, "last"), (1, "kzero")]


@pytest.mark.parametrize("layout", ["qkv", "q_kv"])
@pytest.mark.parametrize("Nq,Nk", ATTN_PAIRS)
def test_attn_bf16(kt, Nq, Nk, layout):
    """attn32_kernel<3,2,true> within tol = 4u (P|V|) + 2u |R|, and attn_pp_kernel<1>, <0> and <2> (kt_attn_pp)
    bit-identical to it."""
    rng = np.random.default_rng(1000 * Nq + Nk)
    worst = 0.0
    for mult, place in ATTN_VARIANTS:
        q, k, v = _attn_inputs(rng, Nq, Nk, mult, place, True)
        R, tol = kr.attn_ref(q, k, v, LN2, 1)
        if place == "kzero":
            assert np.abs(R - v.mean(axis=2, keepdims=True)).max() < 1e-12 * np.abs(v).max()
        o0, raw0 = _attn_run(kt, q, k, v, layout, True, 1)
        r = _ratio(o0, R, tol)
        print("attn bf16 Nq=%d Nk=%d %s x%d %s: err/tol %.3f" % (Nq, Nk, layout, mult, place, r))
        worst = max(worst, r)
        for prio in (1, 0, 2):
            _, raw = _attn_run(kt, q, k, v, layout, True, 1, pp_prio=prio)
            assert np.array_equal(raw, raw0), "attn_pp_kernel<%d> differs from attn32_kernel (x%d %s)" % (prio, mult, place)
    kt.record("attn_bf16[%d,%d,%s]" % (Nq, Nk, layout), err_over_tol=worst, pp_bit_identical=True)
    assert worst <= 1.0


@pytest.mark.parametrize("layout", ["qkv", "q_kv"])
@pytest.mark.parametrize("Nq,Nk", ATTN_PAIRS)
def test_attn_f32(kt, Nq, Nk, layout):
    """attn_kernel<0> within tol = (Nk + 96) e (1 + max_j |s_ij|) (P|V|)"""
    rng = np.random.default_rng(2000 * Nq + Nk)
    worst = 0.0
    for mult, place in ATTN_VARIANTS:
        q, k, v = _attn_inputs(rng, Nq, Nk, mult, place, False)
        R, tol = kr.attn_ref(q, k, v, 0.125, 0)
        o, _ = _attn_run(kt, q, k, v, layout, False, 0)
        r = _ratio(o, R, tol)
        print("attn f32 Nq=%d Nk=%d %s x%d %s: err/tol %.3f" % (Nq, Nk, layout, mult, place, r))
        worst = max(worst, r)
    kt.record("attn_f32[%d,%d,%s]" % (Nq, Nk, layout), err_over_tol=worst)
    assert worst <= 1.0


def test_attn_refuses_wide_pitch(kt):
    """a K / V row pitch of 2^23 elements or more does not fit the LDS-DMA staging's 24-bit offsets: bf16 mode refuses
    it (no launch) instead of computing with a wrapped pitch, and so does every form of attn_pp_kernel"""
    import ctypes
    bo = kt.Buf(np.full(512, kt.BF16_SENTINEL_BITS, dtype=np.uint16), "bf16", 512, output=True)
    bq = kt.Buf(np.zeros(1536, dtype=np.uint16), "bf16", 1536)
    d = kt.fill(kt.KtAttn, q_bf16=1, k_bf16=1, v_bf16=1, o_bf16=1, O=bo.ptr, o_bs=512, o_ld=512, nb=1, Nq=1, Nk=1,
                heads=8, scale_bits=kt.f32_bits(LN2), Q=bq.ptr, q_ld=1536, K=bq.ptr, k_ld=1 << 23, k_off=512, V=bq.ptr,
                v_ld=1 << 23, v_off=1024)
    for launch in (lambda: kt.lib.kt_attn(ctypes.byref(d), 1, None),) + tuple(
            (lambda p=p: kt.lib.kt_attn_pp(ctypes.byref(d), p, None)) for p in (1, 0, 2)):
        rc = launch()
        kt.sync()
        assert rc != 0
        raw, bands = bo.host()
        assert bands and (raw == kt.BF16_SENTINEL_BITS).all()


# =====================================================================================================  GEMM
def _roundup(a, b):
    return (a + b - 1) // b * b


def _bscale(nb, shape_tail):
    """a different power of two for neighbouring batches (period 5)"""
    return 2.0 ** (np.arange(nb) % 5).reshape((nb,) + (1,) * len(shape_tail))


def _gn_stats(nb, count, rng):
    """plausible {sum, sumsq} per batch: mean and variance differ per batch"""
    mean = 0.25 * (np.arange(nb) + 1) * np.where(np.arange(nb) % 2, -1.0, 1.0)
    var = 0.5 * 4.0 ** np.arange(nb)
    return np.stack([mean * count, (var + mean * mean) * count], axis=-1)


def build_gemm(seed, mode, *, nb, H_in, W=1, C_in, N, ntaps=1, in_stride=1, in_off=0, dil=1, H_out=None, a_bf16=1,
               flat=False, a_norm=False, a_gn=False, Kp=None, bias=True, c_bf16=0, act=kr.ACT_NONE, res=None,
               res_bf16=0, res_scale=False, res_gn=False, row_add=False, stats=False, gn=False, store=1, c4=False,
               convt=None, pbias=False, pfold=1, res_div=1, ln=None, sk=False):
    """A call-site form of the forward (csrc/forward_*.cpp) at reduced size, as a kernel_refs.gemm_spec with host
    arrays."""
    rng = np.random.default_rng(seed)
    H_out = H_in if H_out is None else H_out
    K = ntaps * C_in
    Kp = _roundup(K, 64) if Kp is None else Kp
    g = kr.gemm_spec(nb=nb, H_in=H_in, W=W, C_in=C_in, N=N, K=K, Kp=Kp, ntaps=ntaps, in_stride=in_stride, in_off=in_off,
                     dil=dil, H_out=H_out, a_bf16=a_bf16, c_bf16=c_bf16, act=act, store=store, res_bf16=res_bf16,
                     pfold=pfold, res_div=res_div, sk=sk, c4=c4)
    a = rng.standard_normal((nb, H_in, W, C_in)) * _bscale(nb, (1, 1, 1))
    if flat:        # [nb][W][H_in][C_in]: the (tap, ci) row of one position is contiguous (a_hs == C_in)
        g.a_ld, g.a_hs, g.a_bs = H_in * C_in, C_in, W * H_in * C_in
        a = np.ascontiguousarray(np.transpose(a, (0, 2, 1, 3)))
    else:
        g.a_ld = C_in
    g.A = kr.bf16_round(a) if (a_bf16 or mode == 1) and not (a_norm or a_gn) else a.astype(np.float32).astype(np.float64)
    if a_norm:
        g.a_norm = np.stack([0.125 * (np.arange(nb) + 1), 2.0 ** np.arange(nb) * 1.5], axis=-1)
    if a_gn:
        g.a_gn_stats = _gn_stats(nb, H_in * W * C_in, rng) * np.stack([2.0 ** np.arange(nb), 4.0 ** np.arange(nb)], -1)
        g.a_gn_count = H_in * W * C_in
        g.a_gn_w = (1.0 + 0.25 * rng.standard_normal(C_in)).astype(np.float32).astype(np.float64)
        g.a_gn_b = (0.1 * rng.standard_normal(C_in)).astype(np.float32).astype(np.float64)
    w = np.zeros((_roundup(N, 256), Kp))
    w[:N, :K] = rng.standard_normal((N, K)) / np.sqrt(K)
    if convt is not None and convt[0] == "quad" and C_in % 32 == 0:
        # the four-residue packing: residues 0 / 1 have no taps on row u + 1, residues 2 / 3 none on row u - 1
        w[:N // 2, 2 * C_in:] = 0.0
        w[N // 2:N, :C_in] = 0.0
    g.Wp = kr.bf16_round(w) if mode == 1 else w.astype(np.float32).astype(np.float64)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    if bias:
        g.bias = f32(0.5 * rng.standard_normal(N))
    Nout = N // 2 if act == kr.ACT_GLU else N
    g.ldo = Nout
    g.H_out_total = H_out
    if convt is not None:      # ConvTranspose residue groups of cout columns (forward_dec.cpp conv_t)
        kind, keep = convt
        cout = N // 4 if kind == "quad" else N // 2
        g.col_split, g.ldo = cout, cout
        if kind == "quad":
            g.hi_row_off = 1
            if C_in % 32 == 0:
                g.k_blk = C_in
            if not keep:
                g.H_out_total, g.o_stride, g.o_off, g.store_mask = 4 * H_in, 4, 0, 15
            else:
                g.H_out_total, g.o_stride, g.o_off, g.store_mask = 2 * H_in, 2, -1, 6
        else:
            pi = 0 if kind == "pair01" else 1
            if not keep:
                g.H_out_total, g.o_stride, g.o_off, g.hi_row_off, g.store_mask = 4 * H_in, 4, 2 * pi, 1, 3
            else:
                g.H_out_total, g.o_stride = 2 * H_in, 2
                if pi == 0:
                    g.o_off, g.hi_row_off, g.store_mask = 0, 0, 2
                else:
                    g.o_off, g.store_mask = 1, 1
    nbo = nb * (pfold if pbias else 1)
    g.c_elems = nbo * g.H_out_total * W * g.ldo
    if pbias:
        g.pbias = f32(rng.standard_normal((nbo, N)) * _bscale(nbo, (1,)) * 0.25)
    if gn:
        g.gn_stats = _gn_stats(nbo, H_out * W * N, rng)
        g.gn_count = H_out * W * N
        g.gn_w = f32(1.0 + 0.25 * rng.standard_normal(N))
        g.gn_b = f32(0.1 * rng.standard_normal(N))
    if row_add:
        g.row_add = f32(rng.standard_normal((H_out, Nout)))
    if res is not None:
        nres = nbo // res_div if res_div > 1 else nbo
        r = rng.standard_normal((nres, g.H_out_total * W * g.ldo)) * _bscale(nres, (1,))
        g.res = kr.bf16_round(r) if res_bf16 else f32(r)
        g.res_alias = res == "alias"
        if res_div > 1:
            g.res_bs = g.H_out_total * W * g.ldo
        if res_scale:
            g.res_scale = f32(0.5 + 0.25 * rng.standard_normal(Nout))
        if res_gn:
            g.res_gn_stats = _gn_stats(nbo, H_out * W * N, rng) * np.stack([2.0 ** np.arange(nbo), 4.0 ** np.arange(nbo)], -1)
            g.res_gn_count = H_out * W * N
            g.res_gn_w = f32(1.0 + 0.25 * rng.standard_normal(N))
            g.res_gn_b = f32(0.1 * rng.standard_normal(N))
    else:
        g.res_alias = False
    if stats:
        g.stats = np.stack([0.5 * (np.arange(nbo) + 1), 3.0 * (np.arange(nbo) + 1)], axis=-1)   # nonzero start values
    if ln is not None:
        g.ln_w = f32(1.0 + 0.25 * rng.standard_normal(N))
        g.ln_b = f32(0.1 * rng.standard_normal(N))
        g.ln_out = ln == "out"
    return g


def gemm_desc(kt, g, mode, bufs):
    """device buffers (with guard bands) + the flat descriptor for g"""
    def up(name, arr, kind, guard, output=False):
        if arr is None:
            return 0
        host = kr.bf16_bits(np.asarray(arr, dtype=np.float32)) if kind == "bf16" else arr
        bufs[name] = kt.Buf(host, kind, guard, output)
        return bufs[name].ptr

    rows = 256
    a_kind = "bf16" if g.a_bf16 else "f32"
    w_kind = "bf16" if mode == 1 else "f32"
    c_kind = "bf16" if g.c_bf16 else "f32"
    kw = dict(a_bf16=g.a_bf16, nb=g.nb, H_in=g.H_in, W=g.W, C_in=g.C_in, a_ld=g.a_ld, a_cs=g.a_cs, a_bs=g.a_bs,
              a_hs=g.a_hs, ntaps=g.ntaps, in_stride=g.in_stride, in_off=g.in_off, dil=g.dil, H_out=g.H_out,
              a_gn_count=g.a_gn_count, N=g.N, K=g.K, Kp=g.Kp, c_bf16=g.c_bf16, H_out_total=g.H_out_total,
              o_stride=g.o_stride, o_off=g.o_off, ldo=g.ldo, col_off=g.col_off, c_bs=g.c_bs, store=g.store,
              col_split=g.col_split, hi_row_off=g.hi_row_off, store_mask=g.store_mask, k_blk=g.k_blk, act=g.act,
              res_bf16=g.res_bf16, res_gn_count=g.res_gn_count, gn_count=g.gn_count, pfold=g.pfold, res_div=g.res_div,
              res_bs=g.res_bs)
    kw["A"] = up("A", g.A, a_kind, rows * max(g.a_ld, g.C_in) * max(g.W if g.a_hs < 0 else 1, 1))
    kw["Wp"] = up("Wp", g.Wp, w_kind, rows * g.Kp)
    for f in ("a_norm", "a_gn_w", "a_gn_b", "bias", "res_scale", "res_gn_w", "res_gn_b", "row_add", "gn_w", "gn_b",
              "pbias", "ln_w", "ln_b"):
        kw[f] = up(f, getattr(g, f), "f32", 1024)
    for f in ("a_gn_stats", "res_gn_stats", "gn_stats"):
        kw[f] = up(f, getattr(g, f), "f64", 64)
    if g.stats is not None:
        kw["stats"] = up("stats", g.stats, "f64", 64, output=True)
    guard_c = rows * g.ldo * g.W
    if g.res is not None and g.res_alias:
        c_init = _bits_or_f32(g.res, g.c_bf16).ravel()
        assert g.res_bf16 == g.c_bf16 and c_init.size == g.c_elems
    else:
        c_init = np.full(g.c_elems, kt.BF16_SENTINEL_BITS if g.c_bf16 else kt.F32_SENTINEL,
                         dtype=np.uint16 if g.c_bf16 else np.float32)
    bufs["C"] = kt.Buf(c_init, c_kind, guard_c, output=True)
    bufs["c_init"] = c_init
    kw["C"] = bufs["C"].ptr
    if g.res is not None:
        kw["res"] = bufs["C"].ptr if g.res_alias else up("res", g.res, "bf16" if g.res_bf16 else "f32", guard_c)
    M = g.nb * g.H_out * g.W
    if g.c4:
        bufs["c4_init"] = np.full(M * 4, kt.BF16_SENTINEL_BITS if g.c_bf16 else kt.F32_SENTINEL,
                                  dtype=np.uint16 if g.c_bf16 else np.float32)
        bufs["c4"] = kt.Buf(bufs["c4_init"], c_kind, rows * 4, output=True)
        kw["c4"] = bufs["c4"].ptr
    if g.ln_out:
        bufs["ln_init"] = np.full(M * g.N, kt.BF16_SENTINEL_BITS, dtype=np.uint16)
        bufs["ln_out"] = kt.Buf(bufs["ln_init"], "bf16", rows * g.N, output=True)
        kw["ln_out"] = bufs["ln_out"].ptr
    if g.sk:
        import torch
        bufs["sk"] = torch.zeros(kt.lib.kt_sk_bytes() // 4 + 2 * 65536, dtype=torch.float32, device="cuda")
        kw["sk_ws"] = bufs["sk"].data_ptr() + 65536 * 4
    return kt.fill(kt.KtGemm, **kw)


def run_gemm(kt, g, mode, case, ref=None):
    """correct within tolerance, or refused with the output untouched; -> route name"""
    import ctypes
    bufs = {}
    d = gemm_desc(kt, g, mode, bufs)
    route = kt.ROUTES[kt.lib.kt_gemm_route(ctypes.byref(d), mode)]
    rc = kt.lib.kt_gemm(ctypes.byref(d), mode, None)
    kt.sync()
    if route == "REFUSED" or rc != 0:
        assert route == "REFUSED" and rc != 0, (route, rc)
        raw, bands = bufs["C"].host()
        assert bands and np.array_equal(raw, bufs["c_init"]), "refused launch wrote to C"
        kt.record(case, route=route, refused=True)
        return route
    ref = kr.gemm_ref(g, mode) if ref is None else ref
    worst = {}
    if g.store:
        worst["C"] = _check_output(bufs["C"], bufs["c_init"], ref.idx, ref.R, ref.tol, g.c_bf16)
    else:
        raw, bands = bufs["C"].host()
        assert bands and np.array_equal(raw, bufs["c_init"]), "store = 0 wrote to C"
    if g.c4:
        worst["c4"] = _check_output(bufs["c4"], bufs["c4_init"], ref.c4_idx, ref.c4_R, ref.c4_tol, g.c_bf16)
    if g.ln_out:
        worst["ln_out"] = _check_output(bufs["ln_out"], bufs["ln_init"], np.arange(ref.ln_R.size), ref.ln_R.ravel(),
                                        ref.ln_tol.ravel(), True)
    if g.stats is not None:
        st, bands = bufs["stats"].host()
        assert bands, "statistics written outside the batches"
        worst["stats"] = _ratio(st.reshape(-1, 2) - g.stats, ref.stats, ref.stats_tol)
    print("gemm %s mode %d route %s: err/tol %s" % (case, mode, route, worst))
    kt.record(case, route=route, err_over_tol=worst)
    assert worst and max(worst.values()) <= 1.0, worst
    return route


def _m_edges(bm):
    """(nb, rows per batch): BM - 1 and BM + 1 rows in one batch; three batches of BM / 2 + 5 rows (tiles straddle two
    and three batches)"""
    return [(1, bm - 1), (1, bm + 1), (3, bm // 2 + 5)]


GEMM_CASES = {}


def _case(name, mode, expect=None, **kw):
    GEMM_CASES[name] = (mode, expect, kw)


# dense linear layers (forward.h lin()): upsampler, q / kv / qkv, linear1, text.mlp0, downsampler
for _nb, _h in _m_edges(256):
    _case("upsampler[%dx%d]" % (_nb, _h), 1, "GEMM5", nb=_nb, H_in=_h, C_in=384, N=512)
    _case("qkv[%dx%d]" % (_nb, _h), 1, "GEMM5", nb=_nb, H_in=_h, C_in=512, N=1536, c_bf16=1)
    _case("linear1.gelu[%dx%d]" % (_nb, _h), 1, "GEMM5", nb=_nb, H_in=_h, C_in=512, N=512, c_bf16=1, act=kr.ACT_GELU)
    _case("out_proj[%dx%d]" % (_nb, _h), 1, "GEMM5", nb=_nb, H_in=_h, C_in=512, N=512, res="alias", res_scale=True)
    _case("linear2.stats[%dx%d]" % (_nb, _h), 1, "GEMM5", nb=_nb, H_in=_h, C_in=2048, N=512, res="alias", res_scale=True,
          stats=True)
    _case("k64.n320[%dx%d]" % (_nb, _h), 1, "GEMM3_V3", nb=_nb, H_in=_h, C_in=64, N=320, c_bf16=1)
    _case("k72.kp128.n192[%dx%d]" % (_nb, _h), 1, "GEMM3_V3", nb=_nb, H_in=_h, C_in=72, N=192, Kp=128)
_case("out_proj.res_gn[2x261]", 1, "GEMM5", nb=2, H_in=261, C_in=512, N=512, res="alias", res_scale=True, res_gn=True)
_case("out_proj.res_gn[3x256]", 1, "GEMM5", nb=3, H_in=256, C_in=512, N=512, res="alias", res_scale=True, res_gn=True)
_case("out_proj.res_gn.short[3x133]", 1, "REFUSED", nb=3, H_in=133, C_in=512, N=512, res="alias", res_scale=True,
      res_gn=True)
for _nb, _h in _m_edges(192):
    _case("text.mlp0[%dx%d]" % (_nb, _h), 1, "GEMM3_V7", nb=_nb, H_in=_h, C_in=384, N=384, bias=False, pbias=True, pfold=2,
          c_bf16=1, act=kr.ACT_GELU)
for _nb, _h in _m_edges(128):
    _case("downsampler.a_gn[%dx%d]" % (_nb, _h), 1, "GEMM2_AGN", nb=_nb, H_in=_h, C_in=512, N=384, a_bf16=0, a_gn=True)
    _case("linear.f32A.n48[%dx%d]" % (_nb, _h), 1, "GEMM2", nb=_nb, H_in=_h, C_in=64, N=48, a_bf16=0)
# rowln: out_proj + the next LayerNorm (144-row tiles); fewer rows per batch than a tile are refused
for _nb, _h in [(1, 143), (1, 145), (3, 150)]:
    _case("out_proj.ln[%dx%d]" % (_nb, _h), 1, "REFUSED" if _h < 144 else "ROWLN", nb=_nb, H_in=_h, C_in=512, N=512,
          res="alias", res_scale=True, ln="out")
_case("out_proj.ln.res_gn[3x150]", 1, "ROWLN", nb=3, H_in=150, C_in=512, N=512, res="alias", res_scale=True, res_gn=True,
      ln="out")
# the text mlp2 + norm_out (NI = 4 items of P = 2 prompts: residual batch = item / 2)
for _h in (145, 150):
    _case("text.mlp2.ln[4x%d]" % _h, 1, None, nb=4, H_in=_h, C_in=384, N=384, bias=False, pbias=True, res="sep", res_div=2,
          c_bf16=1, ln="epi")
# DConv: dilated 3-tap conv with statistics (narrow gemm2), the 1x1's statistics-only pass, GN + GLU + residual
for _dil in (1, 2):
    for _nb, _h in _m_edges(256):
        _case("dconv.conv3.d%d[%dx%d]" % (_dil, _nb, _h), 1, "GEMM2", nb=_nb, H_in=_h, C_in=192, N=24, ntaps=3,
              in_off=-_dil, dil=_dil, stats=True)
for _nb, _h in _m_edges(256):
    _case("dconv.conv3.n48[%dx%d]" % (_nb, _h), 1, "GEMM2", nb=_nb, H_in=_h, C_in=384, N=48, ntaps=3, in_off=-1,
          stats=True)
    _case("dconv.1x1.stats[%dx%d]" % (_nb, _h), 1, "GEMM3_V3", nb=_nb, H_in=_h, C_in=24, N=384, stats=True, store=0)
    _case("dconv.1x1.glu[%dx%d]" % (_nb, _h), 1, "GEMM3_V3", nb=_nb, H_in=_h, C_in=24, N=384, act=kr.ACT_GLU, gn=True,
          res="alias", res_bf16=1, c_bf16=1, res_scale=True)
    _case("dconv.1x1.glu.n768[%dx%d]" % (_nb, _h), 1, "GEMM5", nb=_nb, H_in=_h, C_in=48, N=768, act=kr.ACT_GLU, gn=True,
          res="alias", res_bf16=1, c_bf16=1, res_scale=True)
# encoders: the stride-4 8-tap conv + GELU (W = Tspec columns), level 0 with flat K on the f32 spectrogram, rewrite GLU
for _nb, _h, _w in [(1, 17, 15), (1, 37, 7), (3, 9, 5)]:
    _case("fenc.conv.l2[%dx%dx%d]" % (_nb, _h, _w), 1, "GEMM3_V7", nb=_nb, H_in=4 * _h, H_out=_h, W=_w, C_in=96, N=192,
          ntaps=8, in_stride=4, in_off=-2, c_bf16=1, act=kr.ACT_GELU)
for _nb, _h, _w in [(1, 16, 8), (1, 43, 3), (3, 23, 3)]:
    _case("fenc.conv.l0.flat[%dx%dx%d]" % (_nb, _h, _w), 1, "GEMM2", nb=_nb, H_in=4 * _h, H_out=_h, W=_w, C_in=4, N=48,
          ntaps=8, in_stride=4, in_off=-2, a_bf16=0, flat=True, a_norm=True, c_bf16=1, act=kr.ACT_GELU)
    _case("fenc.rewrite.l0[%dx%dx%d]" % (_nb, _h, _w), 1, "GEMM2", nb=_nb, H_in=_h, W=_w, C_in=48, N=96, act=kr.ACT_GLU,
          row_add=True, c4=True, c_bf16=1)
for _nb, _h in _m_edges(128):
    _case("tenc.conv.l1[%dx%d]" % (_nb, _h), 1, "GEMM2", nb=_nb, H_in=4 * _h - 1, H_out=_h, C_in=48, N=96, ntaps=8,
          in_stride=4, in_off=-2, c_bf16=1, act=kr.ACT_GELU)
# ConvTranspose residues as GEMM column groups (forward_dec.cpp conv_t): quad (k_blk) and pairs, all rows / kept rows
for _keep in (0, 1):
    for _nb, _h, _w in [(1, 8, 31), (3, 8, 11)]:
        _case("convt.quad.c192.keep%d[%dx%dx%d]" % (_keep, _nb, _h, _w), 1, "GEMM3_V7", nb=_nb, H_in=_h, W=_w, C_in=192,
              N=384, ntaps=3, in_off=-1, c_bf16=1, stats=True, convt=("quad", _keep))
        _case("convt.quad.c384.keep%d[%dx%dx%d]" % (_keep, _nb, _h, _w), 1, "GEMM5", nb=_nb, H_in=_h, W=_w, C_in=384,
              N=768, ntaps=3, in_off=-1, c_bf16=1, stats=True, convt=("quad", _keep))
        for _pi, _kind in enumerate(("pair01", "pair23")):
            _case("convt.%s.c48.keep%d[%dx%dx%d]" % (_kind, _keep, _nb, _h, _w), 1, "V1_BF16", nb=_nb, H_in=_h, W=_w,
                  C_in=48, N=8, ntaps=2, in_off=-1 + _pi, c_bf16=1, stats=True, convt=(_kind, _keep))
            _case("convt.%s.c96.keep%d[%dx%dx%d]" % (_kind, _keep, _nb, _h, _w), 1, "GEMM2", nb=_nb, H_in=_h, W=_w,
                  C_in=96, N=96, ntaps=2, in_off=-1 + _pi, c_bf16=1, stats=True, convt=(_kind, _keep))
# bf16 mode shapes no tuned kernel takes (gemm.hip's own bf16 tiles): N = 4 and 16
for _n in (4, 16):
    _case("v1.bf16.n%d[3x133]" % _n, 1, "V1_BF16", nb=3, H_in=133, C_in=48, N=_n)
# f32 parity mode: the four tile configurations of gemm.hip (N <= 16, <= 32, <= 64, > 64)
for _n, _bm in [(4, 256), (16, 256), (24, 256), (48, 128), (192, 128), (320, 128)]:
    for _nb, _h in _m_edges(_bm):
        _case("v1.f32.n%d[%dx%d]" % (_n, _nb, _h), 0, "V1_F32", nb=_nb, H_in=_h, C_in=72, N=_n, Kp=96, a_bf16=0,
              act=kr.ACT_GELU if _n == 48 else kr.ACT_NONE, stats=_n in (24, 192))
_case("v1.f32.conv3[3x69]", 0, "V1_F32", nb=3, H_in=69, C_in=48, N=24, ntaps=3, in_off=-2, dil=2, a_bf16=0, stats=True,
      Kp=160)
_case("v1.f32.glu.res[3x69]", 0, "V1_F32", nb=3, H_in=69, C_in=24, N=96, Kp=32, a_bf16=0, act=kr.ACT_GLU, gn=True,
      res="alias", res_scale=True)


@pytest.mark.parametrize("name", sorted(GEMM_CASES))
def test_gemm(kt, name):
    """gemm_launch on one call-site form of the forward (csrc/forward_*.cpp) at reduced size: tol = (K + 16) e S
    propagated through the epilogue (kernel_refs.gemm_ref), statistics by the sum rule; the route is recorded and,
    where the form pins it, asserted"""
    mode, expect, kw = GEMM_CASES[name]
    g = build_gemm(sum(map(ord, name)), mode, **kw)
    route = run_gemm(kt, g, mode, "gemm[%s]" % name)
    if expect is not None:
        assert route == expect, (route, expect)


@pytest.mark.parametrize("rlt", ["1", "0"])
@pytest.mark.parametrize("h", [145, 150])
def test_gemm_text_ln_forms(kt, rlt, h):
    """the text row-LayerNorm in both forms: rowln.hip's (ATHD_RLT=1) and gemm3's (ATHD_RLT=0)"""
    mode, _, kw = GEMM_CASES["text.mlp2.ln[4x%d]" % h]
    g = build_gemm(77 + h, mode, **kw)
    old = os.environ.get("ATHD_RLT")
    os.environ["ATHD_RLT"] = rlt
    try:
        route = run_gemm(kt, g, mode, "gemm[text.mlp2.ln 4x%d RLT=%s]" % (h, rlt))
    finally:
        if old is None:
            del os.environ["ATHD_RLT"]
        else:
            os.environ["ATHD_RLT"] = old
    assert route == ("ROWLN_TEXT" if rlt == "1" else "GEMM3_LN")


def test_gemm_routes_covered(kt):
    """every route but REFUSED is reached by at least one case of this file"""
    import ctypes
    seen = set()
    for name, (mode, expect, kw) in GEMM_CASES.items():
        if expect is not None:
            seen.add(expect)
    seen.update(["ROWLN_TEXT", "GEMM3_LN"])      # test_gemm_text_ln_forms asserts both
    missing = set(kt.ROUTES) - {"REFUSED"} - seen
    assert not missing, missing


# ---- split-K tail ----
def _sk_case(kt, rows_per_batch, nb, seed):
    g = build_gemm(seed, 1, nb=nb, H_in=rows_per_batch, C_in=2048, N=512, res="alias", res_scale=True, stats=True,
                   sk=True)
    return g


def _dense_res_ref(g):
    """out = res + rs (A W^T + bias) for the dense residual-stream form, in row chunks (the full-size split-K case)"""
    M = g.nb * g.H_out
    A = g.A.reshape(M, g.K)
    W = g.Wp[:g.N, :g.K]
    res = g.res.reshape(M, g.N)
    R = np.empty((M, g.N))
    tol = np.empty((M, g.N))
    aW = np.abs(W).T
    for r0 in range(0, M, 4096):
        a = A[r0:r0 + 4096]
        v = a @ W.T + g.bias
        S = np.abs(a) @ aW + np.abs(g.bias)
        t = (g.K + 16) * kr.E32 * S
        rr = res[r0:r0 + 4096]
        R[r0:r0 + 4096] = rr + g.res_scale * v
        tol[r0:r0 + 4096] = np.abs(g.res_scale) * t + 2 * kr.E32 * (np.abs(rr) + np.abs(g.res_scale * v))
    from types import SimpleNamespace
    st, stt = kr.stats_of(R.reshape(g.nb, -1), tol.reshape(g.nb, -1))
    return SimpleNamespace(idx=np.arange(M * g.N), R=R.ravel(), tol=tol.ravel(), stats=st, stats_tol=stt)


def test_gemm_splitk_tail(kt):
    """linear2 (N = 512, K = 2048, residual + statistics) sized from the plan so that the last round has about 10
    tiles: the split launch (gemm5_sk_reduce_kernel) and the unsplit one (sk_ws null) both match float64 on every row
    and in the statistics.  nb = 3 with rows per batch not a multiple of 4 (reduce blocks of 4 rows straddle batches).
    Fails if the plan reports no split."""
    import ctypes
    probe = build_gemm(5, 1, nb=3, H_in=300, C_in=2048, N=512, res="alias", res_scale=True, stats=True, sk=True)
    bufs = {}
    d = gemm_desc(kt, probe, 1, bufs)
    R = kt.lib.kt_sk_resident(ctypes.byref(d))
    assert R >= 64, "no resident-block count for the split-K kernel: %d" % R
    ntm = (R + 10 + 1) // 2                      # row tiles: 2 N tiles each -> tiles = R + 10 or R + 11
    hb = ntm * 256 // 3
    while hb % 4 == 0 or (3 * hb + 255) // 256 != ntm:
        hb -= 1
    del bufs, d
    g = _sk_case(kt, hb, 3, 11)
    ref = _dense_res_ref(g)
    # the plan for this shape
    bufs = {}
    d = gemm_desc(kt, g, 1, bufs)
    plan = (ctypes.c_int64 * 3)()
    kt.lib.kt_sk_plan(ctypes.byref(d), plan)
    full, tail, S = list(plan)
    del bufs, d
    assert S >= 2 and tail > 0, "no split on this device: R=%d M=%d plan=%s" % (R, 3 * hb, (full, tail, S))
    assert run_gemm(kt, g, 1, "gemm[linear2.splitk R=%d M=%d tail=%d S=%d]" % (R, 3 * hb, tail, S), ref=ref) == "GEMM5"
    g.sk = False
    assert run_gemm(kt, g, 1, "gemm[linear2.unsplit M=%d]" % (3 * hb), ref=ref) == "GEMM5"
    kt.record("splitk_plan", R=int(R), M=3 * hb, full=int(full), tail=int(tail), S=int(S))


def test_gemm_splitk_needs_four_rows_per_batch(kt):
    """fewer than 4 rows per batch: the reduce kernel's 4-row blocks would span more than two batches, so the plan
    must not split (and the launch is still right)"""
    import ctypes
    probe = build_gemm(5, 1, nb=3, H_in=300, C_in=512, N=512, res="alias", res_scale=True, sk=True)
    bufs = {}
    d = gemm_desc(kt, probe, 1, bufs)
    R = kt.lib.kt_sk_resident(ctypes.byref(d))
    del bufs, d
    assert R >= 64
    ntm = (R + 10 + 1) // 2
    nb = (ntm * 256 - 100) // 3
    g = build_gemm(13, 1, nb=nb, H_in=3, C_in=512, N=512, res="alias", res_scale=True, sk=True)
    bufs = {}
    d = gemm_desc(kt, g, 1, bufs)
    plan = (ctypes.c_int64 * 3)()
    kt.lib.kt_sk_plan(ctypes.byref(d), plan)
    d.H_in, d.H_out, d.H_out_total, d.nb = 3 * nb // 4, 3 * nb // 4, 3 * nb // 4, 4
    plan4 = (ctypes.c_int64 * 3)()
    kt.lib.kt_sk_plan(ctypes.byref(d), plan4)
    del bufs, d
    assert plan[2] == 1 and plan[1] == 0, list(plan)
    assert plan4[2] >= 2, "the same M with long batches should split: %s" % list(plan4)
    run_gemm(kt, g, 1, "gemm[linear2.splitk.short_batches nb=%d]" % nb, ref=_dense_res_ref(g))


# =====================================================================================================  norms
LN_ROWS = [1, 3, 15, 16, 17, 33]


def _ln_run(kt, x, nb, N, C, w, b, gn=None, gn_writeback=1, pos=None, out_bf16=0, w2=None, b2=None, inplace=False):
    import ctypes
    bufs = {}
    f = lambda name, arr, kind="f32", g=1024, out=False: bufs.setdefault(name, kt.Buf(arr, kind, g, out)).ptr
    kw = dict(nb=nb, N=N, C=C, gn_writeback=gn_writeback, out_bf16=out_bf16)
    kw["x"] = f("x", x, "f32", 16 * C, out=False)
    kw["w"], kw["b"] = f("w", w), f("b", b)
    if gn is not None:
        kw["gn_stats"], kw["gn_w"], kw["gn_b"] = f("gs", gn[0], "f64", 64), f("gw", gn[1]), f("gb", gn[2])
    if pos is not None:
        kw["pos"] = f("pos", pos, "f32", 16 * C)
    rows = nb * N
    okind = "bf16" if out_bf16 else "f32"
    init = np.full(rows * C, kt.BF16_SENTINEL_BITS if out_bf16 else kt.F32_SENTINEL, dtype=np.uint16 if out_bf16 else np.float32)
    kw["out"] = kw["x"] if inplace else f("out", init, okind, 16 * C, out=True)
    if w2 is not None:
        # (out2 has out's type: bf16 on the fused path, and the two-launch path's second launch writes out's type)
        kw["w2"], kw["b2"], kw["out2"] = f("w2", w2), f("b2", b2), f("out2", init, okind, 16 * C, out=True)
    d = kt.fill(kt.KtLn, **kw)
    rc = kt.lib.kt_layernorm(ctypes.byref(d), None)
    kt.sync()
    assert rc == 0
    res = {}
    for name in ("x", "out", "out2"):
        if name in bufs:
            raw, bands = bufs[name].host()
            assert bands, "guard band of %s overwritten" % name
            res[name] = _vals(raw, name != "x" and bool(out_bf16)).reshape(rows, C)
    return res


@pytest.mark.parametrize("C", [512, 384])
@pytest.mark.parametrize("N", LN_ROWS)
def test_layernorm(kt, C, N):
    """layernorm_launch against tol = 16e (|v| + |mean|) rstd |w| + 4e (|y| + |b| + |pos|) (+ half a bf16 ulp): plain, positional
    table, pending GroupNorm with and without write-back, out2 (fused and two-launch), a constant row and a row with
    mean 1e3 and std 1"""
    nb = 2
    rng = np.random.default_rng(C + N)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    x = f32(rng.standard_normal((nb, N, C)) * _bscale(nb, (1, 1)))
    x[0, 0] = 0.75                                     # a constant row
    x[1, N - 1] = f32(1e3 + rng.standard_normal(C))    # mean 1e3, std 1
    w, b = f32(1 + 0.25 * rng.standard_normal(C)), f32(0.1 * rng.standard_normal(C))
    w2, b2 = f32(1 + 0.25 * rng.standard_normal(C)), f32(0.1 * rng.standard_normal(C))
    pos = f32(rng.standard_normal((N, C)))
    gn = (_gn_stats(nb, N * C, rng), f32(1 + 0.25 * rng.standard_normal(C)), f32(0.1 * rng.standard_normal(C)))
    gm, gr = kr.gn_params(gn[0], N * C)
    xg = (x - gm[:, None, None]) * gr[:, None, None] * gn[1] + gn[2]
    # the GroupNorm in f32 ahead of the LayerNorm: 4e of its terms, propagated as an input bound
    xg_tol = 4 * kr.E32 * (np.abs(xg) + np.abs(gn[2]) + np.abs(gm[:, None, None]) * gr[:, None, None] * np.abs(gn[1]))
    worst = {}
    flat = lambda a: a.reshape(nb * N, C)
    posr = np.tile(pos, (nb, 1))
    for out_bf16 in (0, 1):
        for use_pos in (False, True):
            y, tol = kr.layernorm_ref(flat(x), w, b, pos=posr if use_pos else None, out_bf16=bool(out_bf16))
            got = _ln_run(kt, x, nb, N, C, w, b, pos=pos if use_pos else None, out_bf16=out_bf16)
            worst["plain bf16=%d pos=%d" % (out_bf16, use_pos)] = _ratio(got["out"], y, tol)
            assert np.array_equal(got["x"], flat(x))
        for wb in (1, 0):
            y, tol = kr.layernorm_ref(flat(xg), w, b, out_bf16=bool(out_bf16), d_in=flat(xg_tol))
            got = _ln_run(kt, x, nb, N, C, w, b, gn=gn, gn_writeback=wb, out_bf16=out_bf16)
            worst["gn wb=%d bf16=%d" % (wb, out_bf16)] = _ratio(got["out"], y, tol)
            if wb == 0 and C == 512:
                assert np.array_equal(got["x"], flat(x)), "gn_writeback = 0 changed x"
            else:          # (C = 384 has no register-only form: layernorm_launch writes back)
                worst["gn x wb=%d bf16=%d" % (wb, out_bf16)] = _ratio(got["x"], flat(xg), flat(xg_tol))
    # in place (the input LayerNorms: out == x, f32)
    y, tol = kr.layernorm_ref(flat(x), w, b, pos=posr)
    got = _ln_run(kt, x, nb, N, C, w, b, pos=pos, inplace=True)
    worst["inplace"] = _ratio(got["x"], y, tol)
    # out2: fused (C = 512, bf16, no pos) and the two-launch path (f32 out or pos)
    for out_bf16, use_pos, use_gn in ((1, False, False), (1, False, True), (0, False, True), (1, True, False)):
        src, d_in = (flat(xg), flat(xg_tol)) if use_gn else (flat(x), None)
        y, tol = kr.layernorm_ref(src, w, b, pos=posr if use_pos else None, out_bf16=bool(out_bf16), d_in=d_in)
        y2, tol2 = kr.layernorm_ref(src, w2, b2, out_bf16=bool(out_bf16), d_in=d_in)
        got = _ln_run(kt, x, nb, N, C, w, b, gn=gn if use_gn else None, pos=pos if use_pos else None, out_bf16=out_bf16,
                      w2=w2, b2=b2)
        key = "out2 bf16=%d pos=%d gn=%d" % (out_bf16, use_pos, use_gn)
        worst[key] = _ratio(got["out"], y, tol)
        worst[key + " (2)"] = _ratio(got["out2"], y2, tol2)
    print("layernorm C=%d N=%d: %s" % (C, N, worst))
    kt.record("layernorm[%d,%d]" % (C, N), err_over_tol=worst)
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


@pytest.mark.parametrize("n", [8, 8 * (4096 * 256 + 1000)])
def test_to_bf16(kt, n):
    """to_bf16_launch is bit-exact round-to-nearest-even: ties both ways, denormals, +-0, the largest finite value,
    +-inf; n = 8 and n large enough that the 4096-block grid strides"""
    rng = np.random.default_rng(n % 1000)
    x = rng.standard_normal(n).astype(np.float32)
    special = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x00000001, 0x00008000,
                        0x00018000, 0x807FFFFF, 0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F800000,
                        0xFF800000, 0x7F7F8000], dtype=np.uint32).view(np.float32)
    if n == 8:
        cases = [special[0:8], special[8:16], np.concatenate([special[16:], x[:6]])]
    else:
        x[:special.size] = special
        x[-special.size:] = special
        x[n // 2:n // 2 + special.size] = special
        cases = [x]
    for c in cases:
        bx = kt.Buf(c, "f32", 4096)
        by = kt.Buf(np.full(c.size, kt.BF16_SENTINEL_BITS, dtype=np.uint16), "bf16", 4096, output=True)
        assert kt.lib.kt_to_bf16(bx.ptr, by.ptr, c.size, None) == 0
        kt.sync()
        got, bands = by.host()
        assert bands
        assert np.array_equal(got, kr.bf16_bits(c))
    kt.record("to_bf16[%d]" % n, bit_exact=True)


@pytest.mark.parametrize("per_batch_rows", [31, 32, 33, 171])
def test_groupnorm_passes(kt, per_batch_rows):
    """gn_gelu (both GELU forms), gn_gelu_bf16, gn_apply against GN in float64 with the f32 rule: the affine form
    (v - m) r w + b costs 4e of its terms, GELU multiplies by 1.13 and adds 8e |v| (+ 4.8e-4 for the fast form), a
    bf16 output half a bf16 ulp.  Row counts on both sides of one 256-thread block (H = 24: 32 rows = 768 elements = 3 per thread)."""
    nb, H = 3, 24
    per = per_batch_rows * H
    rng = np.random.default_rng(per)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    h = f32(rng.standard_normal((nb, per_batch_rows, H)) * _bscale(nb, (1, 1)))
    st = np.stack([h.reshape(nb, -1).sum(1), (h.reshape(nb, -1) ** 2).sum(1)], -1)
    w, b = f32(1 + 0.25 * rng.standard_normal(H)), f32(0.1 * rng.standard_normal(H))
    gm, gr = kr.gn_params(st, per)
    c = (h - gm[:, None, None]) * gr[:, None, None] * w
    v = c + b
    vt = 4 * kr.E32 * (np.abs(c) + np.abs(b) + np.abs(gm[:, None, None]) * gr[:, None, None] * np.abs(w))
    y = kr.gelu(v)
    worst = {}
    up = lambda: (kt.Buf(st, "f64", 64), kt.Buf(w, "f32", 256), kt.Buf(b, "f32", 256))
    for fast in (0, 1):
        bs, bw, bb = up()
        bh = kt.Buf(h, "f32", 256 * H, output=False)
        assert kt.lib.kt_gn_gelu(bh.ptr, nb, per, H, bs.ptr, bw.ptr, bb.ptr, fast, None) == 0
        kt.sync()
        got, bands = bh.host()
        assert bands
        tol = 1.13 * vt + 8 * kr.E32 * np.abs(v) + (kr.GELU_FAST_ABS if fast else 0.0)
        worst["gn_gelu fast=%d" % fast] = _ratio(got.astype(np.float64), y.ravel(), tol.ravel())
    bs, bw, bb = up()
    bh = kt.Buf(h, "f32", 256 * H)
    bo = kt.Buf(np.full(h.size, kt.BF16_SENTINEL_BITS, dtype=np.uint16), "bf16", 256 * H, output=True)
    assert kt.lib.kt_gn_gelu_bf16(bh.ptr, bo.ptr, nb, per, H, bs.ptr, bw.ptr, bb.ptr, None) == 0
    kt.sync()
    got, bands = bo.host()
    assert bands
    tol = 1.13 * vt + 8 * kr.E32 * np.abs(v) + kr.GELU_FAST_ABS
    tol = tol + kr.hulp16(np.abs(y) + tol)
    worst["gn_gelu_bf16"] = _ratio(_vals(got, True), y.ravel(), tol.ravel())
    bs, bw, bb = up()
    bh = kt.Buf(h, "f32", 256 * H)
    assert kt.lib.kt_gn_apply(bh.ptr, nb, per_batch_rows, H, bs.ptr, bw.ptr, bb.ptr, None) == 0
    kt.sync()
    got, bands = bh.host()
    assert bands
    worst["gn_apply"] = _ratio(got.astype(np.float64), v.ravel(), vt.ravel())
    print("groupnorm passes rows=%d: %s" % (per_batch_rows, worst))
    kt.record("groupnorm[%d]" % per_batch_rows, err_over_tol=worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("n", [255, 256, 257, 100003])
def test_stats_and_input_norm(kt, n):
    """stats_launch: per-batch {sum, sumsq} in fp64 of f32 data.  Every element enters as an exact double and its
    square is exact in double (24-bit significands), so only the additions round: n - 1 of them in any order, each
    2^-53 relative to a partial sum bounded by the sum of magnitudes: |dsum| <= n 2^-53 sum|x|, |dsumsq| <= n 2^-53
    sum x^2.  input_norm_params_launch: (mean, 1e-5 + unbiased std) and (mean, std) as floats, 4e relative on top
    of the statistics' bound (the cancellation in sumsq - n mean^2 is carried in double)."""
    nb = 3
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((nb, n)) * _bscale(nb, (1,)) + 0.5).astype(np.float32)
    x64 = x.astype(np.float64)
    bx = kt.Buf(x, "f32", 4096)
    bs = kt.Buf(np.zeros(2 * nb), "f64", 64, output=True)
    assert kt.lib.kt_stats(bx.ptr, nb, n, bs.ptr, None) == 0
    bmi = kt.Buf(np.zeros(2 * nb), "f32", 64, output=True)
    bms = kt.Buf(np.zeros(2 * nb), "f32", 64, output=True)
    assert kt.lib.kt_input_norm_params(bs.ptr, nb, n, bmi.ptr, bms.ptr, None) == 0
    kt.sync()
    st, bands = bs.host()
    assert bands
    ref = np.stack([x64.sum(1), (x64 * x64).sum(1)], -1)
    tol = n * 2.0 ** -53 * np.stack([np.abs(x64).sum(1), (x64 * x64).sum(1)], -1)
    worst = {"stats": _ratio(st.reshape(nb, 2), ref, tol)}
    mean = x64.mean(1)
    std = np.sqrt(((x64 - mean[:, None]) ** 2).sum(1) / (n - 1))
    mi, b1 = bmi.host()
    ms, b2 = bms.host()
    assert b1 and b2
    mi, ms = mi.reshape(nb, 2).astype(np.float64), ms.reshape(nb, 2).astype(np.float64)
    rel = 4 * kr.E32 + 1e-9
    worst["mean"] = _ratio(mi[:, 0], mean, rel * np.abs(mean))
    worst["div"] = _ratio(mi[:, 1], 1e-5 + std, rel * (1e-5 + std))
    worst["mean2"] = _ratio(ms[:, 0], mean, rel * np.abs(mean))
    worst["std"] = _ratio(ms[:, 1], std, rel * std)
    print("stats n=%d: %s" % (n, worst))
    kt.record("stats[%d]" % n, err_over_tol=worst)
    assert max(worst.values()) <= 1.0, worst


# =====================================================================================================  convt4
CT_UNIT = [(1, 32, 1), (3, 40, 1), (5, 33, 1), (2, 11, 3), (4, 6, 6), (2, 7, 5)]
CT_WALK = [(nb, H, W) for H in (14, 15, 29) for W in (32, 33, 47, 65) for nb in (1, 3)]


@pytest.fixture(scope="module")
def ct_weights():
    rng = np.random.default_rng(4)
    wt = kr.bf16_round(rng.standard_normal((96, 48, 8)) / np.sqrt(192.0))
    bias = np.asarray(0.5 * rng.standard_normal(48), dtype=np.float32).astype(np.float64)
    return wt, kr.convt_pack(wt), bias


def _ct_run(kt, x, wp, bias, keep, st0):
    import ctypes
    nb, H, W, _ = x.shape
    rows_out = (2 if keep else 4) * H
    bx = kt.Buf(kr.bf16_bits(x.astype(np.float32)), "bf16", 64 * 96 * max(W, 1))
    bw = kt.Buf(kr.bf16_bits(wp.astype(np.float32)), "bf16", 192 * 32)
    bb = kt.Buf(bias, "f32", 256)
    init = np.full(nb * rows_out * W * 48, kt.BF16_SENTINEL_BITS, dtype=np.uint16)
    bo = kt.Buf(init, "bf16", 64 * 48 * 4 * max(W, 1), output=True)
    bs = kt.Buf(st0, "f64", 64, output=True)
    d = kt.fill(kt.KtConvT4, x=bx.ptr, w=bw.ptr, bias=bb.ptr, out=bo.ptr, stats=bs.ptr, nb=nb, H=H, W=W, keep=keep)
    rc = kt.lib.kt_convt4(ctypes.byref(d), None)
    kt.sync()
    out, b1 = bo.host()
    st, b2 = bs.host()
    assert b1 and b2, "guard band overwritten"
    return rc, out, init, st.reshape(nb, 2)


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("nb,H,W", CT_UNIT + CT_WALK)
def test_convt4(kt, ct_weights, nb, H, W, keep):
    """convt4_launch (unit kernel W < 32, walk kernel W >= 32) against conv_transpose2d (8,1) / (4,1) / (2,0):
    tol = (192 + 16) e S + half a bf16 ulp; keep = 1 stores residues 1, 2 as rows 2u, 2u + 1 while the fp64 statistics,
    accumulated onto a nonzero start value, cover all four residues (sum rule of kernel_refs.stats_of)."""
    wt, wp, bias = ct_weights
    rng = np.random.default_rng(100 * H + W + nb)
    x = kr.bf16_round(rng.standard_normal((nb, H, W, 96)) * _bscale(nb, (1, 1, 1)))
    R, tol, S, tol_acc = kr.convt_ref(x, wp, bias)
    st0 = np.stack([1.5 * (np.arange(nb) + 1), -2.0 * (np.arange(nb) + 1)], -1)
    rc, out, init, st = _ct_run(kt, x, wp, bias, keep, st0)
    assert rc == 0, rc
    got = _vals(out, True).reshape(nb, (2 if keep else 4) * H, W, 48)
    if keep:
        sel = np.sort(np.concatenate([np.arange(1, 4 * H, 4), np.arange(2, 4 * H, 4)]))
        Rk, tk = R[:, sel], tol[:, sel]
    else:
        Rk, tk = R, tol
    worst = {"out": _ratio(got, Rk, tk), "rows 0, H-1": _ratio(got[:, [0, 1, -2, -1]], Rk[:, [0, 1, -2, -1]], tk[:, [0, 1, -2, -1]])}
    sref, stol = kr.stats_of(R, tol_acc)          # (statistics of the values before the bf16 rounding)
    worst["stats"] = _ratio(st - st0, sref, stol)
    print("convt4 nb=%d H=%d W=%d keep=%d: %s" % (nb, H, W, keep, worst))
    kt.record("convt4[%d,%d,%d,keep=%d]" % (nb, H, W, keep), err_over_tol=worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("nb,H,W", [(1, 31, 1), (2, 5, 6), (3, 1, 1)])
def test_convt4_refuses_short_items(kt, ct_weights, nb, H, W):
    """H W < 32 (a 32-row unit would cover more than two items): -1 and nothing written"""
    wt, wp, bias = ct_weights
    x = np.ones((nb, H, W, 96))
    st0 = np.ones((nb, 2))
    rc, out, init, st = _ct_run(kt, x, wp, bias, 0, st0)
    assert rc == -1
    assert np.array_equal(out, init) and np.array_equal(st, st0)
