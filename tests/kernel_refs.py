"""float64 references and derived tolerances for the kernel-level parity tests (tests/test_gpu_kernels.py).

Every reference is written from the operation's formula (csrc/gemm.h's header comment, csrc/attn.h, csrc/kernels.h),
not from a kernel.  Beside every result R it returns tol, an error bound derived from the number formats:

    e = 2^-24  (f32 round to nearest, relative)        u = 2^-9  (bf16, as the attention bound uses it)

* GEMM / ConvT: the operands are exactly representable in the compute type, so every product is exact in f32 and only
  the accumulation rounds: |acc - R| <= (K + 16) e S, with S the same formula on absolute values (bias included).
  An epilogue step f propagates the bound through its Lipschitz constant and adds its own f32 roundings (4e of the
  magnitudes involved per step).
* A bf16 output adds half a bf16 ulp of the stored value, hulp(R) = 2^(floor(log2 |R|) - 8): round to nearest keeps 8
  significant bits.  That is u |R| only at the top of a binade and 2u |R| at its bottom (R = 0.7168 rounds 1.9e-3
  away, u |R| = 1.4e-3), so a flat u |R| is exceeded by a correctly rounding kernel; hulp is the exact term.  It is
  taken at |R| + tol, the largest magnitude the value before rounding can have.
* f32 A converted on load (gemm2, bf16 mode): the reference rounds A to bf16 first.  Where a normalisation (a_norm,
  a_gn_*) runs before that conversion the kernel's f32 value and the reference's f64 value can round to different
  neighbours, but only when the value lies within 8e |a| of a rounding tie; for exactly those elements the bound
  gains one bf16 ulp of the element times |W| (term `amb`).
* Row LayerNorm of values v_i known to d_i:  y_i = (v_i - m) r w_i + b_i.  |dm| <= mean(d); dr / r <= r rms(d)
  (Cauchy-Schwarz on d(var) = 2 mean((v - m) dv), with r sigma <= 1), so
  |dy_i| <= |w_i| r (d_i + mean(d) + |v_i - m| r rms(d)) + the LayerNorm kernel's own bound (layernorm_ref).
* Statistics {sum, sumsq} of values R_i known to tol_i:  |dsum| <= sum tol_i, |dsumsq| <= sum (2 |R_i| tol_i + tol_i^2);
  the f32 partial sums of at most a tile of rows add n_part e sum|R_i| (n_part <= 64 additions per lane).
"""
import math
from types import SimpleNamespace

import numpy as np

E32 = 2.0 ** -24
U16 = 2.0 ** -9
GELU_FAST_ABS = 4.8e-4      # csrc/common.h: |gelu_fast - gelu_erf|
ACT_NONE, ACT_GELU, ACT_GLU = 0, 1, 2

try:
    from scipy.special import erf as _erf     # (optional; math.erf otherwise)
except Exception:  # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])


# ------------------------------------------------------------------------------------------------ bf16
def bf16_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (finite values and infinities)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b >> 16) & 1) + 0x7FFF
    return ((b + r) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    """values rounded to bf16, returned as float64"""
    return bf16_value(bf16_bits(np.asarray(x, dtype=np.float32))).astype(np.float64)


def bf16_round_amb(a64):
    """bf16(a) for f64 values that a kernel computed in f32 before converting: (rounded, amb) with amb = one bf16 ulp
    where a lies within 8e |a| of a rounding tie (the kernel may have rounded the other way), else 0."""
    a64 = np.asarray(a64, dtype=np.float64)
    r = bf16_round(a64)
    mant, expo = np.frexp(np.where(a64 == 0, 1.0, a64))
    ulp = np.ldexp(1.0, expo - 8)                      # bf16: 8 significant bits
    frac = np.abs(a64 - r) / ulp                       # 0 .. 0.5
    amb = np.where((0.5 - frac) * ulp <= 8 * E32 * np.abs(a64), ulp, 0.0)
    return r, np.where(a64 == 0, 0.0, amb)


def hulp16(x):
    """half a bf16 ulp at magnitude x: 2^(floor(log2 |x|) - 8), 0 at 0"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(np.where(x == 0, 1.0, x))          # x = m 2^e, 0.5 <= m < 1
    return np.where(x == 0, 0.0, np.ldexp(1.0, e - 1 - 8))


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gn_params(stats, count):
    """GroupNorm(1) (mean, rstd) per batch from {sum, sumsq} (eps 1e-5)"""
    st = np.asarray(stats, dtype=np.float64).reshape(-1, 2)
    mean = st[:, 0] / count
    var = np.maximum(st[:, 1] / count - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + 1e-5)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_ref(v, w, b, pos=None, out_bf16=False, d_in=None):
    """LayerNorm over the last axis (eps 1e-5) + optional pos.  v [rows][C]; pos [rows][C] (already per row).
    tol = 16e (|v| + |mean|) rstd |w| + 4e (|y| + |b| + |pos|) (+ hulp(y) for a bf16 output); d_in: bound on v itself
    (propagated as in the module docstring)."""
    v = np.asarray(v, dtype=np.float64)
    m = v.mean(axis=-1, keepdims=True)
    var = ((v - m) ** 2).mean(axis=-1, keepdims=True)
    r = 1.0 / np.sqrt(var + 1e-5)
    y = (v - m) * r * w + b
    p = 0.0 if pos is None else pos
    y = y + p
    tol = 16 * E32 * (np.abs(v) + np.abs(m)) * r * np.abs(w) + 4 * E32 * (np.abs(y) + np.abs(b) + np.abs(p))
    if d_in is not None:
        d = np.asarray(d_in, dtype=np.float64)
        tol = tol + np.abs(w) * r * (d + d.mean(axis=-1, keepdims=True) +
                                     np.abs(v - m) * r * np.sqrt((d * d).mean(axis=-1, keepdims=True)))
    if out_bf16:
        tol = tol + hulp16(np.abs(y) + tol)
    return y, tol


# ------------------------------------------------------------------------------------------------ attention
def attn_ref(q, k, v, scale, mode):
    """softmax(scale q k^T) v per head.  q [nb][H][Nq][64], k / v [nb][H][Nk][64] (float64).
    mode 1 (bf16): tol = 4u (P |V|) + 2u |R|;  mode 0 (f32): tol = (Nk + 96) e (1 + max_j |s_ij|) (P |V|)."""
    s = scale * np.einsum("bhqd,bhkd->bhqk", q, k)
    smax = s.max(axis=-1, keepdims=True)
    p = np.exp(s - smax)
    p /= p.sum(axis=-1, keepdims=True)
    r = np.einsum("bhqk,bhkd->bhqd", p, v)
    pv = np.einsum("bhqk,bhkd->bhqd", p, np.abs(v))
    if mode == 1:
        tol = 4 * U16 * pv + 2 * U16 * np.abs(r)
    else:
        nk = k.shape[2]
        tol = (nk + 96) * E32 * (1.0 + np.abs(s).max(axis=-1, keepdims=True)) * pv
    return r, tol


def attn_emulate_bf16(q, k, v, scale, kt=64):
    """The bf16 kernels' arithmetic on the CPU: 64-key online softmax in f32, P rounded to bf16 once, f32
    accumulation, bf16 output.  (tests/test_kernel_refs.py holds it to attn_ref's bound.)"""
    f = np.float32
    nb, nh, nq, _ = q.shape
    nk = k.shape[2]
    q32, k32, v32 = q.astype(f), k.astype(f), v.astype(f)
    m = np.full((nb, nh, nq, 1), -np.inf, dtype=f)
    l = np.zeros((nb, nh, nq, 1), dtype=f)
    o = np.zeros((nb, nh, nq, 64), dtype=f)
    for k0 in range(0, nk, kt):
        s = (np.einsum("bhqd,bhkd->bhqk", q32, k32[:, :, k0:k0 + kt]) * f(scale)).astype(f)
        mn = np.maximum(m, s.max(axis=-1, keepdims=True))
        alpha = np.exp(m - mn).astype(f)
        p = np.exp(s - mn).astype(f)
        l = (l * alpha + p.sum(axis=-1, keepdims=True, dtype=f)).astype(f)
        pb = bf16_round(p).astype(f)
        o = (o * alpha + np.einsum("bhqk,bhkd->bhqd", pb, v32[:, :, k0:k0 + kt])).astype(f)
        m = mn
    return bf16_round((o / l).astype(f))


# ------------------------------------------------------------------------------------------------ ConvTranspose
RES_OFF = (-1, -1, 0, 0)      # csrc/ctx.h: output row 4u + rho reads input rows u + RES_OFF[rho] and the next one
RES_K0 = (6, 7, 4, 5)         #             with kernel taps RES_K0[rho] and RES_K1[rho]
RES_K1 = (2, 3, 0, 1)


def convt_pack(wt):
    """ConvTranspose2d weight [Ci][Co][8] -> the four-residue rows of kernels.h: row rho*Co + co,
    K = [row u + RES_OFF[rho] | next row] x Ci"""
    ci, co, _ = wt.shape
    w = np.zeros((4 * co, 2 * ci), dtype=np.float64)
    for rho in range(4):
        w[rho * co:(rho + 1) * co, :ci] = wt[:, :, RES_K0[rho]].T
        w[rho * co:(rho + 1) * co, ci:] = wt[:, :, RES_K1[rho]].T
    return w


def convt_ref_direct(x, wt, bias):
    """conv_transpose2d, kernel (8,1), stride (4,1), padding (2,0), from its definition:
    out[b][4i - 2 + k][w][co] += x[b][i][w][ci] wt[ci][co][k].  x [nb][H][W][Ci] -> (R, S) [nb][4H][W][Co]"""
    nb, H, W, ci = x.shape
    co = wt.shape[1]
    R = np.zeros((nb, 4 * H, W, co))
    S = np.zeros_like(R)
    for i in range(H):
        for kk in range(8):
            o = 4 * i - 2 + kk
            if 0 <= o < 4 * H:
                R[:, o] += x[:, i] @ wt[:, :, kk]
                S[:, o] += np.abs(x[:, i]) @ np.abs(wt[:, :, kk])
    return R + bias, S + np.abs(bias)


def convt_ref(x, wp, bias, res_off=RES_OFF):
    """The same ConvTranspose from packed four-residue weights wp [4 Co][2 Ci] (convt_pack).  Returns
    (R, tol, S, tol_acc): tol_acc = (K + 16) e S with K = 2 Ci bounds the f32 value, tol = tol_acc + hulp(R) the bf16
    output."""
    nb, H, W, ci = x.shape
    co = wp.shape[0] // 4
    xp = np.zeros((nb, H + 2, W, ci))
    xp[:, 1:H + 1] = x
    R = np.zeros((nb, 4 * H, W, co))
    S = np.zeros_like(R)
    for rho in range(4):
        lo = xp[:, 1 + res_off[rho]:1 + res_off[rho] + H]
        hi = xp[:, 2 + res_off[rho]:2 + res_off[rho] + H]
        a = np.concatenate([lo, hi], axis=-1)
        w = wp[rho * co:(rho + 1) * co]
        R[:, rho::4] = a @ w.T + bias
        S[:, rho::4] = np.abs(a) @ np.abs(w).T + np.abs(bias)
    tol_acc = (2 * ci + 16) * E32 * S
    return R, tol_acc + hulp16(np.abs(R) + tol_acc), S, tol_acc


def stats_of(R, tol, n_part=64):
    """{sum, sumsq} of R (any shape, reduced over all axes but the first) and their bounds (module docstring)"""
    ax = tuple(range(1, R.ndim))
    a = np.abs(R)
    s1, s2 = R.sum(axis=ax), (R * R).sum(axis=ax)
    t1 = tol.sum(axis=ax) + n_part * E32 * a.sum(axis=ax)
    t2 = (2 * a * tol + tol * tol).sum(axis=ax) + (n_part + 2) * E32 * (R * R).sum(axis=ax)
    return np.stack([s1, s2], axis=-1), np.stack([t1, t2], axis=-1)


# ------------------------------------------------------------------------------------------------ GEMM
def gemm_spec(**kw):
    """A GemmDesc with host arrays (numpy, float64 values as the device holds them) in place of pointers; defaults as
    csrc/gemm.h"""
    d = dict(A=None, a_bf16=0, nb=1, H_in=1, W=1, C_in=0, a_ld=0, a_cs=1, a_bs=-1, a_hs=-1, ntaps=1, in_stride=1,
             in_off=0, dil=1, H_out=1, a_norm=None, a_gn_stats=None, a_gn_count=0, a_gn_w=None, a_gn_b=None,
             Wp=None, N=0, K=0, Kp=0, bias=None, c_bf16=0, H_out_total=1, o_stride=1, o_off=0, ldo=0, col_off=0,
             c_bs=-1, store=1, c4=False, col_split=0, hi_row_off=1, store_mask=3, k_blk=0, act=ACT_NONE, res=None,
             res_bf16=0, res_scale=None, res_gn_stats=None, res_gn_count=0, res_gn_w=None, res_gn_b=None,
             row_add=None, stats=None, gn_stats=None, gn_count=0, gn_w=None, gn_b=None, pbias=None, pfold=1,
             res_div=1, res_bs=0, ln_w=None, ln_b=None, ln_out=False, sk=False, c_elems=0)
    for k in kw:
        if k not in d:
            raise KeyError(k)
    d.update(kw)
    return SimpleNamespace(**d)


def gemm_gather(g, tap_shift=0, pad_neighbour=False):
    """A as the [M][ntaps * C_in] matrix of the implicit GEMM: row (b, ho, w), column tap * C_in + ci reads
    A[b][ho * in_stride + in_off + tap * dil][w][ci], zero outside [0, H_in).  Returns (a, inb) with inb the in-bounds
    mask.  (tap_shift / pad_neighbour: the deliberate mutations of tests/test_kernel_refs.py.)"""
    a_bs = g.a_bs if g.a_bs >= 0 else g.H_in * g.W * g.a_ld
    a_hs = g.a_hs if g.a_hs >= 0 else g.W * g.a_ld
    b = np.arange(g.nb).reshape(-1, 1, 1, 1, 1)
    ho = np.arange(g.H_out).reshape(1, -1, 1, 1, 1)
    w = np.arange(g.W).reshape(1, 1, -1, 1, 1)
    t = np.arange(g.ntaps).reshape(1, 1, 1, -1, 1)
    ci = np.arange(g.C_in).reshape(1, 1, 1, 1, -1)
    h = ho * g.in_stride + g.in_off + t * g.dil + np.where(t == g.ntaps - 1, tap_shift, 0)
    inb = (h >= 0) & (h < g.H_in)
    idx = b * a_bs + h * a_hs + w * g.a_ld + ci * g.a_cs
    flat = np.asarray(g.A, dtype=np.float64).ravel()
    if pad_neighbour:
        ok = (idx >= 0) & (idx < flat.size)
        a = np.where(ok, flat[np.clip(idx, 0, flat.size - 1)], 0.0)
        inb_full = np.broadcast_to(inb, idx.shape) | ok
    else:
        inb_full = np.broadcast_to(inb, idx.shape)
        a = np.where(inb_full, flat[np.clip(idx, 0, flat.size - 1)], 0.0)
    M = g.nb * g.H_out * g.W
    return a.reshape(M, g.ntaps * g.C_in), inb_full.reshape(M, g.ntaps * g.C_in)


def gemm_ref(g, mode, tap_shift=0, pad_neighbour=False, stats_shift=False):
    """out = epi(A (*) Wp^T) as csrc/gemm.h describes it.  Returns a namespace:
    idx, R, tol  - flat element index into C, value and bound of every stored element
    v, v_tol     - the final values [nb (x pfold)][H_out][W][Nout] before routing (rows kept in C for ln_out)
    stats, stats_tol - per-batch {sum, sumsq} increments (None without g.stats)
    c4_idx, c4_R, c4_tol; ln_R, ln_tol (the bf16 LayerNorm rows of ln_out, dense [M][N])"""
    M = g.nb * g.H_out * g.W
    K = g.ntaps * g.C_in
    assert K == g.K and g.Kp >= K
    a, inb = gemm_gather(g, tap_shift, pad_neighbour)
    bidx = np.repeat(np.arange(g.nb), g.H_out * g.W)
    amb = np.zeros_like(a)
    normed = False
    if g.a_norm is not None:
        nrm = np.asarray(g.a_norm, dtype=np.float64).reshape(-1, 2)
        a = np.where(inb, (a - nrm[bidx, 0:1]) / nrm[bidx, 1:2], 0.0)
        normed = True
    if g.a_gn_stats is not None:
        gm, gr = gn_params(g.a_gn_stats, g.a_gn_count)
        cw = np.tile(np.asarray(g.a_gn_w, dtype=np.float64), g.ntaps)
        cb = np.tile(np.asarray(g.a_gn_b, dtype=np.float64), g.ntaps)
        a = np.where(inb, (a - gm[bidx, None]) * gr[bidx, None] * cw + cb, 0.0)
        normed = True
    if mode == 1 and not g.a_bf16:        # f32 A converted on load
        if normed:
            a, amb = bf16_round_amb(a)
        else:
            a = bf16_round(a)
    W = np.asarray(g.Wp, dtype=np.float64)[:g.N, :K].copy()
    if g.k_blk:
        grp = np.arange(g.N) // g.col_split
        kk = np.arange(K)
        keep = np.where(grp[:, None] < 2, kk[None, :] < 2 * g.k_blk, (kk[None, :] >= g.k_blk) & (kk[None, :] < 3 * g.k_blk))
        W = W * keep
    bias = np.zeros(g.N) if g.bias is None else np.asarray(g.bias, dtype=np.float64)
    v = a @ W.T + bias
    S = np.abs(a) @ np.abs(W).T + np.abs(bias)
    tol = (K + 16) * E32 * S + amb @ np.abs(W).T
    if normed and not (mode == 1 and not g.a_bf16):
        tol = tol + 8 * E32 * S          # f32 mode: the normalisation's own roundings on every A element
    pf = g.pfold if (g.pbias is not None and g.pfold > 1) else 1
    # output batches: bo = b * pfold + p
    v = np.repeat(v.reshape(g.nb, 1, g.H_out * g.W, g.N), pf, axis=1).reshape(g.nb * pf, g.H_out * g.W, g.N)
    tol = np.repeat(tol.reshape(g.nb, 1, g.H_out * g.W, g.N), pf, axis=1).reshape(v.shape)
    nbo = g.nb * pf
    if g.pbias is not None:
        pb = np.asarray(g.pbias, dtype=np.float64).reshape(nbo, 1, g.N)
        v = v + pb
        tol = tol + 2 * E32 * (np.abs(v) + np.abs(pb))
    if g.gn_stats is not None:
        gm, gr = gn_params(g.gn_stats, g.gn_count)
        gw, gb = np.asarray(g.gn_w, dtype=np.float64), np.asarray(g.gn_b, dtype=np.float64)
        c = (v - gm[:, None, None]) * gr[:, None, None] * gw
        tol = tol * gr[:, None, None] * np.abs(gw) + 4 * E32 * (np.abs(c) + np.abs(gb) +
                                                                np.abs(gm[:, None, None]) * gr[:, None, None] * np.abs(gw))
        v = c + gb
    fast = mode == 1
    if g.act == ACT_GELU:
        tol = 1.13 * tol + 8 * E32 * np.abs(v) + (GELU_FAST_ABS if fast else 0.0)
        v = gelu(v)
    elif g.act == ACT_GLU:
        vv = v.reshape(nbo, -1, g.N // 32, 2, 16)
        tt = tol.reshape(vv.shape)
        aa, gg = vv[:, :, :, 0], vv[:, :, :, 1]
        v = (aa * sigmoid(gg)).reshape(nbo, -1, g.N // 2)
        tol = (tt[:, :, :, 0] + np.abs(aa) * tt[:, :, :, 1] / 4).reshape(v.shape) + 8 * E32 * np.abs(v)
    Nout = v.shape[-1]
    ho_of = np.repeat(np.arange(g.H_out), g.W)
    if g.row_add is not None:
        ra = np.asarray(g.row_add, dtype=np.float64).reshape(-1, Nout)[ho_of]
        v = v + ra
        tol = tol + 2 * E32 * (np.abs(v) + np.abs(ra))
    c_bs = g.c_bs if g.c_bs >= 0 else g.H_out_total * g.W * g.ldo
    # position of (bo, ho, w) in C before column routing
    w_of = np.tile(np.arange(g.W), g.H_out)
    inb_off = ((ho_of * g.o_stride + g.o_off) * g.W + w_of) * g.ldo + g.col_off          # [H_out*W]
    if g.res is not None:
        rs = np.ones(Nout) if g.res_scale is None else np.asarray(g.res_scale, dtype=np.float64)
        rflat = np.asarray(g.res, dtype=np.float64).ravel()
        bo = np.arange(nbo)
        rbase = np.where(g.pbias is not None and g.res_div > 1, (bo // max(g.res_div, 1)) * g.res_bs, bo * c_bs)
        ridx = rbase[:, None, None] + inb_off[None, :, None] + np.arange(Nout)[None, None, :]
        rr = rflat[ridx]
        rt = 0.0
        if g.res_gn_stats is not None:
            gm, gr = gn_params(g.res_gn_stats, g.res_gn_count)
            gw, gb = np.asarray(g.res_gn_w, dtype=np.float64), np.asarray(g.res_gn_b, dtype=np.float64)
            c = (rr - gm[:, None, None]) * gr[:, None, None] * gw
            rt = 8 * E32 * (np.abs(c) + np.abs(gb) + np.abs(gm[:, None, None]) * gr[:, None, None] * np.abs(gw))
            rr = c + gb
        tol = np.abs(rs) * tol + rt + 2 * E32 * (np.abs(rr) + np.abs(rs * v))
        v = rr + rs * v
    out = SimpleNamespace(v=v.reshape(nbo, g.H_out, g.W, Nout), v_tol=tol.reshape(nbo, g.H_out, g.W, Nout),
                          stats=None, stats_tol=None, ln_R=None, ln_tol=None, c4_idx=None, c4_R=None, c4_tol=None,
                          idx=None, R=None, tol=None)
    if g.stats is not None:
        st, stt = stats_of(v, tol)
        if stats_shift:      # mutation: the first row of every batch but the first is credited to the batch before
            for bq in range(1, nbo):
                row = v[bq, 0]
                st[bq] -= [row.sum(), (row * row).sum()]
                st[bq - 1] += [row.sum(), (row * row).sum()]
        out.stats, out.stats_tol = st, stt
    store_R, store_tol = v, tol
    if g.ln_w is not None:
        lw, lb = np.asarray(g.ln_w, dtype=np.float64), np.asarray(g.ln_b, dtype=np.float64)
        y, yt = layernorm_ref(v, lw, lb, out_bf16=False, d_in=tol)
        if g.ln_out:
            out.ln_R, out.ln_tol = y.reshape(-1, Nout), (yt + hulp16(np.abs(y) + yt)).reshape(-1, Nout)
        else:
            store_R, store_tol = y, yt          # (the bf16 term is added below with c_bf16)
    if g.store:
        n = np.arange(Nout)
        if g.col_split:
            grp = n // g.col_split
            col = n - grp * g.col_split
            rowoff = grp * g.hi_row_off * g.W * g.ldo
            keep = ((g.store_mask >> grp) & 1).astype(bool)
        else:
            col, rowoff, keep = n, np.zeros(Nout, dtype=np.int64), np.ones(Nout, dtype=bool)
        idx = (np.arange(nbo) * c_bs)[:, None, None] + inb_off[None, :, None] + (rowoff + col)[None, None, :]
        t = store_tol + (hulp16(np.abs(store_R) + store_tol) if g.c_bf16 else 0.0)
        out.idx, out.R, out.tol = idx[:, :, keep].ravel(), store_R[:, :, keep].ravel(), t[:, :, keep].ravel()
        if g.c4:
            rows = (np.arange(nbo) * c_bs)[:, None] + inb_off[None, :] - g.col_off
            out.c4_idx = ((rows // g.ldo)[:, :, None] * 4 + np.arange(4)).ravel()
            out.c4_R, out.c4_tol = store_R[:, :, :4].ravel(), t[:, :, :4].ravel()
    return out
