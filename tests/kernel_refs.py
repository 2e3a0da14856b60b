"""float64 references and derived tolerances for the kernel-level parity tests (tests/test_gpu_kernels.py,
tests/test_gpu_dconv.py, tests/test_gpu_dec.py).

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

The DConv kernels (tests/test_gpu_dconv.py; formulas: csrc/kernels.h, the header comments of csrc/dconv.hip and
SURVEY.md Appendix A: conv3 -> GroupNorm(1) -> GELU -> 1x1 -> GroupNorm(1) -> GLU -> LayerScale -> residual) add:

* GLU step a sigma(g) of a, g known to da, dg:  d(a sigma) = sigma da + a sigma' dg with sigma' = sigma (1 - sigma)
  <= 1/4, so |d| <= |da| sigma(g) + |a| (|dg| / 4 + 4e); the 4e covers the f32 exp, add, divide and product.  The
  bf16 mode's sigmoid_fast is rcp(1 + exp2(-g log2 e)) on v_exp_f32 and v_rcp_f32 (about 1 ulp = 2e each, common.h):
  the argument's rounding moves t = exp(-g) by |g| e relative and v_exp by 2e more, d sigma = sigma (1 - sigma) dt / t;
  the add rounds once (e) and v_rcp adds 2e relative to sigma.  Together |d sigma| <= sigma ((1 - sigma)(|g| + 4) + 4) e,
  which multiplies |a| (term `fast`).
* GroupNorm from statistics known to a bound (dm on the mean, drr = dr / r on rstd), values known to d:
  z = (v - m) r w + b,  |dz| <= |w| r (d + dm + |v - m| drr) + 4e (|c| + |b| + |m| r |w|) with c = (v - m) r w: the
  LayerNorm rule above with the statistics' own bound as input instead of mean(d), rms(d).  Statistics a kernel reads
  from memory (fp64 {sum, sumsq} written by an earlier pass) are exact inputs: dm = drr = 0.
* Moment-form statistics of y = W x + b over its N outputs (pack.h conv1x1_moments: G = W^T W, v = W^T b, ws = W^T 1):
  sum_n y = sum b + ws.x,  sum_n y^2 = sum b^2 + 2 v.x + x^T G x.  The reference evaluates y itself in f64 from the
  row x the kernel stored (bf16, checked separately: no rounding-tie ambiguity).  The kernel evaluates the form in f32:
  H^2 + H products and as many additions for the quadratic term, 2H for each linear term, 4 to combine, every one
  bounded by e times the form on absolute values A = (|sum b| + |ws|.|x|,  sum b^2 + 2 |v|.|x| + |x|^T |G| |x|), so
  (H^2 + 3H + 4) e A; the moments themselves are f32 roundings of f64 sums, e relative per entry: + e A.  Per-position
  values are added in fp64 over n positions: + n 2^-53 sum A (the term stats_of takes as n64).  Where x is only known
  to d (dconv_small: x = GELU(GN(stored h))) the form's derivative adds |ws|.d and 2 |v|.d + 2 (|G| |x|).d + d^T |G| d.
* bf16 rounding of a value known only to d (the updated row before the fused rewrite): bf16_round_amb(a, d) marks an
  element within d' = 8e |a| + d of a rounding tie; it gets one bf16 ulp, times |W| of the GEMM that reads it.  One
  ulp holds only while d' <= ulp / 2, and below a power of two the spacing halves, so the function takes the bound
  from monotonicity instead: the kernel's bf16 lies between bf16(a - d') and bf16(a + d').
* fenc_row (a whole encoder level per (b, f) row, end to end): both GroupNorm statistics of a layer are one-pass f32
  sums over the row's n values v (gn_from_sums): s1 = sum v, s2 = sum v^2, m = s1 / n, var = s2 / n - m^2.  With the
  values known to t:  |ds1| <= sum t + n_part e sum |v|,  |ds2| <= sum (2 |v| t + t^2) + (n_part + 2) e sum v^2, so
  dm = |ds1| / n + e |m| and dvar = |ds2| / n + 2 |m| dm + dm^2 + 3e (s2 / n + m^2): the variance bound carries
  n_part e sum v^2 / n however small var is, which is what a large mean-to-deviation ratio amplifies.  drr is the
  larger relative change of (var + eps)^-1/2 over var +- dvar (var - dvar clamped at 0) + 4e for the add, sqrtf and
  divide.  n_part is the depth of the documented reduction: level 0 - 12 additions per lane (3 m-tiles x 4
  channels), 4 DPP row steps, 2 readlane levels, 3 levels over the 8 waves = 21; level 1 - 8 per lane (2 m-tiles),
  6 wave_sum steps, 12 sequential wave partials = 26.  The 1x1 statistics are the moment form per position added in
  f32 the same way (level 0: 1 + 4 + 2 + 3 = 10, level 1: 2 + 6 + 12 = 20 additions of partial forms, each bounded
  by the form on absolute values).  The 1x1 apply uses the folded affine y' wa + ca with wa = r w s, ca = ((b1 - m)
  r w + beta) s (s the LayerScale; the gate half carries -log2 e instead): y' and b1 - m no longer cancel before the
  roundings, so 6e (|y'| + |b1 - m|) r |w| + 4e |beta| is added.  The residual stream x stays in f32 (bound d,
  accumulated over the stages); its bf16 image and the bf16 hidden tile follow bf16_round_amb(., d).
  The reference's GELU here is the tanh form v sigmoid(u), u = sqrt(8 / pi) (v + 0.044715 v^3), the function the bf16
  mode documents (common.h gelu_fast), not the erf form + GELU_FAST_ABS: carried as an unknown error, 4.8e-4 puts 70 %
  of the first bf16 image within the bound of a rounding tie and the end-to-end bound reaches 7e2 at the output.
  gelu_fast evaluates x rcp(1 + exp2(x fma(K1, x^2, K0))): five roundings in the argument (e |u| each on exp), v_exp
  and v_rcp about 2e each, the add and the product e each, and |gelu_tanh'| <= 1.13:
  |d| <= 1.13 t + |v| sigma ((1 - sigma)(5 |u| + 2) + 4) e.
  Even so the bound is worst case over every tie and every sum |w|: it grows by about 2 (tie) x 11 (sum |w| of conv3)
  x 2.4 (1x1) x 1.3 per DConv layer.  Level 0 ends with a median bound of 0.4 .. 1.0 on outputs that carry row scales
  of 1 .. 16, where a float32 evaluation (bf16 flips included) uses 0.01 .. 0.6 of it: it separates wrong taps, rows,
  embeddings and channels, not a statistics count off by 5 %.  Level 1 (conv K = 384: a bound of 1.8e-4 on the first
  image, 44 % of it within that of a tie, every element after the first layer) ends at 1e3: the comparison there only
  shows finite values of the right order.  tests/test_dconv_refs.py holds the measured figures and asserts them.
* Short GroupNorm rows (L = 1, 2 in dconv_small) have a tiny variance, so rstd is large (up to 316) and every bound
  above that carries r grows with it.  That is the arithmetic's own conditioning, not slack.

The decoder kernels (tests/test_gpu_dec.py; formulas: csrc/kernels.h, the header comments of csrc/fdec_lr.hip and
csrc/dec_last.hip, ATHTDemucs_v2.py:76-139 as cited there) add:

* The resize index rule (common.h lin_index) is evaluated in float32 exactly as the device does, the multiply-add of
  the source index fused (lin_index_ref), so the references use the kernels' own lerp weights bit for bit and no bound
  carries a weight error.  A lerp l0 a + l1 b adds 3e (l0 |a| + l1 |b|) (two products, one sum) to the resized input
  bounds (resize_h_ref); an identity resize adds nothing.
* The decoder merge (dec_merge_ref): GroupNorm from the exact fp64 {sum, sumsq} the kernel reads (dm = drr = 0; the
  float32 roundings of mean and rstd are part of the 4e terms), gelu_step or gelu_tanh_step, the resize, the skip
  0.1 resize(skip) (2e for the float32 0.1 and the product), 2e for the sum; the 1x1 projection: |P| tol + (C + 4) e
  |P| |v|; hulp16 at |R| + tol for a bf16 store.  Where a kernel folds the affine into x (r w) + (b - m r w) (the bf16
  forms of dec_merge_w1, fdec_tail, tdec_tail, fdec_lr_merge3), x and m no longer cancel before the roundings:
  + 6e (|x| + |m|) r |w| + 4e |b|.  Two GELUs sharing one reciprocal (gelu_fast_wsum_pk): + 8e of each weighted term.
  tdec_tail keeps the activated rows as bf16 in LDS: the reference rounds them too and bf16_round_amb gives the bound
  (the rounded value feeds the resize and the folded projection).
* The folded last level (dec_last_ref) is computed from the unfolded weights; the kernels get the product's fold.
  tol = (K + 32) e A, A the same chain on absolute values, K = 3 x 48 (freq) or 4 x 48 (time) accumulated products;
  the 32 covers the fold's own float32 rounding (e |P| |W|), the skip products and the last sums.  A bound on the
  input (the fused level-2 merge) goes through |W|, the resize and |P|.
* The low-rank level 1 (fdec_lr_ref) is staged: Z, Zs are the stored roundings of float64 products and stand for S and
  skip3 (resize and ConvTranspose commute with the per-tap 1x1); D0 is materialised and the plain ConvTranspose scatter
  runs on it, the re-association does not appear.  Per D0 value: the two resize bounds + 2e; per ConvT row: the sum of
  its D0 bounds + 3e (|terms| + |bias|).  The v3 passes update the lerp base incrementally (base += dr at every row
  change): one float32 rounding of the base per change, e (|Z[i0]| + 0.1 |Zs[k0]| + |bias|), accumulated over the
  changes counted from the step table up to the row's step.  {sum, sumsq}: the statistics rule with n_part = 68 (16
  steps x 4 rows per float32 partial sum) and the fp64 additions above it.
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


def bf16_round_amb(a64, d=0.0):
    """bf16(a) for f64 values that a kernel computed in f32 before converting: (rounded, amb).  The kernel's value lies
    within d' = 8e |a| + d of a (d: absolute bound on it before the conversion, scalar or array) and rounding is
    monotone, so its bf16 lies between bf16(a - d') and bf16(a + d'): amb is the larger distance of the two from
    bf16(a).  That is 0 unless a rounding tie lies within d' of a, and then one bf16 ulp (the kernel may have rounded
    the other way) as long as d' is below half an ulp."""
    a64 = np.asarray(a64, dtype=np.float64)
    r = bf16_round(a64)
    dd = 8 * E32 * np.abs(a64) + d
    return r, np.maximum(r - bf16_round(a64 - dd), bf16_round(a64 + dd) - r)


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
RES_OFF = (-1, -1, 0, 0)      # csrc/pack.h: output row 4u + rho reads input rows u + RES_OFF[rho] and the next one
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


def stats_of(R, tol, n_part=64, n64=0):
    """{sum, sumsq} of R (any shape, reduced over all axes but the first) and their bounds (module docstring); n64:
    the number of fp64 additions behind one sum (2^-53 relative each)"""
    ax = tuple(range(1, R.ndim))
    a = np.abs(R)
    s1, s2 = R.sum(axis=ax), (R * R).sum(axis=ax)
    t1 = tol.sum(axis=ax) + (n_part * E32 + n64 * 2.0 ** -53) * a.sum(axis=ax)
    t2 = (2 * a * tol + tol * tol).sum(axis=ax) + ((n_part + 2) * E32 + n64 * 2.0 ** -53) * (R * R).sum(axis=ax)
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


# ------------------------------------------------------------------------------------------------ DConv packers
def glu_src(pr, n):
    """pack.h: packed row pr of a GLU-interleaved [n = 2C] layer reads natural row glu_src: per 32 packed rows
    [a(16q .. 16q+15) | gate(C + 16q .. C + 16q + 15)]"""
    C, q, s = n // 2, pr // 32, pr % 32
    return 16 * q + s if s < 16 else C + 16 * q + (s - 16)


def glu_order(v):
    """a [2C] (or [2C][...]) array in packed GLU order"""
    v = np.asarray(v)
    return v[[glu_src(i, v.shape[0]) for i in range(v.shape[0])]]


def rewrite_perm(k):
    """K slot k of the fused rewrite's weights holds channel rewrite_perm(k) (kernels.h DcRewrite, pack.h
    dconv_rewrite_perm): slot 32 ks + 8 g + i <- channel 32 ks + 4 g + i (i < 4) or 32 ks + 16 + 4 g + (i - 4)"""
    ks, g, i = k // 32, (k % 32) // 8, k % 8
    return 32 * ks + (4 * g + i if i < 4 else 16 + 4 * g + (i - 4))


def conv3_pack(w3, rows=None):
    """Conv1d weight [H][C][3] -> [rows][tap * C + c] (rows >= H, the extra ones zero: the MFMA tile of 16)"""
    H, C, _ = w3.shape
    out = np.zeros((rows or H, 3 * C), dtype=np.float64)
    out[:H] = np.transpose(w3, (0, 2, 1)).reshape(H, 3 * C)
    return out


def conv1x1_pack(w1, kp=64):
    """1x1 weight [2C][H] -> GLU-interleaved rows, K zero-padded to kp"""
    out = np.zeros((w1.shape[0], kp), dtype=np.float64)
    out[:, :w1.shape[1]] = glu_order(w1)
    return out


def rewrite_pack(wr):
    """rewrite weight [2C][C] -> GLU-interleaved rows in the K order of rewrite_perm, K = roundup(C, 32)"""
    n, C = wr.shape
    K2 = (C + 31) // 32 * 32
    src = glu_order(wr)
    out = np.zeros((n, K2), dtype=np.float64)
    for k in range(K2):
        ch = rewrite_perm(k)
        if ch < C:
            out[:, k] = src[:, ch]
    return out


def conv1x1_moments(w, b, round_bf16):
    """[G = W^T W (H x H) | v = W^T b | ws = W^T 1 | sum b | sum b^2] of W [N][H], b [N] as float32, accumulated in
    float64 row by row (pack.h conv1x1_moments); round_bf16: from the bf16-rounded weights"""
    w = np.asarray(w, dtype=np.float32)
    w = bf16_round(w) if round_bf16 else w.astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    N, H = w.shape
    G, v, ws, sb, sb2 = np.zeros((H, H)), np.zeros(H), np.zeros(H), 0.0, 0.0
    for n in range(N):
        G += np.outer(w[n], w[n])
        v += b[n] * w[n]
        ws += w[n]
        sb += b[n]
        sb2 += b[n] * b[n]
    return np.concatenate([G.ravel(), v, ws, [sb, sb2]]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ DConv references
def group_sums(v, L):
    """{sum, sumsq} per GroupNorm row of v [M][n] (rows of L positions, the last one possibly short)"""
    M = v.shape[0]
    gi = np.arange(M) // L
    ng = int(gi[-1]) + 1
    return np.stack([np.bincount(gi, v.sum(1), ng), np.bincount(gi, (v * v).sum(1), ng)], -1)


def dconv_conv3_ref(x, w3, bias, dil, mut=None):
    """h[b][t][j] = bias[j] + sum_{tap, c} w3[j][c][tap] x[b][t + (tap - 1) dil][c], zero outside [0, L).
    x [nb][L][C] (values exact in the compute type), w3 [H][C][3].  tol = (3C + 16) e S (GEMM rule), batch by batch
    (large cases).  mut: 'neighbour' (a tap past a row end reads the neighbouring row), 'reversed' (taps reversed)."""
    nb, L, C = x.shape
    H = w3.shape[0]
    R, S = np.empty((nb, L, H)), np.empty((nb, L, H))
    flat = x.reshape(nb * L, C)
    for b in range(nb):
        r = np.tile(np.asarray(bias, dtype=np.float64), (L, 1))
        s = np.abs(r)
        for tap in range(3):
            off = (tap - 1) * dil
            xs = np.zeros((L, C))
            if mut == "neighbour":
                p = b * L + np.arange(L) + off
                ok = (p >= 0) & (p < nb * L)
                xs[ok] = flat[p[ok]]
            else:
                t0, t1 = max(0, -off), min(L, L - off)
                if t1 > t0:
                    xs[t0:t1] = x[b, t0 + off:t1 + off]
            wt = w3[:, :, 2 - tap if mut == "reversed" else tap]
            r += xs @ wt.T
            s += np.abs(xs) @ np.abs(wt).T
        R[b], S[b] = r, s
    return R, (3 * C + 16) * E32 * S


def conv3_stats_ref(h, L, n_part=16, mut=None):
    """{sum, sumsq} per row of the stored h [nb * L][H] (exact inputs).  The kernels add at most 12 values per lane in
    f32 (H / TPP outputs of a position, or 4 NT of a 16-row unit's lane) before going to fp64: n_part = 16; the fp64
    sums run over L H values.  mut 'unit_first': every 16-row unit's sums credited to the row of its first position."""
    M, H = h.shape
    st, tol = stats_of(h.reshape(-1, L, H), np.zeros((M // L, L, H)), n_part=n_part, n64=L * H)
    if mut == "unit_first":
        gi = (np.arange(M) // 16 * 16) // L
        ng = M // L
        st = np.stack([np.bincount(gi, h.sum(1), ng), np.bincount(gi, (h * h).sum(1), ng)], -1)
    return st, tol


def gn_affine(v, gi, stats, count, w, b, d=0.0, dm=0.0, drr=0.0):
    """z = (v - m) r w + b with (m, r) of GroupNorm row gi[p] for position p (v [M][n]); the rule of the module
    docstring.  Returns (z, tol)."""
    m, r = gn_params(stats, count)
    m, r = m[gi][:, None], r[gi][:, None]
    c = (v - m) * r * w
    tol = np.abs(w) * r * (d + dm + np.abs(v - m) * drr) + 4 * E32 * (np.abs(c) + np.abs(b) + np.abs(m) * r * np.abs(w))
    return c + b, tol


def gelu_step(v, tol, fast):
    """the parent's GELU rule: 1.13 x the input bound + 8e |v| (+ GELU_FAST_ABS for the tanh form)"""
    return gelu(v), 1.13 * tol + 8 * E32 * np.abs(v) + (GELU_FAST_ABS if fast else 0.0)


def gelu_tanh(v):
    """the bf16 mode's GELU as common.h documents it: v sigmoid(sqrt(8 / pi) (v + 0.044715 v^3))"""
    with np.errstate(over="ignore"):
        return v * sigmoid(1.5957691216057308 * (v + 0.044715 * v ** 3))


def gelu_tanh_step(v, tol):
    """gelu_tanh(v) of v known to tol, evaluated as gelu_fast does (module docstring, fenc_row)"""
    u = 1.5957691216057308 * (v + 0.044715 * v ** 3)
    with np.errstate(over="ignore"):               # (exp(-u) -> inf for very negative v: sigmoid 0)
        sg = sigmoid(u)
    return v * sg, 1.13 * tol + np.abs(v) * sg * ((1.0 - sg) * (5.0 * np.abs(u) + 2.0) + 4.0) * E32


def glu_step(a, da, g, dg, fast):
    """a sigma(g) and its bound (module docstring)"""
    sg = sigmoid(g)
    f = sg * ((1.0 - sg) * (np.abs(g) + 4.0) + 4.0) * E32 if fast else 0.0
    return a * sg, da * sg + np.abs(a) * (dg / 4 + 4 * E32 + f)


def gn_gelu_ref(h, L, stats, w, b, fast=True, out_bf16=True):
    """GELU(GN(h)) of h [M][H] with the given per-row statistics {sum, sumsq} over L H values -> (y, tol)"""
    M, H = h.shape
    z, tz = gn_affine(h, np.arange(M) // L, stats, L * H, w, b)
    y, t = gelu_step(z, tz, fast)
    if out_bf16:
        t = t + hulp16(np.abs(y) + t)
    return y, t


def moment_stats_ref(x, L, w1, b1, d=None, mut=None, chunk=1 << 15, n_part=0):
    """GroupNorm statistics {sum, sumsq} of y = W1 x + b1 (N = 2C outputs) per row of L positions, x [M][H], and
    the bound of their moment-form evaluation in f32 (module docstring); evaluated chunk positions at a time.
    d: bound on x (None: exact).
    mut: 'swap' (v and ws swapped), 'no2' (factor 2 dropped), 'nob2' (sum b^2 dropped), 'boundary' (the first
    position of every row but the first credited to the row before)."""
    M, H = x.shape
    G, v, ws, sb, sb2 = w1.T @ w1, w1.T @ b1, w1.sum(0), b1.sum(), (b1 * b1).sum()
    aG = np.abs(G)
    k = (H * H + 3 * H + 4 + 1 + n_part) * E32      # n_part: f32 additions between positions (fenc_row)
    n64 = L * 2.0 ** -53
    ng = (M + L - 1) // L
    st, tol = np.zeros((ng, 2)), np.zeros((ng, 2))
    for p0 in range(0, M, chunk):
        xc = x[p0:p0 + chunk]
        y = xc @ w1.T + b1
        s1, s2 = y.sum(1), (y * y).sum(1)
        if mut == "swap":
            s1, s2 = sb + xc @ v, sb2 + 2 * (xc @ ws) + ((xc @ G) * xc).sum(1)
        elif mut == "no2":
            s2 = sb2 + xc @ v + ((xc @ G) * xc).sum(1)
        elif mut == "nob2":
            s2 = s2 - sb2
        ax = np.abs(xc)
        A1 = abs(sb) + ax @ np.abs(ws)
        A2 = sb2 + 2 * (ax @ np.abs(v)) + ((ax @ aG) * ax).sum(1)
        t1, t2 = k * A1, k * A2
        if d is not None:
            dc = d[p0:p0 + chunk]
            t1 = t1 + dc @ np.abs(ws)
            t2 = t2 + 2 * (dc @ np.abs(v)) + 2 * ((ax @ aG) * dc).sum(1) + ((dc @ aG) * dc).sum(1)
        pos = np.arange(p0, p0 + xc.shape[0])
        gi0 = pos // L
        gi = gi0
        if mut == "boundary":
            gi = gi0 - ((pos % L == 0) & (gi0 > 0))
        st += np.stack([np.bincount(gi, s1, ng), np.bincount(gi, s2, ng)], -1)
        tol += np.stack([np.bincount(gi0, t1 + n64 * A1, ng), np.bincount(gi0, t2 + n64 * A2, ng)], -1)
    return st, tol


def dconv_apply_ref(hv, d_hv, w1, b1, st_y, L, g2w, g2b, scale, x, fast, out_bf16, mut=None, dm=0.0, drr=0.0,
                    folded=False):
    """x + scale GLU(GN(W1 hv + b1)) per position: hv [M][H] known to d_hv (None: exact), w1 [2C][H], b1 / g2w / g2b
    [2C] in natural order ('a' half first), st_y the given per-row {sum, sumsq} of the 1x1 output over L 2C values,
    scale [C], x [M][C].  Returns (R, tol_value, tol_stored): the bound of the f32 value and of what is stored (bf16:
    + half an ulp).  1x1: (H + 16) e S + |W1| d_hv; GroupNorm, GLU rules; LayerScale and residual: |scale| d +
    2e (|x| + |scale glu|).
    mut: 'swap' (a and gate halves swapped), 'gate_tile' (gate from the neighbouring 16-channel tile), 'scale_packed'
    (LayerScale indexed by the packed column), 'unit_first' (GroupNorm row of the 16-row unit's first position),
    'no_res' (residual not added).  dm, drr: the bound of the statistics themselves (0: read from memory); folded:
    the affine in fenc_row's folded form."""
    M, H = hv.shape
    C = w1.shape[0] // 2
    y = hv @ w1.T + b1
    S = np.abs(hv) @ np.abs(w1).T + np.abs(b1)
    ty = (H + 16) * E32 * S
    if d_hv is not None:
        ty = ty + d_hv @ np.abs(w1).T
    gi = np.arange(M) // L
    if mut == "unit_first":
        gi = (np.arange(M) // 16 * 16) // L
    z, tz = gn_affine(y, gi, st_y, L * 2 * C, g2w, g2b, d=ty, dm=dm, drr=drr)
    if folded:      # fenc_row: y' (r w s) + ((b1 - m) (r w) + beta) s, see the module docstring
        m_, r_ = gn_params(st_y, L * 2 * C)
        m_, r_ = m_[gi][:, None], r_[gi][:, None]
        tz = tz + 6 * E32 * (np.abs(y - b1) + np.abs(b1 - m_)) * r_ * np.abs(g2w) + 4 * E32 * np.abs(g2b)
    a, g, ta, tg = z[:, :C], z[:, C:], tz[:, :C], tz[:, C:]
    if mut == "swap":
        a, g, ta, tg = g, a, tg, ta
    if mut == "gate_tile":
        perm = (np.arange(C) + 16) % C
        g, tg = g[:, perm], tg[:, perm]
    glu, tglu = glu_step(a, ta, g, tg, fast)
    sc = np.asarray(scale, dtype=np.float64)
    if mut == "scale_packed":      # channel c sits at packed column 32 (c // 16) + c % 16
        sc = sc[(32 * (np.arange(C) // 16) + np.arange(C) % 16) % C]
    res = 0.0 if mut == "no_res" else x
    R = res + sc * glu
    tol = np.abs(sc) * tglu + 2 * E32 * (np.abs(x) + np.abs(sc * glu))
    return R, tol, tol + (hulp16(np.abs(R) + tol) if out_bf16 else 0.0)


def dconv_rewrite_ref(xnew, d, wr, br, mut=None, row_add=None):
    """The encoder layer's rewrite on the updated rows: GLU(Wr bf16(xnew) + br), wr [2C][C] natural order, xnew known
    to d before its bf16 rounding.  tol = (C + 16) e S + amb |Wr| through the GLU rule + half a bf16 ulp.
    mut 'natural_k': the kernel's K slots read in natural instead of permuted order."""
    C = xnew.shape[1]
    xb, amb = bf16_round_amb(xnew, d)
    if mut == "natural_k":
        K2 = (C + 31) // 32 * 32
        wp = rewrite_pack(wr)                       # [2C][K2] packed rows
        xk = np.zeros((xnew.shape[0], K2))
        xk[:, :C] = xb                              # slot k <- channel k
        inv = [glu_src(i, 2 * C) for i in range(2 * C)]
        y = np.empty((xnew.shape[0], 2 * C))
        y[:, inv] = xk @ wp.T
        y = y + br
    else:
        y = xb @ wr.T + br
    S = np.abs(xb) @ np.abs(wr).T + np.abs(br)
    ty = (C + 16) * E32 * S + amb @ np.abs(wr).T
    if row_add is not None:       # fenc_row level 0 (gate bias and scaling folded: two more roundings of the gate)
        ty = ty + 4 * E32 * S
    out, t = glu_step(y[:, :C], ty[:, :C], y[:, C:], ty[:, C:], True)
    if row_add is not None:
        out = out + row_add
        t = t + 2 * E32 * (np.abs(out) + np.abs(row_add))
    return out, t + hulp16(np.abs(out) + t)


# ------------------------------------------------------------------------------------------------ fenc_row
FENC_NPART = {0: (21, 10), 1: (26, 20)}       # f32 reduction depth of the (conv3, 1x1) statistics (module docstring)


def onepass_bounds(v, t, n_part, count=None):
    """one-pass f32 GroupNorm statistics of the values v known to t (module docstring) -> ({sum, sumsq}, dm, drr)"""
    n = v.size if count is None else count
    s1, s2 = v.sum(), (v * v).sum()
    a = np.abs(v)
    return _onepass(s1, s2, t.sum() + n_part * E32 * a.sum(),
                    (2 * a * t + t * t).sum() + (n_part + 2) * E32 * s2, n)


def _onepass(s1, s2, ds1, ds2, n):
    m = s1 / n
    dm = ds1 / n + E32 * abs(m)
    var = max(s2 / n - m * m, 0.0)
    dvar = ds2 / n + 2 * abs(m) * dm + dm * dm + 3 * E32 * (s2 / n + m * m)
    r = 1.0 / math.sqrt(var + 1e-5)
    lo, hi = 1.0 / math.sqrt(var + dvar + 1e-5), 1.0 / math.sqrt(max(var - dvar, 0.0) + 1e-5)
    return np.array([[s1, s2]]), dm, max(1.0 - lo / r, hi / r - 1.0) + 4 * E32


def fenc_row_ref(level, p, xin, a_norm, f, Fin, row_add=None, mut=None):
    """One (b, f) row of a frequency-encoder level (fenc_row.hip's header): Conv2d (8,1) stride
    (4,1) padding (2,0) over frequency -> GELU -> two DConv layers (dilation 1, 2) over the row's T positions ->
    rewrite 1x1 -> GLU (+ the frequency embedding row).  xin: the batch item's input as [Fin][T][Cin] values (level 0:
    raw f32 values, normalised here by a_norm = (sub, div) and rounded to bf16; level 1: bf16 values).  p: natural-
    order weights (wc [C][Cin][8], bc, and per layer w3 [H][C][3], b3, g1w, g1b, w1 [2C][H], b1, g2w, g2b, scale;
    wr [2C][C], br).  Both GELUs are the tanh form.  Returns (out [T][C], tol) with the end-to-end bound of the module
    docstring.
    mut: 'tap_shift' (frequency taps shifted by one), 'emb_next' (embedding row f + 1), 'count_pad' (the statistics
    count includes the positions of the last 16-position tile >= T)."""
    T, Cin = xin.shape[1], xin.shape[2]
    C = p["wc"].shape[0]
    H = C // 8
    np3, npy = FENC_NPART[level]
    a = np.zeros((T, 8, Cin))
    amb = np.zeros((T, 8, Cin))
    for tap in range(8):
        fi = 4 * f - 2 + tap + (1 if mut == "tap_shift" else 0)
        if 0 <= fi < Fin:
            if level == 0:
                a[:, tap], amb[:, tap] = bf16_round_amb((xin[fi] - a_norm[0]) / a_norm[1])
            else:
                a[:, tap] = xin[fi]
    wc = np.transpose(p["wc"], (0, 2, 1)).reshape(C, 8 * Cin)          # [C][tap Cin + ci]
    a, amb = a.reshape(T, 8 * Cin), amb.reshape(T, 8 * Cin)
    v = a @ wc.T + p["bc"]
    tv = (8 * Cin + 16) * E32 * (np.abs(a) @ np.abs(wc).T + np.abs(p["bc"])) + amb @ np.abs(wc).T
    x, d = gelu_tanh_step(v, tv)
    Tc = (T + 15) // 16 * 16 if mut == "count_pad" else T
    for dd in range(2):
        q = p["dc"][dd]
        xb, ax = bf16_round_amb(x, d)
        h, th = dconv_conv3_ref(xb[None], q["w3"], q["b3"], 1 << dd)
        th = th[0] + dconv_conv3_ref(ax[None], np.abs(q["w3"]), np.zeros(H), 1 << dd)[0][0]
        h = h[0]
        st, dm, drr = onepass_bounds(h, th, np3, count=H * Tc)
        z, tz = gn_affine(h, np.zeros(T, dtype=np.int64), st, H * Tc, q["g1w"], q["g1b"], d=th, dm=dm, drr=drr)
        hv, dhv = gelu_tanh_step(z, tz)
        hb, ah = bf16_round_amb(hv, dhv)
        sy, sty = moment_stats_ref(hb, T, q["w1"], q["b1"], d=ah, n_part=npy)
        _, dmy, drry = _onepass(sy[0, 0], sy[0, 1], sty[0, 0], sty[0, 1], 2 * C * Tc)
        # (count_pad: sums over T positions divided by 2C Tc, i.e. the statistics scaled by T / Tc)
        xn, t, _ = dconv_apply_ref(hb, ah, q["w1"], q["b1"], sy * (T / Tc), T, q["g2w"], q["g2b"], q["scale"], x, True,
                                   False, dm=dmy, drr=drry, folded=True)
        x, d = xn, d + t
    ra = None
    if row_add is not None:
        ra = row_add[(f + 1) % row_add.shape[0] if mut == "emb_next" else f]
    elif level == 0:
        ra = np.zeros(C)
    return dconv_rewrite_ref(x, d, p["wr"], p["br"], row_add=ra)


# ------------------------------------------------------------------------------------------------ decoder
SKIP_GAIN = 0.1               # ATHTDemucs_v2.py:102 / :137: x + 0.1 * resize(skip)


def lin_index_ref(in_size, out_size, fma=True):
    """common.h lin_index for dst = 0 .. out_size - 1 in float32 -> (i0, i1, l0, l1) (int64, int64, float32, float32).
    fma: src = scale (dst + 0.5) - 0.5 rounded once (the device compiler contracts the multiply-add; the product of two
    float32 and the - 0.5 are exact in float64 for sizes below 2^24, so one rounding of the float64 value is the fused
    result); False: the product rounded first (a host build without fused multiply-add)."""
    f = np.float32
    d = np.arange(out_size)
    if in_size == out_size:
        return d.copy(), d.copy(), np.ones(out_size, dtype=f), np.zeros(out_size, dtype=f)
    scale = f(in_size) / f(out_size)
    t = d.astype(f) + f(0.5)
    if fma:
        src = (t.astype(np.float64) * np.float64(scale) - 0.5).astype(f)
    else:
        src = (t * scale).astype(f) - f(0.5)
    src = np.maximum(src, f(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    lam = np.clip(src - i0.astype(f), f(0), f(1)).astype(f)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, (f(1) - lam).astype(f), lam


def lin_slack(in_size, out_size):
    """bound on the change of a lerp weight when scale (dst + 0.5) is rounded before the - 0.5 (lin_index_ref's two
    forms): one rounding of a product below in_size.  Not part of any kernel bound: the device evaluates the fused form
    bit for bit (tests/test_gpu_dec.py test_fdec_lr_steps), so the references use the kernels' own weights."""
    return 0.0 if in_size == out_size else E32 * in_size


def resize_h_ref(x, H_out, axis=1, tol=None, mut=None):
    """linear resize of x along `axis` by lin_index_ref (float64 values, float32 weights) -> (R, T): T = the resized
    input bound `tol` + 3e (l0 |a| + l1 |b|) (two products, one sum).  Equal sizes: the identity, (x, tol).
    mut 'i1_as_i0': row i1 taken as i0."""
    x = np.asarray(x, dtype=np.float64)
    t = np.zeros_like(x) if tol is None else np.broadcast_to(np.asarray(tol, dtype=np.float64), x.shape)
    H_in = x.shape[axis]
    if H_in == H_out:
        return x.copy(), t.copy()
    i0, i1, l0, l1 = lin_index_ref(H_in, H_out)
    if mut == "i1_as_i0":
        i1 = i0
    sh = [1] * x.ndim
    sh[axis] = H_out
    l0, l1 = l0.astype(np.float64).reshape(sh), l1.astype(np.float64).reshape(sh)
    a, b = np.take(x, i0, axis=axis), np.take(x, i1, axis=axis)
    T = l0 * np.take(t, i0, axis=axis) + l1 * np.take(t, i1, axis=axis)
    T = T + 3 * E32 * (l0 * np.abs(a) + l1 * np.abs(b))
    return l0 * a + l1 * b, T


def dec_merge_ref(src, skip, H_out, P, stats=None, gn_count=0, gn_w=None, gn_b=None, fast=False, folded=False,
                  kept=False, proj_w=None, proj_b=None, out_bf16=False, act_bf16=False, wsum=False, d_src=None,
                  mut=None):
    """kernels.h MergeDesc: out[item][ho][w][c] = resize_H(act(GN(src)))[ho][w][c] + 0.1 resize_H(skip[item / P])[..][c]
    (ATHTDemucs_v2.py:88-103 / :126-138).  src [NI][H_src][W][C] logical ConvT rows (float64 values as stored), skip
    [NI / P][H_skip][W][C_skip >= C]; stats: the fp64 {sum, sumsq} per item the kernel reads (exact inputs, dm = drr =
    0; None: no GroupNorm and no activation); fast: the tanh GELU (gelu_tanh_step), else erf (gelu_step); folded: the
    affine evaluated as x (r w) + (b - m r w) (adds 6e (|x| + |m|) r |w| + 4e |b|: x and m no longer cancel before the
    roundings); act_bf16: the activated rows are rounded to bf16 before the resize (tdec_tail's LDS tile); wsum: the
    two GELUs of a resize share one reciprocal (common.h gelu_fast_wsum_pk: + 8e of each weighted term); d_src: bound
    on src itself.  kept: only rows 4d + 1, 4d + 2 of src exist (the others are NaN here: they must not be read).
    proj_w [2][C], proj_b [2]: the 1x1 projection, out [NI][W][H_out][2].  Returns (R, tol).
    mut: 'i1_as_i0', 'skip_next_seg', 'skip_prompt' (the skip rows of the segment of item + 1), 'no_gain' (the 0.1
    dropped), 'gn_next_item' (GroupNorm statistics of item n + 1)."""
    src = np.asarray(src, dtype=np.float64)
    skip = np.asarray(skip, dtype=np.float64)
    NI, H_src, W, C = src.shape
    nseg = NI // P
    a = src.copy()
    ta = np.zeros_like(a) if d_src is None else np.array(d_src, dtype=np.float64)
    if kept:
        dead = np.ones(H_src, dtype=bool)
        dead[1::4] = dead[2::4] = False
        a[:, dead] = np.nan
    if stats is not None:
        st = np.asarray(stats, dtype=np.float64).reshape(NI, 2)
        if mut == "gn_next_item":
            st = np.roll(st, -1, axis=0)
        m, r = gn_params(st, gn_count)
        m, r = m[:, None, None, None], r[:, None, None, None]
        w, b = np.asarray(gn_w, dtype=np.float64), np.asarray(gn_b, dtype=np.float64)
        c = (a - m) * r * w
        tz = np.abs(w) * r * ta + 4 * E32 * (np.abs(c) + np.abs(b) + np.abs(m) * r * np.abs(w))
        if folded:
            tz = tz + 6 * E32 * (np.abs(a) + np.abs(m)) * r * np.abs(w) + 4 * E32 * np.abs(b)
        z = c + b
        if fast:
            a, ta = gelu_tanh_step(z, tz)
        else:
            a, ta = gelu_step(z, tz, False)
        if act_bf16:
            a, amb = bf16_round_amb(a, ta)
            ta = amb              # (the rounding itself is exact in the reference; amb: the kernel's other neighbour)
    with np.errstate(invalid="ignore"):
        mres, tm = resize_h_ref(a, H_out, axis=1, tol=ta, mut=mut)
    if wsum and H_src != H_out:
        i0, i1, l0, l1 = lin_index_ref(H_src, H_out)
        sh = (1, H_out, 1, 1)
        tm = tm + 8 * E32 * (l0.reshape(sh) * np.abs(np.take(a, i0, axis=1)) + l1.reshape(sh) * np.abs(np.take(a, i1, axis=1)))
    sk, tsk = resize_h_ref(skip[..., :C], H_out, axis=1)
    g = 1.0 if mut == "no_gain" else SKIP_GAIN
    sk, tsk = g * sk, g * tsk + 2 * E32 * g * np.abs(sk)         # (the float32 0.1 and the product)
    seg = np.arange(NI) // P
    if mut == "skip_next_seg":
        seg = (seg + 1) % nseg
    elif mut == "skip_prompt":
        seg = ((np.arange(NI) + 1) // P) % nseg
    v = mres + sk[seg]
    tv = tm + tsk[seg] + 2 * E32 * (np.abs(mres) + np.abs(sk[seg]))
    if proj_w is not None:
        pw, pb = np.asarray(proj_w, dtype=np.float64), np.asarray(proj_b, dtype=np.float64)
        o = v @ pw.T + pb
        to = tv @ np.abs(pw).T + (C + 4) * E32 * (np.abs(v) @ np.abs(pw).T + np.abs(pb))
        return np.transpose(o, (0, 2, 1, 3)).copy(), np.transpose(to, (0, 2, 1, 3)).copy()
    if out_bf16:
        tv = tv + hulp16(np.abs(v) + tv)
    return v, tv


def dec_last_fold_ref(w, b, P, pb, br):
    """the fold of dec_last.hip's header in float64 (not rounded): freq [Am | A0 | Ap] (3 x [2][48]), P b + pb (2),
    0.1 P (8); time Q_k (8 x [2][48]), P b (2), pb (2), 0.1 P (8)"""
    w, b, P, pb = (np.asarray(v, dtype=np.float64) for v in (w, b, P, pb))
    Q = np.einsum("jc,ick->kji", P, w)                 # Q[k][j][ci] = sum_c P[j][c] w[ci][c][k]
    if br == 0:
        return np.concatenate([(0.5 * Q[7]).ravel(), (0.5 * (Q[3] + Q[4])).ravel(), (0.5 * Q[0]).ravel(), P @ b + pb,
                               (0.1 * P).ravel()])
    return np.concatenate([Q.ravel(), P @ b, pb, (0.1 * P).ravel()])


def dec_last_ref(br, x, w, b, Pm, pb, skip, P, T=None, d_in=None, mut=None):
    """The last decoder level from the unfolded weights (dec_last.hip's header; ATHTDemucs_v2.py:76-104 / :125-139 with
    i = 3, then freq_out / time_out): ConvTranspose (k8 s4 p2) 48 -> 4 over H, linear resize 4H -> H (freq) or T (time),
    + 0.1 resize(skip[item / P][..., :4]), 1x1 projection Pm [2][4] + pb.
    freq (br 0): x [NI][H][W][48], skip [NI / P][H_skip][W][C_skip] -> out [NI][W][H][2];
    time (br 1): x [NI][H][48], skip [NI / P][H_skip][C_skip] -> out [NI][T][2].
    tol = (K + 32) e A with A the same chain on absolute values and K = 3 x 48 (freq: three folded matrices) or 4 x 48
    (time: two ConvT rows of two taps each); the + 32 covers the folded weights' own float32 rounding (e of |P| |W|),
    the skip products and the final sums; + the resize bounds of resize_h_ref through |Pm|; d_in: bound on x, carried
    through |w|, the resizes and |Pm|.
    mut: 'taps34' (taps 3 and 4 swapped), 'am_ap' (taps 7 and 0: Am and Ap swapped), 'no_bias' (ConvT bias dropped),
    'no_gain', 'skip_next_seg', 'skip_prompt', 'i1_as_i0' (of the skip resize)."""
    x = np.asarray(x, dtype=np.float64)
    skip = np.asarray(skip, dtype=np.float64)
    w = np.array(w, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    Pm, pb = np.asarray(Pm, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    if br == 1:
        x, skip = x[:, :, None, :], skip[:, :, None, :]
        if d_in is not None:
            d_in = np.asarray(d_in)[:, :, None, :]
    NI, H = x.shape[0], x.shape[1]
    Ho = H if br == 0 else int(T)
    if mut == "taps34":
        w[:, :, [3, 4]] = w[:, :, [4, 3]]
    elif mut == "am_ap":
        w[:, :, [0, 7]] = w[:, :, [7, 0]]
    bb = np.zeros_like(b) if mut == "no_bias" else b
    y, S = convt_ref_direct(x, w, bb)
    ty = np.zeros_like(y) if d_in is None else convt_ref_direct(np.asarray(d_in, dtype=np.float64), np.abs(w), 0 * b)[0]
    yr, tyr = resize_h_ref(y, Ho, axis=1, tol=ty)
    Sr, _ = resize_h_ref(S, Ho, axis=1)
    sk, tsk = resize_h_ref(skip[..., :4], Ho, axis=1, mut=mut if mut == "i1_as_i0" else None)
    ska, _ = resize_h_ref(np.abs(skip[..., :4]), Ho, axis=1)
    g = 1.0 if mut == "no_gain" else SKIP_GAIN
    seg = np.arange(NI) // P
    nseg = NI // P
    if mut == "skip_next_seg":
        seg = (seg + 1) % nseg
    elif mut == "skip_prompt":
        seg = ((np.arange(NI) + 1) // P) % nseg
    v = yr + g * sk[seg]
    A = (Sr + g * ska[seg]) @ np.abs(Pm).T + np.abs(pb)
    K = 3 * 48 if br == 0 else 4 * 48
    out = v @ Pm.T + pb
    tol = (K + 32) * E32 * A + (tyr + g * tsk[seg]) @ np.abs(Pm).T
    if br == 0:
        return np.transpose(out, (0, 2, 1, 3)).copy(), np.transpose(tol, (0, 2, 1, 3)).copy()
    return out[:, :, 0], tol[:, :, 0]


def lr_steps_ref(Hd, Hs, Hk, H_skip):
    """the step table of kernels.h LrStep, Hd + 1 entries, as a dict of arrays: step v < Hd holds the Z (Hs -> Hd) and
    skip-projection (Hk -> Hd) lerps of row v; step v >= 1 the skip (H_skip -> Hd) lerp of row v - 1; flag bits 0 / 1 /
    2: the z / k / j rows differ from the previous step's (set at their first step: v = 0, 0, 1; clear where the rows
    are not defined).  Entries that are not defined hold -1 (masked to the field width by the packing)."""
    z0, z1, _, lz = lin_index_ref(Hs, Hd)
    k0, k1, _, lk = lin_index_ref(Hk, Hd)
    j0, j1, _, lj = lin_index_ref(H_skip, Hd)
    n = Hd + 1
    out = {k_: np.full(n, -1, dtype=np.int64) for k_ in ("z0", "z1", "k0", "k1", "j0", "j1")}
    out["z0"][:Hd], out["z1"][:Hd], out["k0"][:Hd], out["k1"][:Hd] = z0, z1, k0, k1
    out["j0"][1:], out["j1"][1:] = j0, j1
    out["lz"], out["lk"], out["lj"] = (np.zeros(n, dtype=np.float32) for _ in range(3))
    out["lz"][:Hd], out["lk"][:Hd], out["lj"][1:] = lz, lk, lj
    fl = np.zeros(n, dtype=np.int64)
    for bit, (a, b_), lo, hi in ((1, ("z0", "z1"), 0, Hd), (2, ("k0", "k1"), 0, Hd), (4, ("j0", "j1"), 1, n)):
        ch = np.ones(n, dtype=bool)
        ch[1:] = (out[a][1:] != out[a][:-1]) | (out[b_][1:] != out[b_][:-1])
        ch[:lo] = False
        ch[hi:] = False
        ch[lo] = True
        fl |= np.where(ch, bit, 0)
    out["flags"] = fl
    return out


def fdec_lr_ref(Z, Zs, bias, Hd, P, v3=False):
    """FreqDecoder level 1 from the tap products (fdec_lr.hip's header; ATHTDemucs_v2.py:90-103): Z [NI][Hs][W][8][Co]
    = W_k S[j] and Zs [NI / P][Hk][W][8][Co] = W_k skip3[m] as stored (the resize and the ConvTranspose commute with
    the per-tap 1x1, so the stored products stand for S and skip3).  D0 = resize_H(Z, Hs -> Hd) + 0.1 resize_H(Zs, Hk ->
    Hd) is materialised and the plain ConvTranspose (k8 s4 p2) scatter runs on it: Y[4u - 2 + k] += D0[u][k], + bias.
    Returns (Y [NI][4 Hd][W][Co], tolY).  tolY: the resize bounds + 2e of the sum per D0 value, 3e (|terms| + |bias|)
    per Y row; v3: the incremental base (base += dr at every row change) carries one float32 rounding of the base per
    change: e (|Z[i0]| + 0.1 |Zs[k0]| + |bias|) accumulated over the changes of the step table up to the row's step."""
    Z, Zs, bias = (np.asarray(v, dtype=np.float64) for v in (Z, Zs, bias))
    NI, Hs, W, _, Co = Z.shape
    Hk = Zs.shape[1]
    seg = np.arange(NI) // P
    a, ta = resize_h_ref(Z, Hd, axis=1)
    s, ts = resize_h_ref(Zs, Hd, axis=1)
    s, ts = SKIP_GAIN * s, SKIP_GAIN * ts + 2 * E32 * SKIP_GAIN * np.abs(s)
    D0 = a + s[seg]
    tD = ta + ts[seg] + 2 * E32 * (np.abs(a) + np.abs(s[seg]))
    if v3:
        st = lr_steps_ref(Hd, Hs, Hk, 1)
        aZ, aS = np.abs(Z), SKIP_GAIN * np.abs(Zs)
        drift = np.zeros_like(D0)
        acc = np.zeros_like(D0[:, 0])
        for u in range(Hd):
            if u and st["flags"][u] & 1:
                acc = acc + E32 * (aZ[:, st["z0"][u]] + aS[seg][:, st["k0"][u]] + np.abs(bias))
            if u and st["flags"][u] & 2:
                acc = acc + E32 * (aZ[:, st["z0"][u]] + aS[seg][:, st["k0"][u]] + np.abs(bias))
            drift[:, u] = acc
        tD = tD + drift
    Y = np.zeros((NI, 4 * Hd, W, Co))
    A = np.zeros_like(Y)
    tY = np.zeros_like(Y)
    for k in range(8):
        o = 4 * np.arange(Hd) - 2 + k
        ok = (o >= 0) & (o < 4 * Hd)
        Y[:, o[ok]] += D0[:, :, :, k][:, ok]
        A[:, o[ok]] += np.abs(D0[:, :, :, k][:, ok])
        tY[:, o[ok]] += tD[:, :, :, k][:, ok]
    return Y + bias, tY + 3 * E32 * (A + np.abs(bias))


def fdec_lr_rows(Z, Zs, bias, Hd, P):
    """the ConvT rows of fdec_lr_ref without their bounds (the same chain, values only)"""
    Z, Zs, bias = (np.asarray(v, dtype=np.float64) for v in (Z, Zs, bias))
    NI = Z.shape[0]

    def lerp(x):
        if x.shape[1] == Hd:
            return x
        i0, i1, l0, l1 = lin_index_ref(x.shape[1], Hd)
        sh = (1, Hd, 1, 1, 1)
        return l0.astype(np.float64).reshape(sh) * x[:, i0] + l1.astype(np.float64).reshape(sh) * x[:, i1]
    D0 = lerp(Z) + (SKIP_GAIN * lerp(Zs))[np.arange(NI) // P]
    Y = np.zeros((NI, 4 * Hd) + Z.shape[2:3] + Z.shape[4:])
    for k in range(8):
        o = 4 * np.arange(Hd) - 2 + k
        ok = (o >= 0) & (o < 4 * Hd)
        Y[:, o[ok]] += D0[:, :, :, k][:, ok]
    return Y + bias


def fdec_lr_stats_ref(Y, tY, Hd):
    """{sum, sumsq} per item over all 4 Hd ConvT rows and their bound (the statistics rule): per thread at most 16 steps
    x 4 rows are added in float32 (n_part = 68), then fp64 over Hd / 16 chunks, the wave, the block and the atomics"""
    nblk = (Y.shape[2] * (Y.shape[3] // 2) + 255) // 256
    return stats_of(Y, tY, n_part=68, n64=Hd // 16 + 16 + nblk)


def gram_z_ref(S, Wt):
    """Z = S W_k^T as the Gram pass holds it in LDS and stores it as z4 (fdec1f.hip's header): the bf16 rounding of a
    float32 accumulation of exact bf16 products, K = Ci.  S [NI][Hs][W][Ci], Wt [8][Co][Ci] (bf16 values) -> (Zr, amb)
    [NI][Hs][W][8][Co]: bf16_round_amb of the float64 product with the GEMM bound (K + 16) e |S| |W|."""
    S, Wt = np.asarray(S, dtype=np.float64), np.asarray(Wt, dtype=np.float64)
    sh = S.shape[:-1] + Wt.shape[:2]
    W2 = Wt.reshape(-1, Wt.shape[-1])
    Zx = (S.reshape(-1, S.shape[-1]) @ W2.T).reshape(sh)
    Za = (np.abs(S).reshape(-1, S.shape[-1]) @ np.abs(W2).T).reshape(sh)
    return bf16_round_amb(Zx, (S.shape[-1] + 16) * E32 * Za)


def fdec1_gram_stats_ref(Zr, amb, Zs, bias, Hd, P):
    """{sum, sumsq} per item over the 4 Hd ConvT rows of fdec_lr_ref on (Zr, Zs), and the bound of their evaluation as
    quadratic forms of per-item Gram matrices (fdec1f.hip's header): the Gram entries and per-channel sums are float32
    accumulations of exact bf16 products over the item's (w, c), 16 W per channel group, then the partial slots and the
    6 groups: n = 16 W + 32 additions, each bounded by e times the form on absolute values (every lerp coefficient is
    >= 0, so <Q, |x| |x|^T> is the sum of squares of the same chain on |Z|, |Zs|, |bias|: the cancellation between
    sum b^2, 2 c1 . ub and <Q, G> at a large mean is inside it); the coefficients (double, from the float32 lambda) and
    the final sums are fp64.  amb (gram_z_ref: Z elements the kernel may have rounded to the other neighbour) goes
    through the same positive chain into the statistics rule."""
    Y = fdec_lr_rows(Zr, Zs, bias, Hd, P)
    tY = fdec_lr_rows(amb, 0.0 * np.asarray(Zs), 0.0 * np.asarray(bias), Hd, P)
    Ya = fdec_lr_rows(np.abs(Zr), np.abs(Zs), np.abs(bias), Hd, P)
    n = 16 * Zr.shape[2] + 32
    ax = (1, 2, 3)
    st = np.stack([Y.sum(axis=ax), (Y * Y).sum(axis=ax)], -1)
    t1 = tY.sum(axis=ax) + n * E32 * Ya.sum(axis=ax)
    t2 = (2 * np.abs(Y) * tY + tY * tY).sum(axis=ax) + n * E32 * (Ya * Ya).sum(axis=ax)
    return st, np.stack([t1, t2], -1), Y


# ---------------------------------------------------------------------------------------------- encoder level shapes
ENC_CH = (48, 96, 192, 384)


def encoder_levels(T, B):
    """The DConv problem of every encoder level for B segments of T samples (csrc/forward_plan.cpp make_dims):
    {stage: (C, nb, L, cin, rewrite_fusable)}.  Frequency level i: nb = B F[i + 1] rows of Tspec = ceil(T / 1024) frames;
    time level i: nb = B rows of L[i + 1] = ceil(L[i] / 4) samples, the only one whose rewrite the apply pass can take."""
    Ts, F, L = -(-T // 1024), 2048, T
    out = {}
    for i, C in enumerate(ENC_CH):
        F, L = F // 4, -(-L // 4)
        out["fenc%d" % i] = (C, B * F, Ts, 4 if i == 0 else ENC_CH[i - 1], 0)
        out["tenc%d" % i] = (C, B, L, 2 if i == 0 else ENC_CH[i - 1], 1)
    return out
