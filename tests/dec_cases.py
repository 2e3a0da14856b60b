"""Inputs and float32 emulations shared by tests/test_dec_refs.py (CPU) and tests/test_gpu_dec.py (GPU): a plain helper
module, not a test.

Inputs follow the rules of tests/test_gpu_dconv.py: neighbouring items and segments are scaled by different powers of
two (a value taken from the wrong item or segment is off by at least 2x), the skip tensors are of order 4 (the model's
0.1 gain would otherwise hide the skip branch beside the main one), GroupNorm weights 1 + 0.25 N, biases 0.1 N, and every
value is exactly representable in the type the kernel reads it in.

The emulations evaluate the documented operation order in numpy float32 (bf16 at the documented rounding points, the
tanh GELU where fast_gelu): an honest low-precision evaluation has to stay inside the derived bounds of
tests/kernel_refs.py, or the bounds are wrong."""
import numpy as np

import kernel_refs as kr

F = np.float32


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def stored(a, bf16):
    """values as the device holds them (float64 of the bf16 / float32 rounding)"""
    return kr.bf16_round(a) if bf16 else f32(a)


def pscale(n, shift=0):
    return 2.0 ** ((np.arange(n) + shift) % 5)


def gn_affine_params(C, rng):
    return f32(1 + 0.25 * rng.standard_normal(C)), f32(0.1 * rng.standard_normal(C))


def true_stats(src):
    """{sum, sumsq} per item of src [NI][...] (exact fp64 inputs of the kernels)"""
    ax = tuple(range(1, src.ndim))
    return np.stack([src.sum(axis=ax), (src * src).sum(axis=ax)], -1)


# ------------------------------------------------------------------------------------------------------ dec_merge
def merge_case(seed, NI, P, C, H_src, H_out, H_skip, W, C_skip, bf16=False, gn=True, proj=False):
    rng = np.random.default_rng(seed)
    c = dict(NI=NI, P=P, C=C, H_src=H_src, H_out=H_out, H_skip=H_skip, W=W, C_skip=C_skip, bf16=bf16)
    c["src"] = stored((rng.standard_normal((NI, H_src, W, C)) + 0.3) * pscale(NI)[:, None, None, None], bf16)
    c["skip"] = stored(4.0 * rng.standard_normal((NI // P, H_skip, W, C_skip)) * pscale(NI // P, 2)[:, None, None, None],
                       bf16)
    c["stats"] = true_stats(c["src"]) if gn else None
    c["gn_count"] = H_src * W * C
    c["gn_w"], c["gn_b"] = gn_affine_params(C, rng)
    c["proj_w"] = f32(rng.standard_normal((2, C)) / 2) if proj else None
    c["proj_b"] = f32(0.3 * rng.standard_normal(2)) if proj else None
    return c


def merge_ref(c, kept=False, fast=False, folded=False, out_bf16=False, mut=None, **kw):
    return kr.dec_merge_ref(c["src"], c["skip"], c["H_out"], c["P"], stats=c["stats"], gn_count=c["gn_count"],
                            gn_w=c["gn_w"], gn_b=c["gn_b"], fast=fast, folded=folded, kept=kept, proj_w=c["proj_w"],
                            proj_b=c["proj_b"], out_bf16=out_bf16, mut=mut, **kw)


def gelu32(z, fast):
    z = z.astype(F)
    if fast:        # common.h gelu_fast: x rcp(1 + exp2(x fma(K1, x^2, K0)))
        K0 = F(-1.5957691216057308 * 1.4426950408889634)
        K1 = F(K0 * F(0.044715))
        with np.errstate(over="ignore"):
            t = z * (K1 * (z * z) + K0)
            return (z * (F(1) / (F(1) + np.exp2(t, dtype=F)))).astype(F)
    return (F(0.5) * z * (F(1) + kr._erf((z * F(0.70710678118654752440)).astype(np.float64)).astype(F))).astype(F)


def lerp32(x, H_out, axis=1):
    H_in = x.shape[axis]
    if H_in == H_out:
        return x.astype(F)
    i0, i1, l0, l1 = kr.lin_index_ref(H_in, H_out)
    sh = [1] * x.ndim
    sh[axis] = H_out
    a, b = np.take(x, i0, axis=axis).astype(F), np.take(x, i1, axis=axis).astype(F)
    return (l0.reshape(sh) * a + l1.reshape(sh) * b).astype(F)


def gn_act32(a, stats, count, gw, gb, fast, folded):
    """act(GN(a)) in float32: (x - mean) rstd w + b, or folded x (rstd w) + (b - mean rstd w); mean, rstd rounded from
    fp64 (common.h gn_params)"""
    m, r = kr.gn_params(stats, count)
    sh = (-1,) + (1,) * (a.ndim - 1)
    m, r = m.astype(F).reshape(sh), r.astype(F).reshape(sh)
    gw, gb = np.asarray(gw, dtype=F), np.asarray(gb, dtype=F)
    a = a.astype(F)
    if folded:
        ga = (gw * r).astype(F)
        z = a * ga + (gb - m * ga).astype(F)
    else:
        z = (a - m) * r * gw + gb
    return gelu32(z.astype(F), fast)


def merge_emulate(c, kept=False, fast=False, folded=False, out_bf16=False, act_bf16=False):
    a = c["src"].astype(F)
    if c["stats"] is not None:
        a = gn_act32(a, c["stats"], c["gn_count"], c["gn_w"], c["gn_b"], fast, folded)
    if act_bf16:
        a = kr.bf16_round(a).astype(F)
    m = lerp32(a, c["H_out"])
    sv = (lerp32(c["skip"][..., :c["C"]].astype(F), c["H_out"]) * F(0.1)).astype(F)
    v = (m + sv[np.arange(c["NI"]) // c["P"]]).astype(F)
    if c["proj_w"] is not None:
        o = (c["proj_b"].astype(F) + (v[..., None, :] * c["proj_w"].astype(F)).sum(-1, dtype=F)).astype(F)
        return np.transpose(o, (0, 2, 1, 3)).astype(np.float64)
    return kr.bf16_round(v) if out_bf16 else v.astype(np.float64)


# ------------------------------------------------------------------------------------------------------ dec_last
def last_weights(seed):
    """ConvT weight [48][4][8], bias [4], projection [2][4], bias [2] (float32 values)"""
    rng = np.random.default_rng(seed)
    return (f32(rng.standard_normal((48, 4, 8)) / np.sqrt(96.0)), f32(0.5 * rng.standard_normal(4)),
            f32(rng.standard_normal((2, 4)) / 2), f32(0.3 * rng.standard_normal(2)))


def last_case(seed, br, NI, P, H, W, H_skip, C_skip, bf16=False, T=None):
    rng = np.random.default_rng(seed)
    xs = (NI, H, W, 48) if br == 0 else (NI, H, 48)
    ss = (NI // P, H_skip, W, C_skip) if br == 0 else (NI // P, H_skip, C_skip)
    one = (1,) * (len(xs) - 1)
    c = dict(br=br, NI=NI, P=P, H=H, W=W, H_skip=H_skip, C_skip=C_skip, bf16=bf16, T=T if br else None)
    c["x"] = stored((rng.standard_normal(xs) + 0.2) * pscale(NI).reshape((-1,) + one), bf16)
    c["skip"] = stored(4.0 * rng.standard_normal(ss) * pscale(NI // P, 2).reshape((-1,) + one), bf16)
    c["wts"] = last_weights(seed + 1)
    return c


def last_ref(c, x=None, d_in=None, mut=None):
    w, b, Pm, pb = c["wts"]
    return kr.dec_last_ref(c["br"], c["x"] if x is None else x, w, b, Pm, pb, c["skip"], c["P"], T=c["T"], d_in=d_in,
                           mut=mut)


def last_emulate(c, fold, x=None):
    """the folded form of dec_last.hip's header in float32 from the product's fold (pack.h dec_last_fold)"""
    br, NI, P, H = c["br"], c["NI"], c["P"], c["H"]
    x = (c["x"] if x is None else x).astype(F)
    fold = np.asarray(fold, dtype=F)
    seg = np.arange(NI) // P
    if br == 0:
        Am, A0, Ap = (fold[96 * i:96 * (i + 1)].reshape(2, 48) for i in range(3))
        cst, S = fold[288:290], fold[290:298].reshape(2, 4)
        xp = np.zeros((NI, H + 2, c["W"], 48), dtype=F)
        xp[:, 1:H + 1] = x
        s4 = lerp32(c["skip"][..., :4].astype(F), H)[seg]
        o = cst + (s4 @ S.T).astype(F) + (xp[:, :H] @ Am.T).astype(F) + (xp[:, 1:H + 1] @ A0.T).astype(F)
        o = (o + (xp[:, 2:] @ Ap.T).astype(F)).astype(F)
        return np.transpose(o, (0, 2, 1, 3)).astype(np.float64)
    T = int(c["T"])
    Q = fold[:768].reshape(8, 2, 48)
    pbias, tb, S = fold[768:770], fold[770:772], fold[772:780].reshape(2, 4)
    xp = np.zeros((NI, H + 2, 48), dtype=F)
    xp[:, 1:H + 1] = x
    z = np.zeros((NI, 4 * H, 2), dtype=F)
    for rho in range(4):
        lo = xp[:, 1 + kr.RES_OFF[rho]:1 + kr.RES_OFF[rho] + H]
        hi = xp[:, 2 + kr.RES_OFF[rho]:2 + kr.RES_OFF[rho] + H]
        z[:, rho::4] = ((lo @ Q[kr.RES_K0[rho]].T).astype(F) + (hi @ Q[kr.RES_K1[rho]].T).astype(F) + pbias).astype(F)
    s4 = lerp32(c["skip"][..., :4].astype(F), T)[seg]
    return (lerp32(z, T) + tb + (s4 @ S.T).astype(F)).astype(np.float64)


# ---------------------------------------------------------------------------------------------- dec_tail (merge + last)
def tail_case(seed, br, NI, P, H, W, H_skip, C_skip, H_skip2, C_skip2, bf16=False, Hg=None):
    """the level-2 merge in front of the last level: g = the level-2 ConvT output (freq: logical rows 4H, of which the
    kernel sees the kept slots; time: Hg rows), skip2 [NI / P][H_skip2][W][C_skip2]"""
    c = last_case(seed, br, NI, P, H, W, H_skip, C_skip, bf16=bf16, T=4 * H)
    Hg = 4 * H if br == 0 else Hg
    m = merge_case(seed + 7, NI, P, 48, Hg, H, H_skip2, W, C_skip2, bf16=bf16)
    c["merge"] = m
    c["Hg"] = Hg
    return c


def tail_ref(c, mut=None, mut_last=None):
    """(R, tol, x, tx): the merged 48-channel input x (never stored by the kernel) and the output"""
    bf = c["bf16"]
    # bf16: the tanh GELU with the folded affine; freq pairs the two GELUs on one reciprocal, time keeps bf16 rows in LDS
    x, tx = merge_ref(c["merge"], kept=c["br"] == 0, fast=bf, folded=bf, wsum=bf and c["br"] == 0,
                      act_bf16=bf and c["br"] == 1, mut=mut)
    if c["br"] == 1:
        x, tx = x[:, :, 0], tx[:, :, 0]
    R, tol = last_ref(c, x=x, d_in=tx, mut=mut_last)
    return R, tol, x, tx


def tail_emulate(c, fold):
    bf = c["bf16"]
    x = merge_emulate(c["merge"], kept=c["br"] == 0, fast=bf, folded=bf, act_bf16=bf and c["br"] == 1)
    if c["br"] == 1:
        x = x[:, :, 0]
    return last_emulate(c, fold, x=x)


# ------------------------------------------------------------------------------------------------------ fdec_lr
def taps(S, Wt):
    """[..][Ci] x Wt [8][Co][Ci] -> the tap products [..][8][Co]"""
    return (S.reshape(-1, S.shape[-1]) @ Wt.reshape(-1, Wt.shape[-1]).T).reshape(S.shape[:-1] + Wt.shape[:2])


def lr_case(seed, NI, P, Hd, W, Co, H_skip, C_skip, z_bf16, skip_bf16=None, out_bf16=None, Hs=32, Hk=8, Ci=24):
    """Z = the bf16 / float32 rounding of a float64 S @ W_k, so the kernels read exactly representable operands and the
    check is staged (the GEMM that makes Z has its own tests)"""
    rng = np.random.default_rng(seed)
    skip_bf16 = z_bf16 if skip_bf16 is None else skip_bf16
    out_bf16 = z_bf16 if out_bf16 is None else out_bf16
    nseg = NI // P
    S = (rng.standard_normal((NI, Hs, W, Ci)) + 0.2) * pscale(NI)[:, None, None, None]
    K3 = 4.0 * rng.standard_normal((nseg, Hk, W, Ci)) * pscale(nseg, 2)[:, None, None, None]
    Wt = rng.standard_normal((8, Co, Ci)) / np.sqrt(2.0 * Ci)
    c = dict(NI=NI, P=P, Hd=Hd, W=W, Co=Co, H_skip=H_skip, C_skip=C_skip, Hs=Hs, Hk=Hk, z_bf16=z_bf16,
             skip_bf16=skip_bf16, out_bf16=out_bf16, S=S, K3=K3, Wt=Wt)
    c["Z"] = stored(taps(S, Wt), z_bf16)
    c["Zs"] = stored(taps(K3, Wt), z_bf16)
    c["bias"] = f32(0.5 * rng.standard_normal(Co))
    c["gn_w"], c["gn_b"] = gn_affine_params(Co, rng)
    c["skip"] = stored(4.0 * rng.standard_normal((nseg, H_skip, W, C_skip)) * pscale(nseg, 1)[:, None, None, None],
                       skip_bf16)
    return c


def lr_v3_stats(c):
    return bool(c["z_bf16"] and c["Hd"] > c["Hs"] and c["Hd"] > c["Hk"])


def lr_v3_merge(c, fast):
    return bool(c["z_bf16"] and c["skip_bf16"] and c["out_bf16"] and fast and c["Hd"] > c["Hs"] and c["Hd"] > c["Hk"]
                and c["Hd"] > c["H_skip"])


def lr_merge_ref(c, Y, tY, stats, fast, v3, mut=None):
    """D1 from the ConvT rows Y known to tY and the statistics the merge pass reads (exact inputs); merge3 folds the
    GroupNorm affine into y (r w) + (b - m r w) and shares one reciprocal between the two GELUs, merge2 keeps
    (y - m) (r w) + b"""
    return kr.dec_merge_ref(Y, c["skip"], c["Hd"], c["P"], stats=stats, gn_count=4 * c["Hd"] * c["W"] * c["Co"],
                            gn_w=c["gn_w"], gn_b=c["gn_b"], fast=fast, folded=v3, kept=True, out_bf16=c["out_bf16"],
                            wsum=v3, d_src=tY, mut=mut)


def lr_emulate(c, v3):
    """the ConvT rows Y [NI][4 Hd][W][Co] in float32 in the documented order: per step u the 8 tap values T_u[k] = base +
    lz dr(Z) + lk dr(Zs) (base = Z[i0] + 0.1 Zs[k0] (+ bias on taps 2 .. 5); v3: base updated by += dr at every row
    change), then Y[4u + r] = T_u[r + 2] + (r < 2 ? T_{u-1}[r + 6] : T_{u+1}[r - 2])"""
    NI, P, Hd, Hs, Hk = c["NI"], c["P"], c["Hd"], c["Hs"], c["Hk"]
    seg = np.arange(NI) // P
    Z, Zs = c["Z"].astype(F), (c["Zs"].astype(F) * F(0.1)).astype(F)[seg]
    st = kr.lr_steps_ref(Hd, Hs, Hk, 1)
    bias = np.zeros((8, c["Co"]), dtype=F)
    bias[2:6] = c["bias"].astype(F)
    T = np.zeros((NI, Hd + 2, c["W"], 8, c["Co"]), dtype=F)      # T[u + 1] = step u; steps -1 and Hd are zero
    base = zdr = sdr = None
    for u in range(Hd):
        z0, z1, k0, k1 = (int(st[n][u]) for n in ("z0", "z1", "k0", "k1"))
        if u == 0 or not v3:
            if u == 0 or st["flags"][u] & 3:
                zdr, sdr = (Z[:, z1] - Z[:, z0]).astype(F), (Zs[:, k1] - Zs[:, k0]).astype(F)
                base = (Z[:, z0] + Zs[:, k0] + bias).astype(F)
        else:
            if st["flags"][u] & 1:
                base = (base + zdr).astype(F)
                zdr = (Z[:, z1] - Z[:, z0]).astype(F)
            if st["flags"][u] & 2:
                base = (base + sdr).astype(F)
                sdr = (Zs[:, k1] - Zs[:, k0]).astype(F)
        T[:, u + 1] = (st["lz"][u] * zdr + (st["lk"][u] * sdr + base)).astype(F)
    Y = np.zeros((NI, 4 * Hd, c["W"], c["Co"]), dtype=F)
    for r in range(4):
        nb = T[:, :Hd, :, r + 6] if r < 2 else T[:, 2:, :, r - 2]
        Y[:, r::4] = (T[:, 1:Hd + 1, :, r + 2] + nb).astype(F)
    return Y


def lr_stats_emulate(Y32):
    """{sum, sumsq} with float32 partial sums over 16 steps (64 rows) per (w, channel), fp64 above"""
    NI, R = Y32.shape[0], Y32.shape[1]
    s1, s2 = np.zeros(NI), np.zeros(NI)
    for r0 in range(0, R, 64):
        blk = Y32[:, r0:r0 + 64]
        a1, a2 = np.zeros_like(blk[:, 0]), np.zeros_like(blk[:, 0])
        for i in range(blk.shape[1]):
            a1 = (a1 + blk[:, i]).astype(F)
            a2 = (a2 + blk[:, i] * blk[:, i]).astype(F)
        s1 += a1.astype(np.float64).sum(axis=(1, 2))
        s2 += a2.astype(np.float64).sum(axis=(1, 2))
    return np.stack([s1, s2], -1)


def lr_merge_emulate(c, Y32, stats, fast, v3):
    m = dict(src=Y32.astype(np.float64), skip=c["skip"], H_out=c["Hd"], P=c["P"], NI=c["NI"], C=c["Co"], stats=stats,
             gn_count=4 * c["Hd"] * c["W"] * c["Co"], gn_w=c["gn_w"], gn_b=c["gn_b"], proj_w=None, proj_b=None)
    return merge_emulate(m, kept=True, fast=fast, folded=v3, out_bf16=c["out_bf16"])


def lr_steps_pack(st, dtype):
    """lr_steps_ref's table as LrStep records (kernels.h): zk = i0z | i1z << 8 | i0k << 16 | i1k << 24,
    jj = i0j | i1j << 16"""
    out = np.zeros(len(st["flags"]), dtype=dtype)
    out["lz"], out["lk"], out["lj"] = st["lz"], st["lk"], st["lj"]
    zk = (st["z0"] & 0xFF) | (st["z1"] & 0xFF) << 8 | (st["k0"] & 0xFF) << 16 | (st["k1"] & 0xFF) << 24
    out["zk"] = zk.astype(np.uint32)
    out["jj"] = ((st["j0"] & 0xFFFF) | (st["j1"] & 0xFFFF) << 16).astype(np.uint32)
    out["flags"] = st["flags"].astype(np.uint32)
    return out


def z4_pack(Z):
    """Z [..][W][8][Co] -> the 4-tap rows of kernels.h LowRankDesc::z_taps = 4: taps 0, 3, 4, 7 as [..][W][Co / 16][4][16]"""
    lead, Co = Z.shape[:-2], Z.shape[-1]
    z = Z[..., [0, 3, 4, 7], :].reshape(lead + (4, Co // 16, 16))
    return np.ascontiguousarray(np.swapaxes(z, -3, -2))


# ------------------------------------------------------------------------------------------------------ fdec1_gram
def gram_case(seed, NI, P, Hd, W, mean=0.0):
    """the Gram pass's operands: S [NI][32][W][192] and the tap weights Wt [8][96][192] as bf16 values, Zs the bf16
    rounding of a float64 skip3 @ W_k; Z / amb: what the pass holds (kernel_refs.gram_z_ref); mean: added to S (30: the
    large-mean regime where sum b^2, 2 c1 . ub and <Q, G> cancel).  The rows of S grow from 1x to 5x along H, so that the
    last ConvT rows weigh in the statistics (a row count off by one is then visible beside the rounding-tie term)"""
    c = lr_case(seed, NI, P, Hd, W, 96, 32, 96, True, Ci=192)
    c["S"] = kr.bf16_round((c["S"] + mean) * (1.0 + np.arange(32) / 8.0)[None, :, None, None])
    c["Wt"] = kr.bf16_round(c["Wt"])
    c["Zs"] = kr.bf16_round(taps(c["K3"], c["Wt"]))
    c["Z"], c["amb"] = kr.gram_z_ref(c["S"], c["Wt"])
    return c


def gram_coef(Hd, Hs=32, Hk=8):
    """C [4][Hd][80]: ConvT row 4v + rho (class q = (rho + 2) % 4) = bias + C[q][v] . x_q with x_q = (Z_q[0..31],
    Z_{q+4}[0..31], Zs_q[0..7], Zs_{q+4}[0..7]) (fdec1f.hip's header): the row is T_v[rho + 2] + (rho < 2 ? T_{v-1}[rho +
    6] : T_{v+1}[rho - 2]), T_s = lerp of the Z rows + 0.1 lerp of the Zs rows"""
    def lerp_matrix(h_in):
        i0, i1, l0, l1 = kr.lin_index_ref(h_in, Hd)
        M = np.zeros((Hd + 2, h_in))                 # row s + 1 = step s; steps -1 and Hd are zero
        np.add.at(M, (np.arange(Hd) + 1, i0), 1.0 - l1.astype(np.float64))
        np.add.at(M, (np.arange(Hd) + 1, i1), l1.astype(np.float64))
        return M
    Lz, Lk = lerp_matrix(Hs), lerp_matrix(Hk) * float(np.float32(0.1))
    C = np.zeros((4, Hd, 80))
    v = np.arange(Hd)
    for q in range(4):
        rho = (q + 2) % 4
        main = q if rho < 2 else q + 4
        for slot, tap in enumerate((q, q + 4)):
            s = v if tap == main else (v - 1 if rho < 2 else v + 1)
            C[q][:, 32 * slot:32 * slot + 32] = Lz[s + 1]
            C[q][:, 64 + 8 * slot:72 + 8 * slot] = Lk[s + 1]
    return C


def gram_emulate(c, double_count=False):
    """{sum, sumsq} as fdec1f.hip evaluates them: Z = bf16 of a float32 GEMM, per item and class the 80 x 80 Gram matrix
    and the per-channel sums of x_q in float32, then sum y = 4 Hd W sum b + c1 . u and sum y^2 = 4 Hd W sum b^2 +
    2 c1 . ub + <Q, G> in double.  double_count (a mutation): the columns that the last, left-shifted w tile shares with
    the tile before it are counted twice."""
    NI, P, Hd, W = c["NI"], c["P"], c["Hd"], c["W"]
    Zb = kr.bf16_round(np.einsum("nhwi,kci->nhwkc", c["S"].astype(F), c["Wt"].astype(F), dtype=F)).astype(F)
    Zs = c["Zs"].astype(F)
    C = gram_coef(Hd)
    b = c["bias"]
    wsel = np.arange(W)
    if double_count and W % 8:
        wsel = np.concatenate([wsel, np.arange(W - 8, W // 8 * 8)])
    out = np.zeros((NI, 2))
    for n in range(NI):
        s1 = 4.0 * Hd * W * b.sum()
        s2 = 4.0 * Hd * W * (b * b).sum()
        for q in range(4):
            X = np.concatenate([Zb[n, :, :, q], Zb[n, :, :, q + 4], Zs[n // P, :, :, q], Zs[n // P, :, :, q + 4]], 0)
            X = X[:, wsel]                                        # [80][w][96]
            G = (X.reshape(80, -1) @ X.reshape(80, -1).T).astype(F).astype(np.float64)
            u = X.sum(axis=1, dtype=F).astype(np.float64)         # [80][96]
            c1 = C[q].sum(0)
            s1 += c1 @ u.sum(1)
            s2 += 2.0 * c1 @ (u @ b) + ((C[q].T @ C[q]) * G).sum()
        out[n] = s1, s2
    return out
