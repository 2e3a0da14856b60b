"""Inputs of tests/test_gpu_spectral.py and tests/test_spectral_refs.py, and honest emulations of the documented algorithms
of csrc/spectral.hip and csrc/tconv0.hip in float32 numpy (the operation order of the kernels' comments: three radix-16
Stockham passes of two radix-4 layers, running-product twiddles, the register overlap-add with its workgroup split and
boundary join).  The emulations exist to show that the bounds of tests/spectral_refs.py are neither vacuous nor violated
by a correct evaluation; `mut` plants the defects the bounds must separate."""
import math

import numpy as np

import kernel_refs as kr
import spectral_refs as sr

F = np.float32


# ------------------------------------------------------------------------------------------------ inputs
def stft_case(nb, T, seed=0):
    """wav [nb][2][T] float32 noise; batch b scaled by 2^(b % 3 - 1)"""
    rng = np.random.default_rng(1000 + seed)
    wav = rng.standard_normal((nb, 2, T)) * np.ldexp(1.0, np.arange(nb) % 3 - 1)[:, None, None]
    return wav.astype(F)


def istft_case(Tspec, T, S, P, seed=0):
    """S segments x P prompts.  spec [S][Tspec][2048][4]: |Re L|, |Im L| in [0.5, 2] 2^(s % 2 * 2 - 1) (so within
    [0.25, 4]) with random signs, the right channel normal; fo [S P][Tspec][Tspec][2] in [-6, 6] 2^-(item % 3);
    xt2 [S P][T][2] normal 2^(item % 2); tnorm [S][2] = {mean, std}, different per segment"""
    rng = np.random.default_rng(2000 + seed)
    NI = S * P
    spec = rng.standard_normal((S, Tspec, sr.NB, 4))
    mag = rng.uniform(0.5, 2.0, (S, Tspec, sr.NB, 2)) * np.where(rng.random((S, Tspec, sr.NB, 2)) < 0.5, -1.0, 1.0)
    spec[..., :2] = mag
    spec *= np.ldexp(1.0, (np.arange(S) % 2) * 2 - 1)[:, None, None, None]
    fo = rng.uniform(-6.0, 6.0, (NI, Tspec, Tspec, 2)) * np.ldexp(1.0, -(np.arange(NI) % 3))[:, None, None, None]
    xt2 = rng.standard_normal((NI, T, 2)) * np.ldexp(1.0, np.arange(NI) % 2)[:, None, None]
    tnorm = np.stack([0.125 * (1 + np.arange(S)), 0.75 + 0.5 * np.arange(S)], axis=-1)
    return dict(Tspec=Tspec, T=T, S=S, P=P, NI=NI, spec=spec.astype(F), fo=fo.astype(F), xt2=xt2.astype(F),
                tnorm=tnorm.astype(F))


def tconv0_case(B, T, seed=0):
    rng = np.random.default_rng(3000 + seed)
    wav = (rng.standard_normal((B, 2, T)) * np.ldexp(1.0, np.arange(B) % 3 - 1)[:, None, None] + 0.25).astype(F)
    tnorm = np.stack([0.25 - 0.0625 * np.arange(B), 0.5 + 0.375 * np.arange(B)], axis=-1).astype(F)
    w = (rng.standard_normal((48, 16)) * 0.35).astype(F)
    bias = (rng.standard_normal(48) * 0.2).astype(F)
    return dict(B=B, T=T, Lo=-(-T // 4), wav=wav, tnorm=tnorm, w=w, bias=bias)


def textvec_case(NI, P, per_item, seed=0):
    rng = np.random.default_rng(4000 + seed)
    rows = NI if per_item else P
    text = (rng.standard_normal((rows, 512)) * np.ldexp(1.0, np.arange(rows) % 3 - 1)[:, None]).astype(F)
    g = lambda *s: (rng.standard_normal(s) * 0.05).astype(F)
    return dict(NI=NI, P=P, per_item=per_item, text=text, maT=g(512, 384), ma=g(384), mcT=g(512, 384), mc=g(384),
                b2=g(384))


# ------------------------------------------------------------------------------------------------ the FFT, emulated
def _cmul(a, b):
    out = np.empty(np.broadcast(a, b).shape, dtype=np.result_type(a, b))
    out.real = a.real * b.real - a.imag * b.imag
    out.imag = a.real * b.imag + a.imag * b.real
    return out


def _mi(a):
    """-i a"""
    out = np.empty_like(a)
    out.real, out.imag = a.imag, -a.real
    return out


def _r4(x0, x1, x2, x3):
    s02, d02, s13, d13 = x0 + x2, x0 - x2, x1 + x3, x1 - x3
    m = _mi(d13)
    return s02 + s13, d02 + m, s02 - s13, d02 - m


def _dft16(v):
    """v[r], r = 4 r1 + r0 -> list o[q] of the 16 output bins (spectral.hip dft16 / vq)"""
    ct = v[0].dtype
    rt = F if ct == np.complex64 else np.float64
    C1, S1, C2 = rt(0.92387953251128675613), rt(0.38268343236508977173), rt(0.70710678118654752440)
    c = lambda x, y: np.asarray(complex(x, y)).astype(ct)
    v = list(v)
    for r0 in range(4):
        v[r0], v[4 + r0], v[8 + r0], v[12 + r0] = _r4(v[r0], v[4 + r0], v[8 + r0], v[12 + r0])
    W = {1: c(C1, -S1), 2: c(C2, -C2), 3: c(S1, -C1), 6: c(-C2, -C2), 9: c(-C1, S1)}
    for r0 in (1, 2, 3):
        for k0 in (1, 2, 3):
            p = r0 * k0
            v[r0 + 4 * k0] = _mi(v[r0 + 4 * k0]) if p == 4 else _cmul(v[r0 + 4 * k0], W[p])
    for k0 in range(4):
        v[4 * k0], v[4 * k0 + 1], v[4 * k0 + 2], v[4 * k0 + 3] = _r4(v[4 * k0], v[4 * k0 + 1], v[4 * k0 + 2], v[4 * k0 + 3])
    return [v[4 * (q & 3) + (q >> 2)] for q in range(16)]


def tw_powers(tw, idx, running, other=None, mut=None):
    """w^r, r = 0 .. 15 (entry 0 unused) for w = tw[idx]: running products of the base (float mode) or table reads.
    mut 'entry': power 5 read one table entry off; 'base': the chain continued with `other` from r = 8"""
    base = tw[idx]
    p = [None, base]
    for r in range(2, 16):
        if running:
            p.append(_cmul(p[-1], other if (mut == "base" and r >= 8) else base))
        else:
            p.append(tw[idx * r])
    if mut == "entry":
        p[5] = tw[idx * 5 + 1]
    return p


def fft4096_emu(x, tw, running, mut=None):
    """forward FFT of x [..., 4096] (complex64: the float mode; complex128 checks the structure) as spectral.hip
    fft4096: tw complex [4096] of x's dtype"""
    j = np.arange(256)
    lead = x.shape[:-1]
    o = _dft16([x[..., 256 * r + j] for r in range(16)])                       # Ns = 1
    slot = np.stack(o, axis=-1).reshape(lead + (4096,))                         # slot 16 j + q
    v = [slot[..., 256 * r + j] for r in range(16)]
    k = j & 15
    p16 = tw_powers(tw, 16 * k, running)
    v = [v[0]] + [_cmul(v[r], p16[r]) for r in range(1, 16)]                    # Ns = 16
    o = _dft16(v)
    slot = np.empty(lead + (4096,), dtype=x.dtype)
    base = (j >> 4) * 256 + k
    for q in range(16):
        slot[..., base + 16 * q] = o[q]
    v = [slot[..., 256 * r + j] for r in range(16)]
    p256 = tw_powers(tw, j, running, other=tw[16 * k], mut=mut)
    v = [v[0]] + [_cmul(v[r], p256[r]) for r in range(1, 16)]                   # Ns = 256
    o = _dft16(v)
    return np.stack(o, axis=-2).reshape(lead + (4096,))                         # X[j + 256 q]


def _ctab(tw):
    return (tw[:, 0] + 1j * tw[:, 1]).astype(np.complex64 if tw.dtype == F else np.complex128)


def stft_emu(wav, plan, Tspec, tb, fast, mut=None):
    """the STFT kernel: float32 frames, FFT (fast: complex64 running products, else complex128 table), float32 split"""
    fr = sr.stft_frames(wav, plan, Tspec, tb.win, True)
    if fast:
        z = np.empty(fr.shape[:1] + fr.shape[2:], dtype=np.complex64)
        z.real, z.imag = fr[:, 0].astype(F), fr[:, 1].astype(F)
        Z = fft4096_emu(z, _ctab(tb.tw), True, mut)
    else:
        Z = fft4096_emu(fr[:, 0] + 1j * fr[:, 1], _ctab(tb.tw64), False, mut).astype(np.complex64)
    k = np.arange(sr.NB)
    zk, zn = Z[..., k], Z[..., (sr.NFFT - k) % sr.NFFT]
    s = F(0.5 / 64.0)
    out = np.stack([(zk.real + zn.real) * s, (zk.imag - zn.imag) * s, (zk.imag + zn.imag) * s, -(zk.real - zn.real) * s],
                   axis=-1)
    return out.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the iSTFT, emulated
def _sig32(x):
    return (F(1) / (F(1) + np.exp(-x, dtype=F))).astype(F)


def masked_spec_emu(fo, spec, mut=None):
    """float32 evaluation of the mask for one item: the 4096 FFT inputs v (conjugated packed spectrum) per frame"""
    Tspec = fo.shape[0]
    i0, i1, l0, l1 = kr.lin_index_ref(fo.shape[1], sr.NB)
    l0, l1 = l0[None, :, None], l1[None, :, None]
    xd = l0 * fo[:, i0, :] + l1 * fo[:, i1, :]
    m = _sig32(xd)
    X = []
    for c in range(2):
        mag = spec[..., c]
        ms = mag * m[..., c]
        d = mag + F(1e-8) if mut != "no_eps" else mag
        x = np.empty(mag.shape, dtype=np.complex64)
        x.real, x.imag = ms * (spec[..., 2 * c] / d), ms * (spec[..., 2 * c + 1] / d)
        x.imag[:, 0] = 0
        X.append(x)
    v = np.zeros((Tspec, sr.NFFT), dtype=np.complex64)
    zk = np.empty_like(X[0])
    zk.real, zk.imag = X[0].real - X[1].imag, X[0].imag + X[1].real
    zm = np.empty_like(X[0])
    zm.real, zm.imag = X[0].real + X[1].imag, -X[0].imag + X[1].real
    v[:, :sr.NB] = np.conj(zk)
    v[:, sr.NFFT - 1:sr.NB:-1] = np.conj(zm)[:, 1:]
    return v


def istft_emu(c, tb, split, mut=None, fast=True):
    """the fused iSTFT in float32 with the workgroup split (n, g) and the boundary join -> out [NI][2][T] float64
    (fast=False: the f32 mode's double FFT with table twiddles, its result converted to float32).
    mut: 'env3' (the envelope of block 5 from three frames), 'tail' (workgroup 0's first tail partial dropped), 'head'
    (the join reads head block h + 1), 'edge' (n <= T), 'no_eps'"""
    Tspec, T, P, NI = c["Tspec"], c["T"], c["P"], c["NI"]
    n, g = split
    tw = _ctab(tb.tw if fast else tb.tw64)
    wq = (tb.win * F(1.0 / 64.0)).astype(F)
    w2 = tb.win2
    env = ((w2[3072:] + w2[2048:3072]) + w2[1024:2048]) + w2[:1024]
    env3 = (w2[3072:] + w2[2048:3072]) + w2[1024:2048]
    out = np.zeros((NI, 2, T))
    nblk = Tspec + 6
    for it in range(NI):
        b = it // P
        v = masked_spec_emu(c["fo"][it], c["spec"][b], mut)
        y = fft4096_emu(v, tw, True) if fast else fft4096_emu(v.astype(np.complex128), tw, False).astype(np.complex64)
        yw = np.stack([y.real * wq, -y.imag * wq], axis=1).astype(F)            # [Tspec][2][4096]
        tot = np.zeros((2, nblk * 1024), dtype=F)
        head, tail = {}, {}
        for k in range(n):
            t0, t1 = k * g, min(k * g + g, Tspec)
            acc = np.zeros((2, 1024 * (t1 - t0 + 3)), dtype=F)
            for t in range(t0, t1):
                acc[:, 1024 * (t - t0):1024 * (t - t0) + 4096] += yw[t]
            for i in range(t1 - t0 + 3):
                blk, B = acc[:, 1024 * i:1024 * i + 1024], t0 + 2 + i
                if i < 3 and k > 0:
                    head[(k, i)] = blk
                elif i >= t1 - t0 and t1 < Tspec:
                    tail[(k, i - (t1 - t0))] = blk
                else:
                    tot[:, 1024 * B:1024 * B + 1024] = blk
        for k in range(1, n):
            for h in range(3):
                tl = tail[(k - 1, h)]
                if mut == "tail" and k == 1 and h == 0:
                    tl = np.zeros_like(tl)
                hd = head[(k, min(h + 1, 2) if mut == "head" else h)]
                B = 2 + g * k + h
                tot[:, 1024 * B:1024 * B + 1024] = tl + hd
        e = np.tile(env, nblk)
        if mut == "env3":
            e[1024 * 5:1024 * 6] = env3
        sl = slice(3584, 3584 + T)
        mean, std = c["tnorm"][b]
        res = tot[:, sl] / e[sl] + (c["xt2"][it].T * std + mean)
        if mut == "edge":
            res[:, T - 1] = 0
        out[it] = res
    return out


def tconv0_emu(c, bf16):
    """float32: normalise on load, fmaf chain as products and sums, erf GELU (tanh form and a bf16 store in bf16 mode)"""
    B, T, Lo = c["B"], c["T"], c["Lo"]
    p = 4 * np.arange(Lo)[:, None] - 2 + np.arange(8)[None, :]
    ok = (p >= 0) & (p < T)
    raw = c["wav"][:, :, np.where(ok, p, 0)]
    x = ((raw - c["tnorm"][:, 0][:, None, None, None]) / c["tnorm"][:, 1][:, None, None, None]) * ok.astype(F)
    x = x.transpose(0, 2, 3, 1).reshape(B, Lo, 16).astype(F)
    s = np.zeros((B, Lo, 48), dtype=F)
    for k in range(16):
        s = s + x[..., k:k + 1] * c["w"][:, k][None, None, :]
    s = s + c["bias"]
    if bf16:
        u = F(1.5957691216057308) * (s + F(0.044715) * s * s * s)
        return kr.bf16_round(s * _sig32(u))
    return (F(0.5) * s * (F(1) + np.vectorize(math.erf, otypes=[F])(s * F(0.70710678118654752440)))).astype(np.float64)
