"""float64 references and derived tolerances for the kernels tests/test_gpu_spectral.py reaches through
libathd_ktest.so: the STFT and the fused iSTFT (csrc/spectral.hip), the time encoder's first conv (csrc/tconv0.hip), the
prompt vectors and the two position tables (csrc/norm.hip).  The rules of tests/kernel_refs.py hold: every reference is
written from the operation's formula (the header comments of those files and the ATHTDemucs_v2.py lines they cite), is
float64, and returns (R, tol) with tol derived from

    e = 2^-24  (f32 round to nearest, relative)        e64 = 2^-53

STFT (HTDemucs._spec): demucs pad1d (reflect, zero extension first), 4096-point frames at hop 1024 starting at 1024 t in
the padded signal, periodic Hann window, scale 1/64, CaC layout {Re L, Im L, Re R, Im R} of bins 0 .. 2047, {sum, sumsq}
per batch.
* The windowed frame is the float32 product x[n] win[n] in both modes (a single multiplication of two float32 values:
  its rounding is the same on every machine), so the reference rounds it there as the kernel documents and carries no
  bound for it.  round_frame=False gives the plain float64 product that torch.stft uses (tests/test_spectral_refs.py).
* The FFT as a product of scaled unitary stages: a relative normwise error u_s in stage s adds up to first order,
  |dZ|_2 <= c u |Z|_2 with c the sum over stages, and |dZ_k| <= |dZ|_2 for every bin.  Stages of fft4096: three 16-point
  DFTs of two radix-4 layers (two additions deep: 2 each) and the fixed W16 products (sqrt 5 for a complex product,
  Brent et al., + 1 for the rounded constant); two twiddle passes (sqrt 5 + the twiddle's own error); one more for the
  last rounding.  A table twiddle is a rounded value: 1.  A running product w^r of the rounded base carries r times the
  base's error and (r - 1) complex-product roundings: d_r = r + (r - 1) sqrt 5, at most d_15 = 46.3 (in units of e
  relative to |w| = 1, i.e. up to 47 float32 ulps of a component near 0.5: not "<= 15 ulp").  So
      c_table = 3 (4 + sqrt 5 + 1) + 2 (sqrt 5 + 1) + 1 = 29.2        c_run = c_table + 2 (d_15 - 1) = 119.8
  With |Z|_2 = 64 |frame|_2 and the output (Z_k +- Z_-k) / 128, |d out| <= c u |frame|_2.
* f32 mode (double FFT, table twiddles): Z_k and Z_-k are rounded to float32 (e |Z| each), their sum rounds once more
  (e |R|, the scale is a power of two), and the double FFT adds c_table e64 |frame|_2:
      tol = e (|Z_k| + |Z_-k|) / 128 + e |R| + c_table e64 |frame|_2.
  That is two to three roundings, not the one of a correctly rounded spectrum.
* bf16 mode (float FFT, running-product twiddles), two criteria:
    elementwise   |got - R| <= c_run e |frame|_2 + e |R|      (worst case: about 1e3 times the real error)
    per frame     |got - R|_2 / |R|_2 <= 4 R32 + C_TW
  R32 is the same ratio for torch.stft in float32 against float64 on the same inputs (measured and asserted in
  tests/test_spectral_refs.py); the factor 4 is the one tests/test_gpu_audio.py and tests/test_gpu_evalspec.py use for
  that comparison.  C_TW is the rms contribution of the running products: in each twiddle pass register r of every thread
  is multiplied by w^r known to d_r e; after the first 16-point DFT the energy of a noise frame is spread evenly over
  r = 0 .. 15 (d_0 = 0), the two passes are independent, so
      C_TW = e sqrt(2 mean_r d_r^2) = 37.6 e = 2.24e-6.
  (An impulse can put all its energy on one r: the criterion is for noise inputs, which is what the tests use.)
* {sum, sumsq}: the statistics rule of kernel_refs.py on the stored values; every partial sum is fp64, so only the n64
  term applies (32 additions per thread, 6 + 4 across the workgroup, Tspec atomics).

iSTFT (ATHTDemucs_v2.py:297-324 and HTDemucs._ispec): the Tspec decoder rows are resized to 2048 bins with
kernel_refs.lin_index_ref (the kernel's float32 weights bit for bit), sigmoid, the mask formula with Re L and Im L as the
"magnitude" (the reference's own quirk), DC imaginary part and Nyquist bin zeroed, inverse transform with the 1/64
"normalized" scale, window, overlap-add, division by the window envelope of all Tspec + 4 frames, slice at 3584, plus
xt2 std + mean.
* Per bin: 3e (l0 |a| + l1 |b|) for the lerp; the sigmoid's slope is at most 1/4 and its own evaluation adds 4e m, or in
  fast mode m ((1 - m)(|x| + 4) + 4) e (the `fast` term of kernel_refs.py); the mask product, the + 1e-8, the division
  and the last product add 4e |X| (fast: v_rcp is 2e and costs one more product: 6e |X|); packing the two channels adds
  sqrt 2 e (|X_L| + |X_R|).  With |Re L|, |Im L| >= 0.25 the + 1e-8 is below half a float32 ulp: the kernel's
  denominator is Re L itself, 4e-8 relative from the reference's, inside the e counted for that addition.
* A bin error d_k reaches every sample of its frame through the transform: (2 / 64) sum_k d_k (the bin and its mirror),
  plus the FFT's own c u |Z|_2 (c_run e, or c_table e64 in f32 mode, |Z|_2 over the 4096 packed bins).
* Each frame sample is converted and multiplied by win / 64 (2e), up to four are added (3e of the sum of magnitudes, the
  boundary join included), the envelope is known to 5e (win2's rounding, three additions, the division; fast: v_rcp and
  a product instead, 7e), and the time branch adds 3e (|xt2 std| + |mean| + |r|).
* Fast mode also: per hop block of 1024 output samples, |got - R|_2 / |R_freq|_2 <= 4 R32I + C_TW, R32I the same ratio
  for torch.istft in float32 against float64 on the reference's masked spectrum.

tconv0: Conv1d(2, 48, 8, stride 4, padding 2) on (wav - sub) / dv, taps outside [0, T) read zero AFTER the normalisation,
GELU (erf form; bf16 mode: the tanh form, kernel_refs.gelu_tanh_step).  tol = (16 + 4) e sum |w| |x| through the GELU
step, + hulp16 for a bf16 store.

text_vec: a = Ma t + ma, c0 = Mc t + mc, c2 = a + b2; tol = (128 + 8) e sum |M| |t| (a quarter of K per wave, the joins,
the bias; the magnitudes include the biases).

Position tables (oracle/htdemucs_ref.py create_2d_sin_embedding / create_sin_embedding): float64 with float32 roundings
where pos2d_kernel / pos1d_kernel have a single exactly reproducible float32 operation (the constant k, the product
cc k, the exponent a / (half - 1)).  expf, powf, sinf and cosf are documented to 1 ulp (2e relative), the product or
quotient that forms the phase rounds once: the phase is known to 3e |ph|, sin and cos have slope <= 1, and their own
ulp is at most 2e of a value <= 1:  tol = (3 |ph| + 2) e.  exact=True is the plain float64 formula (the oracle's).
"""
import math
from types import SimpleNamespace

import numpy as np

import kernel_refs as kr

E32 = kr.E32
E64 = 2.0 ** -53
NFFT, HOP, NB = 4096, 1024, 2048
SQ5 = math.sqrt(5.0)


def tw_err(r):
    """error of the running product w^r in units of e (module docstring); 1 for r = 0 would be the table's"""
    return 0.0 if r == 0 else r + (r - 1) * SQ5


C_TABLE = 3 * (4 + SQ5 + 1) + 2 * (SQ5 + 1) + 1
C_RUN = C_TABLE + 2 * (tw_err(15) - 1)
C_TW = E32 * math.sqrt(2.0 * sum(tw_err(r) ** 2 for r in range(16)) / 16.0)
# |x32 - x64|_2 / |x64|_2 of torch.stft / torch.istft in float32 on the inputs of tests/test_spectral_refs.py (measured
# there: 1.29e-7 and 1.50e-7; asserted to lie in (R / 2, R]: the margin is for another host's FFT library)
R32 = 2.0e-7
R32I = 2.0e-7
L2_STFT = 4 * R32 + C_TW
L2_ISTFT = 4 * R32I + C_TW


def tables():
    """the tables of athd_api.cpp: tw / tw64 [4096][2], win = float32 of the double periodic Hann, win2 = win * win"""
    k = np.arange(NFFT, dtype=np.float64)
    a = -2.0 * np.pi * k / NFFT
    tw64 = np.stack([np.cos(a), np.sin(a)], axis=-1)
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * k / NFFT)).astype(np.float32)
    return SimpleNamespace(tw=tw64.astype(np.float32), tw64=tw64, win=win, win2=(win * win).astype(np.float32))


# ------------------------------------------------------------------------------------------------ pad1d
def pad_plan_ref(T, Tspec=None):
    """(L, left, ext_left, Lx) of HTDemucs._spec's pad1d(x, (1536, 1536 + 1024 le - T), 'reflect'), le = ceil(T / 1024)"""
    le = -(-T // HOP) if Tspec is None else Tspec
    pl, pr = 1536, 1536 + le * HOP - T
    mx = max(pl, pr)
    el = er = 0
    if T <= mx:
        extra = mx - T + 1
        er = min(pr, extra)
        el = extra - er
    return (T, pl - el, el, T + el + er)


def pad_index(plan, p, mut=None):
    """padded positions p (any integers) -> (source index, valid): the zero extension, then one reflection on either
    side.  mut 'reflect': the right reflection as 2 Lx - 1 - i (the edge sample repeated)"""
    L, left, el, Lx = plan
    i = np.abs(np.asarray(p, dtype=np.int64) - left)
    i = np.where(i >= Lx, (2 * Lx - 1 if mut == "reflect" else 2 * (Lx - 1)) - i, i) - el
    ok = (i >= 0) & (i < L)
    return np.where(ok, i, 0), ok


def pad1d_ref(x, plan, p, mut=None):
    """x [..., T] -> the padded signal at positions p, float64"""
    idx, ok = pad_index(plan, p, mut)
    return np.asarray(x, dtype=np.float64)[..., idx] * ok


# ------------------------------------------------------------------------------------------------ STFT
def stft_frames(wav, plan, Tspec, win, round_frame=True, mut=None):
    """windowed frames [nb][2][Tspec][4096] float64 (round_frame: each the float32 product the kernel forms)"""
    off = -HOP if mut == "frame" else 0          # mut 'frame': stft frame t + 1 for t + 2 (one hop early)
    idx = off + HOP * np.arange(Tspec)[:, None] + np.arange(NFFT)[None, :]
    xf = pad1d_ref(wav, plan, idx, mut)
    w = np.roll(win, 1) if mut == "window" else win          # mut 'window': the window one sample late
    if round_frame:
        return (xf.astype(np.float32) * w.astype(np.float32)).astype(np.float64)
    return xf * w.astype(np.float64)


def stft_ref(wav, plan, Tspec, win, fast, round_frame=True, mut=None):
    """wav [nb][2][T] -> SimpleNamespace(R [nb][Tspec][2048][4], tol, fn [nb][Tspec] (|frame|_2), stats [nb][2],
    stats_tol).  fast: the bf16 mode's float FFT (elementwise bound; the L2 criterion is L2_STFT)."""
    fr = stft_frames(wav, plan, Tspec, win, round_frame, mut)
    z = fr[:, 0] + 1j * fr[:, 1]
    Z = np.fft.fft(z, axis=-1)
    k = np.arange(NB)
    Zk, Zn = Z[..., k], Z[..., (NFFT - k) % NFFT]
    XL, XR = (Zk + np.conj(Zn)) / 128.0, (Zk - np.conj(Zn)) / 128.0j
    if mut == "im_sign":
        XL, XR = np.conj(XL), np.conj(XR)
    R = np.stack([XL.real, XL.imag, XR.real, XR.imag], axis=-1)
    fn = np.sqrt((np.abs(z) ** 2).sum(axis=-1))
    if fast:
        tol = (C_RUN * E32 * fn)[..., None, None] + E32 * np.abs(R)
    else:
        tol = (E32 * (np.abs(Zk) + np.abs(Zn)) / 128.0)[..., None] + E32 * np.abs(R) + (C_TABLE * E64 * fn)[..., None, None]
    st, st_tol = kr.stats_of(R, tol, n_part=0, n64=42 + Tspec)
    return SimpleNamespace(R=R, tol=tol, fn=fn, stats=st, stats_tol=st_tol)


def l2_ratio(got, R, axes):
    """|got - R|_2 / |R|_2 over `axes`"""
    num = np.sqrt(((got - R) ** 2).sum(axis=axes))
    return num / np.maximum(np.sqrt((R ** 2).sum(axis=axes)), 1e-300)


# ------------------------------------------------------------------------------------------------ iSTFT
def masked_spec_ref(fo, spec, fast, mut=None):
    """fo [Tspec][rows][2] (one item), spec [Tspec][2048][4] (its segment) -> (P, d): the Hermitian-packed 4096-bin
    spectrum P = S_L + i S_R per frame [Tspec][4096] and the per-bin error bound d [Tspec][2048] of its first half.
    mut 'l_swap': the lerp weights exchanged; 'nyquist': bin 2048 filled like bin 2047; 'dc_imag': kept."""
    fo, spec = np.asarray(fo, dtype=np.float64), np.asarray(spec, dtype=np.float64)
    i0, i1, l0, l1 = kr.lin_index_ref(fo.shape[1], NB)
    l0, l1 = l0.astype(np.float64)[None, :, None], l1.astype(np.float64)[None, :, None]
    if mut == "l_swap":
        l0, l1 = l1, l0
    a, b = fo[:, i0, :], fo[:, i1, :]
    xd = l0 * a + l1 * b
    dxd = 3 * E32 * (l0 * np.abs(a) + l1 * np.abs(b))
    m = kr.sigmoid(xd)
    dm = dxd / 4 + (m * ((1 - m) * (np.abs(xd) + 4) + 4) * E32 if fast else 4 * E32 * m)
    X, dX = [], []
    for c in range(2):
        mag = spec[..., c]
        zc = spec[..., 2 * c] + 1j * spec[..., 2 * c + 1]
        x = (mag * m[..., c]) * (zc / (mag + 1e-8))
        X.append(x)
        dX.append(np.abs(x) * (dm[..., c] / m[..., c] + (6 if fast else 4) * E32))
    if mut != "dc_imag":
        for x in X:
            x[:, 0] = x[:, 0].real
    d = dX[0] + dX[1] + math.sqrt(2.0) * E32 * (np.abs(X[0]) + np.abs(X[1]))
    P = np.zeros((fo.shape[0], NFFT), dtype=np.complex128)
    P[:, :NB] = X[0] + 1j * X[1]
    P[:, NFFT - 1:NB:-1] = (np.conj(X[0]) + 1j * np.conj(X[1]))[:, 1:]
    if mut == "nyquist":
        P[:, NB] = P[:, NB - 1]
    return P, d


def envelope_ref(win):
    """the interior envelope of torch.istft at offset q mod 1024: the four overlapping win^2 (float64 of float32 win)"""
    w2 = win.astype(np.float64) ** 2
    return w2.reshape(4, HOP).sum(axis=0)


def istft_ref(fo, spec, xt2, tnorm, P, T, win, fast, mut=None):
    """fo [NI][Tspec][rows][2], spec [NI/P][Tspec][2048][4], xt2 [NI][T][2], tnorm [NI/P][2] {mean, std} ->
    SimpleNamespace(R [NI][2][T], tol, Rf (the frequency branch alone), Pk (packed spectra of item 0))"""
    NI, Tspec = fo.shape[0], fo.shape[1]
    w = win.astype(np.float64)
    env = np.tile(envelope_ref(win), Tspec + 6)
    Q = HOP * (Tspec + 6)
    R, Rf, tol, Pk0 = np.zeros((NI, 2, T)), np.zeros((NI, 2, T)), np.zeros((NI, 2, T)), None
    cu = C_RUN * E32 if fast else C_TABLE * E64
    for it in range(NI):
        b = it // P
        Pk, d = masked_spec_ref(fo[it], spec[b], fast, mut)
        if it == 0:
            Pk0 = Pk
        y = np.fft.ifft(Pk, axis=-1) * 64.0                               # [Tspec][4096]: L = Re, R = Im
        ft = (2.0 / 64.0) * d.sum(axis=-1) + cu * np.sqrt((np.abs(Pk) ** 2).sum(axis=-1))     # per frame
        acc, A, Tl = np.zeros((2, Q)), np.zeros((2, Q)), np.zeros(Q)
        for t in range(Tspec):
            q0 = HOP * (t + 2)
            yw = np.stack([y[t].real, y[t].imag]) * w
            acc[:, q0:q0 + NFFT] += yw
            A[:, q0:q0 + NFFT] += np.abs(yw)
            Tl[q0:q0 + NFFT] += ft[t] * w
        sl = slice(3584, 3584 + T)
        r = acc[:, sl] / env[sl]
        mean, std = float(tnorm[b, 0]), float(tnorm[b, 1])
        xs = np.asarray(xt2[it], dtype=np.float64).T * std
        Rf[it] = r
        R[it] = r + (xs + mean)
        tol[it] = ((Tl[sl] + 5 * E32 * A[:, sl]) / env[sl] + (7 if fast else 5) * E32 * np.abs(r) +
                   3 * E32 * (np.abs(xs) + abs(mean) + np.abs(r)))
    return SimpleNamespace(R=R, tol=tol, Rf=Rf, Pk=Pk0)


def block_l2(got, R, Rf, T):
    """per (item, hop block) |got - R|_2 / |Rf|_2 over both channels: [NI][blocks]"""
    nb = -(-(T + 3584) // HOP) - 3
    out = np.zeros((got.shape[0], nb))
    B = (np.arange(T) + 3584) // HOP - 3
    for i in range(nb):
        s = B == i
        num = np.sqrt(((got[:, :, s] - R[:, :, s]) ** 2).sum(axis=(1, 2)))
        out[:, i] = num / np.maximum(np.sqrt((Rf[:, :, s] ** 2).sum(axis=(1, 2))), 1e-300)
    return out


def ola_split_ref(Tspec):
    """the frame split of spectral.hip istft_ola_split, transcribed: (workgroups n, frames per workgroup g)"""
    n = (Tspec + 31) // 32
    while True:
        g = (Tspec + n - 1) // n
        if n == 1 or (g >= 3 and Tspec - (n - 1) * g >= 3) or g < 3:
            return n, g
        n += 1


# ------------------------------------------------------------------------------------------------ tconv0
def tconv0_ref(wav, tnorm, w, bias, bf16, mut=None):
    """wav [B][2][T], tnorm [B][2] {sub, div}, w [48][tap * 2 + c], bias [48] -> (R [B][Lo][48], tol), Lo = ceil(T / 4).
    mut 'pad_sub': the taps outside [0, T) read (0 - sub) / dv"""
    wav = np.asarray(wav, dtype=np.float64)
    B, _, T = wav.shape
    Lo = -(-T // 4)
    sub, dv = np.asarray(tnorm, dtype=np.float64)[:, 0], np.asarray(tnorm, dtype=np.float64)[:, 1]
    p = 4 * np.arange(Lo)[:, None] - 2 + np.arange(8)[None, :]
    ok = (p >= 0) & (p < T)
    raw = wav[:, :, np.where(ok, p, 0)] * ok                          # [B][2][Lo][8]
    x = (raw - sub[:, None, None, None]) / dv[:, None, None, None]
    if mut != "pad_sub":
        x = x * ok
    x = x.transpose(0, 2, 3, 1).reshape(B, Lo, 16)                     # k = tap * 2 + c
    w, bias = np.asarray(w, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    acc = x @ w.T + bias
    t = 20 * E32 * (np.abs(x) @ np.abs(w).T + np.abs(bias))
    if bf16:
        R, t = kr.gelu_tanh_step(acc, t)
        return R, t + kr.hulp16(np.abs(R) + t)
    return kr.gelu_step(acc, t, False)


# ------------------------------------------------------------------------------------------------ text_vec
def text_vec_ref(text, NI, P, per_item, maT, ma, mcT, mc, b2):
    """text [rows][512]; maT, mcT [512][384] -> ((a, c0, c2) [NI][384] each, (ta, tc0, tc2))"""
    src = np.arange(NI) if per_item else np.arange(NI) % P
    t = np.asarray(text, dtype=np.float64)[src]
    f = lambda v: np.asarray(v, dtype=np.float64)
    a, c0 = t @ f(maT) + f(ma), t @ f(mcT) + f(mc)
    ta = 136 * E32 * (np.abs(t) @ np.abs(f(maT)) + np.abs(f(ma)))
    tc0 = 136 * E32 * (np.abs(t) @ np.abs(f(mcT)) + np.abs(f(mc)))
    return (a, c0, a + f(b2)), (ta, tc0, ta + E32 * (np.abs(a) + np.abs(f(b2))))


# ------------------------------------------------------------------------------------------------ position tables
def pos2d_ref(Fr, T1, C, exact=False):
    """[(f T1 + t)][C]: channels < C / 2 carry the time axis, the rest the frequency axis; even: sin, odd: cos"""
    half = C // 2
    c = np.arange(C)
    cc = np.where(c < half, c, c - half)
    ev = (cc & ~1).astype(np.float64)
    if exact:
        div = np.exp(ev * -(math.log(10000.0) / half))
    else:
        k = np.float32(-(math.log(10000.0) / half))
        div = np.exp((ev.astype(np.float32) * k).astype(np.float64))
    f, t = np.divmod(np.arange(Fr * T1), T1)
    pos = np.where(c[None, :] < half, t[:, None], f[:, None]).astype(np.float64)
    ph = pos * div[None, :]
    R = np.where((cc & 1)[None, :] == 1, np.cos(ph), np.sin(ph))
    return R, (3 * np.abs(ph) + 2) * E32


def pos1d_ref(T2, C, exact=False):
    """[t][C]: cos(t / 10000^(a / (half - 1))) for c = a < half, sin for c = half + a"""
    half = C // 2
    c = np.arange(C)
    a = np.where(c < half, c, c - half)
    if exact:
        ex = a / (half - 1.0)
    else:
        ex = (a.astype(np.float32) / np.float32(half - 1)).astype(np.float64)
    ph = np.arange(T2, dtype=np.float64)[:, None] / (10000.0 ** ex)[None, :]
    R = np.where(c[None, :] < half, np.cos(ph), np.sin(ph))
    return R, (3 * np.abs(ph) + 2) * E32
