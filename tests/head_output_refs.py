"""References for head training's native output stage (csrc/head_grad.hip, include/athd.h `athd_head_output*`); a helper
module of tests/test_head_output_refs.py and tests/test_gpu_head_output.py, not a test file.

  * `case`: the inputs of `spectral_cases.istft_case` (|Re z_0|, |Im z_0| >= 0.25, so the signed `m + 1e-8` division is
    well conditioned) in the head's layouts, plus a seeded incoming gradient;
  * `torch_stage`: the output stage as the torch ops of `TrainableHead.forward` / `_ispec`, for autograd in any dtype;
  * `autograd`: (dL/dxd, dL/dxtd) of `sum(out * g)` through `torch_stage`;
  * `closed_form`: the adjoint written out (an STFT of g / envelope, the mask derivative, the transposed resize) in numpy,
    in float64 or in float32 in the kernel's order of operations (both channels packed into one complex FFT emulated by
    `spectral_cases.fft4096_emu`, the Hermitian split).  `mut` plants the defects the tests' bound must separate;
  * `item_gap`: the worst |got - want| per item over that item's largest |want|.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import kernel_refs as kr
import spectral_cases as sc
import spectral_refs as sr

N, HOP, NB = 4096, 1024, 2048
# (Ts, T, B) of the GPU kernel tests: one frame (every bin maps to row 0: the resize transpose sums 2048 terms); two
# frames; T a multiple of the hop; the forward's first two-workgroup split with an odd T (channel 1 of g misaligned);
# three forward workgroups and more rows than a wave
CASES = [(1, 1000, 1), (2, 1500, 1), (3, 3072, 2), (33, 33297, 2), (65, 66000, 2)]
ALLOW = 4.0          # a float32 evaluation may sit at this many times the reference's own f32-against-f64 gap


def case(Ts, T, B, seed=0):
    """dict of torch float64 CPU tensors: xd (B, 2, Ts, Ts) [channel][row][frame], xtd (B, 2, T), z (B, 2, 2048, Ts)
    complex128, meant / stdt (B, 1, 1), g (B, 2, T); every value is float32-representable"""
    assert Ts == -(-T // HOP)
    c = sc.istft_case(Ts, T, B, 1, seed)
    spec = c["spec"].astype(np.float64)                                    # [B][t][kb][4]
    z = np.stack([spec[..., 0] + 1j * spec[..., 1], spec[..., 2] + 1j * spec[..., 3]], axis=1).transpose(0, 1, 3, 2)
    g = np.random.default_rng(5000 + seed).standard_normal((B, 2, T)).astype(np.float32)
    g *= np.ldexp(1.0, np.arange(B) % 2)[:, None, None].astype(np.float32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
    return dict(Ts=Ts, T=T, B=B, xd=t(c["fo"].transpose(0, 3, 2, 1)), xtd=t(c["xt2"].transpose(0, 2, 1)),
                z=torch.as_tensor(np.ascontiguousarray(z)), meant=t(c["tnorm"][:, 0].reshape(B, 1, 1)),
                stdt=t(c["tnorm"][:, 1].reshape(B, 1, 1)), g=t(g))


def torch_stage(xd, xtd, z, meant, stdt, length):
    """`TrainableHead.forward` from the mask on, with `_ispec` written in (athd/head.py), in the dtype of its inputs"""
    mask = torch.sigmoid(F.interpolate(xd, size=(z.shape[2], z.shape[3]), mode="bilinear", align_corners=False))
    mag_stereo = torch.stack((z[:, 0].real, z[:, 0].imag), dim=1)
    phase = z / (mag_stereo + 1e-8)
    zz = (mag_stereo * mask) * phase
    B, C, Fr, Ts = zz.shape
    zz = F.pad(F.pad(zz, (0, 0, 0, 1)), (2, 2))
    pad = HOP // 2 * 3
    le = HOP * int(math.ceil(length / HOP)) + 2 * pad
    win = torch.hann_window(N).to(dtype=zz.real.dtype)
    x = torch.istft(zz.reshape(B * C, Fr + 1, Ts + 4), N, HOP, window=win, win_length=N, normalized=True, length=le,
                    center=True)
    freq_wav = x.reshape(B, C, le)[..., pad:pad + length]
    if xtd.shape[-1] != length:
        xtd = F.interpolate(xtd, size=length, mode="linear", align_corners=False)
    return freq_wav + (xtd * stdt + meant)


def autograd(c, dtype, xtd=None):
    """(dL/dxd, dL/dxtd) as float64 numpy for L = sum(out * g), by torch autograd in `dtype` on the CPU"""
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    xd = c["xd"].detach().to(dtype).clone().requires_grad_(True)
    xt = (c["xtd"] if xtd is None else xtd).detach().to(dtype).clone().requires_grad_(True)
    out = torch_stage(xd, xt, c["z"].to(cd), c["meant"].to(dtype), c["stdt"].to(dtype), c["T"])
    out.backward(c["g"].to(dtype))
    return xd.grad.double().numpy(), xt.grad.double().numpy()


def lin_index64(in_size, out_size):
    """the linear resize's (i0, i1, l0, l1) in float64, as ATen computes them for a float64 tensor (align_corners=False)"""
    d = np.arange(out_size)
    if in_size == out_size:
        return d.copy(), d.copy(), np.ones(out_size), np.zeros(out_size)
    src = np.maximum((in_size / out_size) * (d + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    lam = np.clip(src - i0, 0.0, 1.0)
    return i0, i0 + (i0 < in_size - 1), 1.0 - lam, lam


def closed_form(c, f32=False, mut=None):
    """dL/dxd (B, 2, Ts, Ts) and dL/dxtd (B, 2, T) by the closed form of include/athd.h, float64 numpy arrays.
    f32: every operation in float32 in the kernel's order.  mut: 'c1' (c_kb = 1 on the interior bins), 'dc_imag' (the
    packed transform's DC bin is not split, so it keeps an imaginary part)"""
    R = np.float32 if f32 else np.float64
    C = np.complex64 if f32 else np.complex128
    Ts, T, B = c["Ts"], c["T"], c["B"]
    win = torch.hann_window(N).numpy().astype(R)                   # built in float32 and cast, as `_ispec` does
    win2 = win * win
    env = ((win2[3072:] + win2[2048:3072]) + win2[1024:2048]) + win2[:1024]
    wq = win * R(1.0 / 64.0)
    g, xd = c["g"].numpy().astype(R), c["xd"].numpy().astype(R)
    z = c["z"].numpy()
    i0, i1, l0, l1 = kr.lin_index_ref(Ts, NB) if f32 else lin_index64(Ts, NB)
    tw = sr.tables().tw
    twc = (tw[:, 0] + 1j * tw[:, 1]).astype(np.complex64)
    k = np.arange(NB)
    out = np.zeros((B, 2, Ts, Ts))
    for b in range(B):
        u = np.zeros((2, (Ts + 5) * HOP), dtype=R)
        u[:, 3584:3584 + T] = g[b]
        u = (u.reshape(2, -1, HOP) / env).reshape(2, -1)
        fr = np.stack([u[:, HOP * (t + 2):HOP * (t + 2) + N] * wq for t in range(Ts)])        # [t][c][m]
        zp = np.empty((Ts, N), dtype=C)
        zp.real, zp.imag = fr[:, 0], fr[:, 1]
        Z = sc.fft4096_emu(zp, twc, True) if f32 else np.fft.fft(zp, axis=-1)
        zk, zn = Z[:, k], Z[:, (N - k) % N]
        s = np.where(k == 0, 0.5, 1.0 if mut != "c1" else 0.5).astype(R)
        G = [((zk.real + zn.real) * s, (zk.imag - zn.imag) * s), ((zk.imag + zn.imag) * s, -(zk.real - zn.real) * s)]
        if mut == "dc_imag":
            G[0][1][:, 0], G[1][1][:, 0] = zk.imag[:, 0], -zk.real[:, 0]
        for ch in range(2):
            m = (z[b, 0].real if ch == 0 else z[b, 0].imag).T.astype(R)                   # [t][kb]
            d = m + R(1e-8)
            ph_re, ph_im = z[b, ch].real.T.astype(R) / d, z[b, ch].imag.T.astype(R) / d
            dmask = m * (G[ch][0] * ph_re + G[ch][1] * ph_im)
            rows = xd[b, ch].T                                                            # [t][row]
            x = l0 * rows[:, i0] + l1 * rows[:, i1]
            mask = R(1) / (R(1) + np.exp(-x, dtype=R))
            dup = dmask * (mask * (R(1) - mask))
            acc = np.zeros((Ts, Ts), dtype=R)                                             # [t][row]
            for kb in range(NB):                                                          # ascending kb, as the kernel
                if i0[kb] == i1[kb]:
                    acc[:, i0[kb]] += (l0[kb] + l1[kb]) * dup[:, kb]
                else:
                    acc[:, i0[kb]] += l0[kb] * dup[:, kb]
                    acc[:, i1[kb]] += l1[kb] * dup[:, kb]
            out[b, ch] = acc.T
    return out, (c["g"] * c["stdt"]).numpy()


@functools.lru_cache(maxsize=None)
def refs(shape):
    """(case, float64 autograd (dxd, dxt), a per item) of a (Ts, T, B) shape, computed once and shared by the tests; `a`
    is the reference's own noise: torch's float32 autograd against its float64 autograd, per item over the item's
    largest |gradient|.  Treat the arrays as read-only."""
    c = case(*shape)
    g64 = autograd(c, torch.float64)
    g32 = autograd(c, torch.float32)
    return c, g64, item_gap(g32[0], g64[0])


def item_gap(got, want):
    """[per item] max |got - want| / max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    B = want.shape[0]
    return [float(np.abs(got[b] - want[b]).max() / np.abs(want[b]).max()) for b in range(B)]
