"""CPU references for the audio front end (athd/app.py, csrc/audio_io.hip); a helper module, not a test file.

Resampler: torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann, lowpass_filter_width = 6,
rolloff = 0.99), restated from the published algorithm (torchaudio is not a dependency, so parity with torchaudio
itself is "restated, unpinned"):
    g = gcd, o = orig / g, n = new / g, base = min(o, n) * 0.99, w = ceil(6 o / base), taps = 2 w + o
    t[i][k] = clamp((-i / n + (k - w) / o) * base, -6, 6)                       (float64)
    K[i][k] = sinc(pi t) * cos^2(pi t / 12) * base / o, sinc(0) = 1, rounded ONCE to fp32
    y[j n + i] = sum_k xpad[j o + k] K[i][k], xpad[m] = x[m - w] (zero outside the signal), cut to ceil(n L / o)
The convolution is evaluated in float64 on the fp32 table, so the reference carries no accumulation error.

Spectrogram: app.py:74-94, torch.stft(n_fft=2048, hop_length=512) with its defaults (rectangular window,
center=True, reflect pad 1024, one-sided) on the float64 mean of the channels, 20 log10(|X| + 1e-8).
"""
import math

import torch
import torch.nn.functional as F

LOWPASS_WIDTH = 6
ROLLOFF = 0.99
N_FFT = 2048
HOP = 512


def resample_params(orig_freq: int, new_freq: int):
    """(o, n, w, taps)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * ROLLOFF
    w = math.ceil(LOWPASS_WIDTH * o / base)
    return o, n, w, 2 * w + o


def resample_length(length: int, orig_freq: int, new_freq: int) -> int:
    o, n, _, _ = resample_params(orig_freq, new_freq)
    return -((-n * length) // o)


def resample_table(orig_freq: int, new_freq: int) -> torch.Tensor:
    """The (n, taps) interpolation table: computed in float64, rounded once to fp32."""
    o, n, w, taps = resample_params(orig_freq, new_freq)
    base = min(o, n) * ROLLOFF
    idx = torch.arange(-w, w + o, dtype=torch.float64)[None, :] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx
    t = (t * base).clamp(-LOWPASS_WIDTH, LOWPASS_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_WIDTH / 2) ** 2
    tp = t * math.pi
    k = torch.where(tp == 0, torch.ones_like(tp), torch.sin(tp) / tp)
    k = k * (window * (base / o))
    assert k.shape == (n, taps)
    return k.to(torch.float32)


def live_taps(orig_freq: int, new_freq: int) -> int:
    """NT: the widest per-phase band first..last non-zero fp32 coefficient (the taps outside the Hann window's
    support underflow to exact zeros in fp32)."""
    nz = resample_table(orig_freq, new_freq) != 0
    taps = nz.shape[1]
    first = nz.to(torch.int64).argmax(dim=1)
    last = taps - 1 - nz.flip(1).to(torch.int64).argmax(dim=1)
    return int((last - first + 1).max())


def resample_ref(x: torch.Tensor, orig_freq: int, new_freq: int):
    """x (C, L) -> (y (C, L') float64, bound_sum (C, L') float64 = sum_k |xpad| |K| per output sample)."""
    x = torch.as_tensor(x)
    if orig_freq == new_freq:
        return x.double(), x.double().abs()
    o, n, w, taps = resample_params(orig_freq, new_freq)
    k = resample_table(orig_freq, new_freq).double()[:, None, :]            # (n, 1, taps)
    C, L = x.shape
    xp = F.pad(x.double(), (w, w + o))[:, None, :]                            # (C, 1, L + 2 w + o)
    out_len = resample_length(L, orig_freq, new_freq)
    y = F.conv1d(xp, k, stride=o).transpose(1, 2).reshape(C, -1)[:, :out_len]
    s = F.conv1d(xp.abs(), k.abs(), stride=o).transpose(1, 2).reshape(C, -1)[:, :out_len]
    return y, s


def spectrogram_frames(T: int) -> int:
    return 1 + T // HOP


def stft_ref(wav: torch.Tensor, dtype=torch.float64):
    """wav (C, T) -> (X (1025, frames) complex of `dtype`'s precision, frame_norm (frames,) float64 = the l2 norm of
    each 2048-sample reflect-padded frame of the float64 mean)."""
    wav = torch.as_tensor(wav)
    mono64 = wav.double().mean(dim=0) if wav.shape[0] > 1 else wav.double()[0]
    mono = mono64.to(dtype)
    X = torch.stft(mono, n_fft=N_FFT, hop_length=HOP, window=torch.ones(N_FFT, dtype=dtype), return_complex=True)
    padded = F.pad(mono64[None, None], (N_FFT // 2, N_FFT // 2), mode="reflect")[0, 0]
    frames = padded.unfold(0, N_FFT, HOP)
    assert frames.shape[0] == X.shape[1] == spectrogram_frames(wav.shape[1])
    return X, frames.norm(dim=1)


def spectrogram_db_ref(wav: torch.Tensor) -> torch.Tensor:
    """(1025, frames) float64: 20 log10(|X| + 1e-8)."""
    X, _ = stft_ref(wav)
    return 20 * torch.log10(X.abs() + 1e-8)
