"""Float64 restatement of the evaluation spectrogram (athd/utils.py, `athd_eval_spectrogram`), the test inputs and
the interval bound of tests/test_evalspec_refs.py and tests/test_gpu_evalspec.py; a helper module, not a test file.

Per signal (utils.py:30-95): mono = mean of the channels; periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n / 2048);
stft(n_fft = 2048, hop = 512, center = True, reflect pad 1024, one-sided); S = |X|^power; with to_db,
dB = 10 log10(max(S, 1e-10)) and the result is max(dB, max(dB) - top_db).

The bound.  Per frame den = ||frame||_2 + max_k |X64[k]| (the unwindowed reflect-padded frame of the float64 mono
signal; FFT error scales with the largest bin, which for tonal input is far above the frame norm's share per bin).
With e = tol * den, lo = max(|X64| - e, 0), hi = |X64| + e, d(m) = 10 log10(max(m^power, 1e-10)) every bin of a dB
result must lie in
    [max(d(lo), max(d(lo)) - top_db) - 1e-4,  max(d(hi), max(d(hi)) - top_db) + 1e-4]
and every bin of a to_db = False result in [lo^power, hi^power].
"""
import math

import torch
import torch.nn.functional as F

N_FFT = 2048
HOP = 512
AMIN = 1e-10
DB_SLACK = 1e-4
KINDS = ("randn", "tone", "quiet", "late")
# r = the largest |X32 - X64| / den of torch's own fp32 Hann stft against its float64 stft over the tests' inputs
# (measured on the CPU, see tests/test_evalspec_refs.py); the factor 4 is what tests/test_gpu_audio.py allows a
# different FFT factorisation
R_STFT = 1.84e-7
TOL = 4 * R_STFT


def make_input(kind: str, T: int, C: int, seed: int = 0) -> torch.Tensor:
    """(C, T) float32.
    randn: seeded noise.
    tone:  0.5 sin(2 pi 440 t / 44100) in every channel + 1e-6 randn (a range over 80 dB: most bins sit on the floor).
    quiet: 1e-7 randn with samples [T // 3, T // 3 + min(4096, T // 2)) zeroed (exercises the 1e-10 clamp).
    late:  1e-3 randn with its last 1500 samples scaled by 1000 (the maximum lies in the last frame group)."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * T + C)
    n = torch.randn(C, T, generator=g, dtype=torch.float32)
    if kind == "randn":
        return n
    if kind == "tone":
        t = torch.arange(T, dtype=torch.float64)
        s = (0.5 * torch.sin(2 * math.pi * 440.0 * t / 44100.0)).to(torch.float32)
        return s[None].expand(C, -1) + 1e-6 * n
    if kind == "quiet":
        x = 1e-7 * n
        x[:, T // 3:T // 3 + min(4096, T // 2)] = 0.0
        return x
    if kind == "late":
        x = 1e-3 * n
        x[:, -1500:] *= 1000.0
        return x
    raise ValueError(kind)


def frames(T: int) -> int:
    return 1 + T // HOP


def hann(dtype=torch.float64) -> torch.Tensor:
    n = torch.arange(N_FFT, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2 * math.pi * n / N_FFT)).to(dtype)


def mono64(wav: torch.Tensor) -> torch.Tensor:
    wav = torch.as_tensor(wav)
    if wav.dim() == 1:
        return wav.double()
    return wav.double().mean(dim=0) if wav.shape[0] > 1 else wav.double()[0]


def stft_ref(wav: torch.Tensor):
    """wav (C, T) -> (X64 (1025, frames) complex128, frame_norm (frames,) float64 = the l2 norm of each unwindowed
    2048-sample reflect-padded frame of the float64 mono signal)."""
    m = mono64(wav)
    X = torch.stft(m, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=hann(), center=True, pad_mode="reflect",
                   return_complex=True)
    padded = F.pad(m[None, None], (N_FFT // 2, N_FFT // 2), mode="reflect")[0, 0]
    fr = padded.unfold(0, N_FFT, HOP)
    assert fr.shape[0] == X.shape[1] == frames(m.shape[0])
    return X, fr.norm(dim=1)


def to_db(mag: torch.Tensor, power: float, top_db: float) -> torch.Tensor:
    """d(m) = 10 log10(max(m^power, 1e-10)) floored at its own maximum - top_db."""
    d = 10.0 * torch.log10(torch.clamp(mag ** power, min=AMIN))
    return torch.maximum(d, d.max() - top_db)


def spectrogram_ref(wav: torch.Tensor, power: float = 2.0, db: bool = True, top_db: float = 80.0):
    """(X64, frame_norm, final (1025, frames) float64)."""
    X, norm = stft_ref(wav)
    mag = X.abs()
    return X, norm, (to_db(mag, power, top_db) if db else mag ** power)


def den(X: torch.Tensor, norm: torch.Tensor) -> torch.Tensor:
    """(frames,) ||frame||_2 + max_k |X64[k]|."""
    return norm + X.abs().max(dim=0).values


def mag_interval(X: torch.Tensor, norm: torch.Tensor, tol: float):
    e = tol * den(X, norm)[None]
    mag = X.abs()
    return torch.clamp(mag - e, min=0.0), mag + e


def db_interval(X: torch.Tensor, norm: torch.Tensor, tol: float, power: float, top_db: float):
    """(low, high) of the final dB array, without the 1e-4 slack."""
    lo, hi = mag_interval(X, norm, tol)
    return to_db(lo, power, top_db), to_db(hi, power, top_db)


def check_db(got: torch.Tensor, X: torch.Tensor, norm: torch.Tensor, tol: float, power: float, top_db: float,
             wide_db: float, what: str = "") -> None:
    """Every bin inside the interval, and at most 1 % of the bins with an interval wider than `wide_db`."""
    low, high = db_interval(X, norm, tol, power, top_db)
    got = got.double()
    wide = ((high - low) > wide_db).double().mean().item()
    under = (low - DB_SLACK - got).max().item()
    over = (got - high - DB_SLACK).max().item()
    print(f"evalspec {what}: worst below {under:+.3e} dB, worst above {over:+.3e} dB (<= 0 passes), "
          f"{100 * wide:.3f} % of bins wider than {wide_db} dB")
    assert tuple(got.shape) == tuple(low.shape), what
    assert torch.all(got >= low - DB_SLACK) and torch.all(got <= high + DB_SLACK), (what, under, over)
    assert wide <= 0.01, (what, wide)


def check_power(got: torch.Tensor, X: torch.Tensor, norm: torch.Tensor, tol: float, power: float,
                what: str = "") -> None:
    """to_db = False: |X64|^power with the magnitude bound."""
    lo, hi = mag_interval(X, norm, tol)
    got = got.double()
    low, high = lo ** power, hi ** power
    scale = den(X, norm)[None] ** power + 1e-300
    print(f"evalspec {what}: worst below {((low - got) / scale).max().item():+.3e}, worst above "
          f"{((got - high) / scale).max().item():+.3e} of den^power (<= 0 passes)")
    assert tuple(got.shape) == tuple(low.shape), what
    assert torch.all(got >= low) and torch.all(got <= high), what


def stft_error_ratio(wav: torch.Tensor) -> float:
    """r of one input: the largest |X32 - X64| / den of torch's own fp32 Hann stft against its float64 stft."""
    X, norm = stft_ref(wav)
    w = torch.as_tensor(wav)
    m32 = w.float().mean(dim=0) if w.shape[0] > 1 else w.float()[0]
    X32 = torch.stft(m32, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=torch.hann_window(N_FFT),
                     center=True, pad_mode="reflect", return_complex=True)
    d = den(X, norm)[None]
    r = (X32.to(torch.complex128) - X).abs() / torch.where(d > 0, d, torch.ones_like(d))
    return r.max().item()
