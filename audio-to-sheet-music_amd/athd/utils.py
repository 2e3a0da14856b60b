"""`utils.py` twin for the functions that compute numbers: the evaluation spectrograms of `benchmark.py
--plot-spectrograms` and `generate_spectrogram.py`, on the device (`athd_eval_spectrogram`, csrc/audio_io.hip).

Mirrors, name for name:
  * `compute_spectrogram`       <- `utils.py:30-79` with `amplitude_to_db` (`:82-95`) folded in: periodic Hann window,
                                   n_fft 2048, hop 512, |X|^power, 10 log10(max(., 1e-10)), floor at max - top_db.
  * `compute_spectrograms`      the same for N equal-shaped signals in one call, with each array's (min, max).
  * `separation_spectrograms`   <- the data of `plot_separation_spectrograms` (`:220-264`): three panels and the shared
                                   colour range of `plot_spectrogram_comparison` (`:184-188`).
  * `all_stems_spectrograms`    <- the data of `plot_all_stems_spectrograms` (`:267-356`).
No figure is drawn (DESIGN.md §7 keeps UI out): the functions return the arrays, `vmin` / `vmax` and `extent` a
figure would be drawn from.  `amplitude_to_db` on an arbitrary tensor is not offered separately; only the STFT sizes
of the reference's callers (2048 / 512) are built.  The reference runs this on the CPU per spectrogram; there is no
CPU path here.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple, Union

import torch

from . import native

N_FFT = 2048
HOP_LENGTH = 512
N_BINS = N_FFT // 2 + 1


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _check_args(n_fft: int, hop_length: int, power: float, top_db: float) -> None:
    if n_fft != N_FFT or hop_length != HOP_LENGTH:
        raise ValueError(f"only n_fft = {N_FFT}, hop_length = {HOP_LENGTH} are built (the reference's callers use "
                         f"no other), got {n_fft} / {hop_length}")
    if float(power) not in (1.0, 2.0):
        raise ValueError(f"power must be 1.0 or 2.0, got {power}")
    if not float(top_db) >= 0.0:
        raise ValueError(f"top_db must be non-negative, got {top_db}")


def compute_spectrograms(waveforms: Union[torch.Tensor, Sequence[torch.Tensor]], n_fft: int = N_FFT,
                         hop_length: int = HOP_LENGTH, power: float = 2.0, to_db: bool = True,
                         top_db: float = 80.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(N, C, T) or a sequence of N equal-shaped (C, T) tensors -> (specs (N, 1025, 1 + T // 512), ranges (N, 2) =
    each array's (min, max)), float32 on the device, in one call.  Each array equals `compute_spectrogram` of its
    signal bit for bit."""
    _check_args(n_fft, hop_length, power, top_db)
    if not isinstance(waveforms, torch.Tensor):
        waveforms = list(waveforms)
        if not waveforms or any(w.dim() != 2 or w.shape != waveforms[0].shape for w in waveforms):
            raise ValueError("expected a non-empty sequence of equal-shaped (C, T) waveforms")
        dev = next((w.device for w in waveforms if w.device.type == "cuda"), torch.device("cuda"))
        waveforms = torch.stack([w.to(dev).float() for w in waveforms])
    if waveforms.dim() != 3 or waveforms.shape[0] == 0 or waveforms.shape[1] == 0:
        raise ValueError(f"expected (N, C, T) waveforms, got {tuple(waveforms.shape)}")
    x = waveforms.float()
    if x.device.type != "cuda":
        x = x.cuda()
    x = x.contiguous()
    N, C, T = x.shape
    if T <= N_FFT // 2:
        raise ValueError(f"the spectrogram's reflect padding needs more than {N_FFT // 2} samples, got {T}")
    frames = int(native.lib.athd_spectrogram_frames(T))
    specs = torch.empty((N, N_BINS, frames), dtype=torch.float32, device=x.device)
    ranges = torch.empty((N, 2), dtype=torch.float32, device=x.device)
    need = int(native.lib.athd_eval_spectrogram_scratch_bytes(N))
    scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    rc = native.lib.athd_eval_spectrogram(x.data_ptr(), N, C, T, C * T, float(power), int(bool(to_db)), float(top_db),
                                          specs.data_ptr(), ranges.data_ptr(), scratch.data_ptr(), need,
                                          _stream(x.device))
    if rc != 0:
        raise native.AthdError(f"athd_eval_spectrogram failed ({rc})")
    return specs, ranges


def compute_spectrogram(waveform: torch.Tensor, n_fft: int = N_FFT, hop_length: int = HOP_LENGTH, power: float = 2.0,
                        to_db: bool = True, top_db: float = 80.0) -> torch.Tensor:
    """`utils.py:30-79`: (C, T) or (T,) -> (1025, 1 + T // 512) float32 device tensor.  A CPU tensor is moved to the
    device."""
    if waveform.dim() == 1:
        waveform = waveform[None]
    if waveform.dim() != 2:
        raise ValueError(f"expected a (C, T) or (T,) waveform, got {tuple(waveform.shape)}")
    return compute_spectrograms(waveform[None], n_fft, hop_length, power, to_db, top_db)[0][0]


def _spectrograms_of(waveforms: Sequence[torch.Tensor]) -> Tuple[List[torch.Tensor], float, float]:
    """The default dB spectrogram of every (C, T) waveform and the global (min, max): one call per distinct shape
    (one call in all when the lengths agree, as they do for the stems of a track)."""
    specs: List = [None] * len(waveforms)
    groups: Dict[tuple, List[int]] = {}
    for i, w in enumerate(waveforms):
        groups.setdefault(tuple(w.shape), []).append(i)
    lows, highs = [], []
    for idx in groups.values():
        out, ranges = compute_spectrograms([waveforms[i] for i in idx])
        for j, i in enumerate(idx):
            specs[i] = out[j]
        lows.append(ranges[:, 0].min())
        highs.append(ranges[:, 1].max())
    return specs, float(torch.stack(lows).min().item()), float(torch.stack(highs).max().item())


def _extent(frames: int, sample_rate: int) -> List[float]:
    """`imshow`'s extent of `utils.py:193-202`: seconds and kHz."""
    return [0.0, frames * HOP_LENGTH / sample_rate, 0.0, sample_rate / 2 / 1000]


def separation_spectrograms(mixture: torch.Tensor, estimated: torch.Tensor, reference: torch.Tensor,
                            stem_name: str = "stem", sample_rate: int = 44100) -> dict:
    """The data of `plot_separation_spectrograms` (`utils.py:220-264`): `spectrograms` = {title: (1025, frames)} in
    the reference's panel order, `vmin` / `vmax` = the global extremes of the three arrays (`:187-188`), `extent`
    and `suptitle`."""
    specs, vmin, vmax = _spectrograms_of([mixture, estimated, reference])
    titles = ["Mixture", f"Estimated ({stem_name})", f"Ground Truth ({stem_name})"]
    return {"spectrograms": {t: specs[i] for i, t in enumerate(titles)}, "vmin": vmin, "vmax": vmax,
            "extent": _extent(specs[-1].shape[-1], sample_rate),
            "suptitle": f"Stem Separation: {stem_name.capitalize()}"}


def all_stems_spectrograms(mixture: torch.Tensor, estimated_stems: Dict[str, torch.Tensor],
                           reference_stems: Dict[str, torch.Tensor], sample_rate: int = 44100) -> dict:
    """The data of `plot_all_stems_spectrograms` (`utils.py:267-356`): `stems` = {stem: {"estimated", "reference"}}
    in `estimated_stems`' key order, `vmin` / `vmax` global over all of them (`:318-319`), `extent`.  The mixture is
    accepted and unused, as in the reference."""
    names = list(estimated_stems.keys())
    specs, vmin, vmax = _spectrograms_of([w for s in names for w in (estimated_stems[s], reference_stems[s])])
    return {"stems": {s: {"estimated": specs[2 * i], "reference": specs[2 * i + 1]} for i, s in enumerate(names)},
            "vmin": vmin, "vmax": vmax, "extent": _extent(specs[0].shape[-1], sample_rate)}


def all_stems_npz(data: dict) -> dict:
    """The arrays of an `all_stems_spectrograms` result as `numpy.savez` takes them: `{stem}_estimated`,
    `{stem}_reference`, `vmin`, `vmax`, `extent`."""
    import numpy as np
    out = {}
    for s, d in data["stems"].items():
        out[f"{s}_estimated"] = d["estimated"].cpu().numpy()
        out[f"{s}_reference"] = d["reference"].cpu().numpy()
    out["vmin"] = np.float32(data["vmin"])
    out["vmax"] = np.float32(data["vmax"])
    out["extent"] = np.asarray(data["extent"], dtype=np.float64)
    return out
