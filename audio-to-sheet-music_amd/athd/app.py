"""`app.py` twin (the reference's user-facing path, `app.py:74-256`): a WAV file of any rate, mono or stereo, plus a
free-text prompt -> the separated stem and the dB spectrograms of input and output, on the native hot path.

Mirrors, name for name (the model is passed in instead of being a module global):
  * `load_audio`          <- `app.py:113-126`: torchaudio.load + Resample(sr, 44100) + mono -> stereo.  Here the file
                             is read with `musdb.read_wav`, its interleaved frames go to the device once, and
                             `athd_resample` de-interleaves, resamples and duplicates a mono channel in one pass.
  * `resample`            <- `torchaudio.transforms.Resample(orig, new)(waveform)` with its defaults.
  * `create_spectrogram`  <- `app.py:74-94`: the dB array (`athd_spectrogram_db`); the matplotlib figure of `:96-110`
                             is UI and is not drawn.
  * `chunked_inference`   <- `app.py:129-178`, which is `benchmark.py:155-204`: `OurModel._chunked_inference`.
  * `process_audio`       <- `app.py:205-256` with the reference's status strings; failures end in the status.
  * `main`                <- `python -m athd.app IN.wav "prompt" OUT.wav [--config config.yaml]`.
The YouTube download of `app.py:180-198` needs the network and is not part of this build.
"""
from __future__ import annotations

import sys
from typing import Optional, Tuple

import numpy as np
import torch

from . import native
from .benchmark import SAMPLE_RATE, OurModel
from .musdb import read_wav, wav_info, write_wav


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _resample(src: torch.Tensor, length: int, in_channels: int, frame_stride: int, channel_stride: int,
              orig_freq: int, new_freq: int, out_channels: int) -> torch.Tensor:
    """`athd_resample` on a float32 device buffer -> planar (out_channels, L')."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    need = int(native.lib.athd_resample_scratch_bytes(orig_freq, new_freq))
    if need == 0:
        raise ValueError(f"resampling {orig_freq} Hz -> {new_freq} Hz is not supported (the interpolation table of "
                         f"this rate pair is over the library's bound, see include/athd.h)")
    out_len = int(native.lib.athd_resample_length(length, orig_freq, new_freq))
    out = torch.empty((out_channels, out_len), dtype=torch.float32, device=src.device)
    scratch = torch.empty(need, dtype=torch.uint8, device=src.device)
    rc = native.lib.athd_resample(src.data_ptr(), length, in_channels, frame_stride, channel_stride, orig_freq,
                                  new_freq, out.data_ptr(), out_channels, scratch.data_ptr(), need,
                                  _stream(src.device))
    if rc != 0:
        raise native.AthdError(f"athd_resample failed ({rc})")
    return out


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """`torchaudio.transforms.Resample(orig_freq, new_freq)(waveform)`: (C, L) device tensor -> (C, L')."""
    if waveform.dim() != 2 or waveform.shape[1] == 0:
        raise ValueError(f"expected a (C, L) waveform, got {tuple(waveform.shape)}")
    if waveform.device.type != "cuda":
        raise ValueError("resample runs on a HIP device only (there is no CPU path)")
    x = waveform.float().contiguous()
    C, L = x.shape
    return _resample(x, L, C, 1, L, orig_freq, new_freq, C)


def load_audio(audio_path, target_sr: int = SAMPLE_RATE, device: str = "cuda") -> Tuple[torch.Tensor, int]:
    """`app.py:113-126`: ((2, T) float32 device tensor at `target_sr`, target_sr)."""
    _, channels, _ = wav_info(audio_path)          # ValueError for a file that is not RIFF/WAVE
    if channels not in (1, 2):
        raise ValueError(f"{audio_path}: {channels} channels; only mono and stereo files are supported")
    frames, sr = read_wav(audio_path)              # (L, channels) float32, interleaved in memory
    if frames.shape[0] == 0:
        raise ValueError(f"{audio_path}: no audio samples")
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(device)
    return _resample(x, frames.shape[0], channels, channels, 1, sr, target_sr, 2), target_sr


def create_spectrogram(audio: torch.Tensor) -> torch.Tensor:
    """`app.py:74-94`: audio (C, T) (or (T,)) -> 20 log10(|stft(mean over channels)| + 1e-8) as a (1025, 1 + T // 512)
    float32 device tensor (no figure)."""
    if audio.dim() == 1:
        audio = audio[None]
    if audio.dim() != 2:
        raise ValueError(f"expected a (C, T) waveform, got {tuple(audio.shape)}")
    x = audio.float().contiguous()
    if x.device.type != "cuda":
        x = x.cuda()
    C, T = x.shape
    if T <= 1024:
        raise ValueError(f"the spectrogram's reflect padding needs more than 1024 samples, got {T}")
    out = torch.empty((1025, int(native.lib.athd_spectrogram_frames(T))), dtype=torch.float32, device=x.device)
    rc = native.lib.athd_spectrogram_db(x.data_ptr(), C, T, out.data_ptr(), _stream(x.device))
    if rc != 0:
        raise native.AthdError(f"athd_spectrogram_db failed ({rc})")
    return out


def chunked_inference(model, mixture: torch.Tensor, prompt: str, sample_rate: int = SAMPLE_RATE,
                      segment_seconds: float = 6.0, overlap: float = 0.1) -> torch.Tensor:
    """`app.py:129-178`: mixture (2, T) -> the stem named by `prompt`, (2, T) on the model's device."""
    if sample_rate != SAMPLE_RATE:
        raise ValueError(f"the separator runs at {SAMPLE_RATE} Hz, got sample_rate={sample_rate}")
    return OurModel(model, segment_seconds=segment_seconds, overlap=overlap)._chunked_inference(mixture, prompt)


def process_audio(model, audio_file, text_prompt: Optional[str], sample_rate: int = SAMPLE_RATE,
                  segment_seconds: float = 6.0, overlap: float = 0.1):
    """`app.py:205-256`: ((sr, input (T, 2) numpy), (sr, output (T, 2) numpy), input dB spectrogram, output dB
    spectrogram, status); (None, None, None, None, message) when something is missing or fails."""
    if audio_file is None:
        return None, None, None, None, "Please upload an audio file."
    if not text_prompt or text_prompt.strip() == "":
        return None, None, None, None, "Please enter a text prompt."
    try:
        mixture, sr = load_audio(audio_file, target_sr=sample_rate, device=str(model.device))
        input_spec = create_spectrogram(mixture)
        separated = chunked_inference(model, mixture, text_prompt.strip(), sr, segment_seconds, overlap)
        output_spec = create_spectrogram(separated)
        input_audio = (sr, mixture.T.cpu().numpy())
        output_audio = (sr, separated.T.cpu().numpy())
        status = f"✓ Successfully separated '{text_prompt}' from the mixture!"
        return input_audio, output_audio, input_spec, output_spec, status
    except Exception as e:          # noqa: BLE001 - the reference reports every failure as the status (:251-256)
        return None, None, None, None, f"Error: {str(e)}"


def main(argv=None) -> int:
    """`python -m athd.app IN.wav "prompt" OUT.wav [--config config.yaml]`: the checkpoint and the audio constants
    come from the config as at `app.py:29-33`."""
    import argparse

    from .inference import load_config, load_model
    ap = argparse.ArgumentParser(prog="python -m athd.app", description=__doc__.splitlines()[0])
    ap.add_argument("input")
    ap.add_argument("prompt")
    ap.add_argument("output")
    ap.add_argument("--config", default="config.yaml")
    args = ap.parse_args(argv)
    cfg = load_config(args.config)
    model = load_model(cfg["training"]["resume_from"])
    data = cfg.get("data", {})
    _, out, _, _, status = process_audio(model, args.input, args.prompt, data.get("sample_rate", SAMPLE_RATE),
                                         data.get("segment_seconds", 6.0), data.get("overlap", 0.1))
    print(status)
    if out is None:
        return 1
    write_wav(args.output, out[1], out[0])
    return 0


if __name__ == "__main__":
    sys.exit(main())
