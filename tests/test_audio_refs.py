"""Hand-checkable facts of the resampler restatement (tests/audio_refs.py) and the host side of athd/app.py; no GPU.

The restatement follows torchaudio.transforms.Resample's published algorithm (sinc_interp_hann, lowpass_filter_width 6,
rolloff 0.99); torchaudio is not installed, so these facts are what pins it:
  * (o, n, w, taps) of the common conversions;
  * output length ceil(n L / o);
  * a 1 kHz sine at each source rate comes out as the analytic 1 kHz sine at 44.1 kHz: interior error (60 samples in
    from each end) <= 1e-2 of the amplitude (one sample of delay would give 0.14; measured 1.5e-4 .. 4.6e-4).
"""
import math

import numpy as np
import pytest
import torch

import audio_refs as R

PARAMS = {48000: (160, 147, 7, 174), 96000: (320, 147, 14, 348), 88200: (2, 1, 13, 28), 22050: (1, 2, 7, 15)}


@pytest.mark.parametrize("sr", sorted(PARAMS))
def test_resample_params(sr):
    assert R.resample_params(sr, 44100) == PARAMS[sr]
    assert tuple(R.resample_table(sr, 44100).shape) == (PARAMS[sr][1], PARAMS[sr][3])


@pytest.mark.parametrize("sr", sorted(PARAMS))
def test_resample_lengths(sr):
    o, n, _, _ = PARAMS[sr]
    for L in (1, 159, 160, 161, 5000):
        want = math.ceil(n * L / o)
        assert R.resample_length(L, sr, 44100) == want
        y, s = R.resample_ref(torch.zeros(1, L), sr, 44100)
        assert y.shape == s.shape == (1, want)


def test_live_band_is_narrow():
    """The taps outside the Hann window's support are exact zeros in the fp32 table."""
    for sr, nt in ((48000, 14), (22050, 14), (8000, 14), (96000, 27), (88200, 27)):
        assert R.live_taps(sr, 44100) <= nt, sr
        k = R.resample_table(sr, 44100)
        assert int((k != 0).sum(dim=1).max()) <= nt


@pytest.mark.parametrize("sr", [48000, 96000, 88200, 22050, 8000])
def test_sine_comes_out_as_the_analytic_sine(sr):
    L = sr // 10
    x = torch.sin(2 * math.pi * 1000 * torch.arange(L, dtype=torch.float64) / sr)[None].float()
    y, _ = R.resample_ref(x, sr, 44100)
    want = torch.sin(2 * math.pi * 1000 * torch.arange(y.shape[1], dtype=torch.float64) / 44100)
    err = (y[0] - want)[60:-60].abs().max().item()
    assert err <= 1e-2, err


def test_library_length_and_scratch_agree_with_the_restatement():
    """Host-side entry points (no device needed): lengths, and the band table size n * (1 + NT rounded up to odd)
    floats for the supported pairs; 0 for a pair over the bound."""
    from athd import native
    for sr in (48000, 96000, 88200, 22050, 8000, 16000, 32000):
        o, n, _, _ = R.resample_params(sr, 44100)
        for L in (1, o - 1 or 1, o, o + 1, 5000, 14_400_000):
            assert native.lib.athd_resample_length(L, sr, 44100) == R.resample_length(L, sr, 44100)
        nt = R.live_taps(sr, 44100)
        assert native.lib.athd_resample_scratch_bytes(sr, 44100) == n * (1 + (nt | 1)) * 4, sr
    assert native.lib.athd_resample_scratch_bytes(44100, 44100) > 0
    assert native.lib.athd_resample_scratch_bytes(44101, 44100) == 0
    assert native.lib.athd_resample_scratch_bytes(0, 44100) == 0
    assert native.lib.athd_spectrogram_frames(20000) == R.spectrogram_frames(20000) == 40


def test_load_audio_refuses_more_than_two_channels(tmp_path):
    from athd import app
    from athd.musdb import write_wav
    p = tmp_path / "three.wav"
    write_wav(p, np.zeros((3000, 3), dtype=np.float32), 48000)
    with pytest.raises(ValueError, match="3 channels"):
        app.load_audio(p)
    q = tmp_path / "not_a_wav.mp3"
    q.write_bytes(b"ID3" + bytes(64))
    with pytest.raises(ValueError, match="RIFF"):
        app.load_audio(q)


def test_process_audio_statuses_need_no_model():
    from athd import app
    assert app.process_audio(None, None, "drums") == (None, None, None, None, "Please upload an audio file.")
    assert app.process_audio(None, "x.wav", "  ") == (None, None, None, None, "Please enter a text prompt.")
    assert app.process_audio(None, "x.wav", None)[4] == "Please enter a text prompt."
