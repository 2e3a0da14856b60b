"""The any-rate audio front end on the GPU: `athd_resample`, `athd_spectrogram_db` (csrc/audio_io.hip) and the
`app.py` twin (athd/app.py), against the CPU references of tests/audio_refs.py.

Resampler bound, per output sample, derived (not tuned):
    |y_gpu - y_ref64| <= (NT + 4) * 2^-24 * sum_k |xpad| |K| + 1e-30
y_ref64 is the same fp32 table convolved in float64 (no accumulation error); NT = live taps per phase.  The kernel does
NT fp32 FMAs (each rounding <= 2^-24 of a partial sum bounded by sum |x| |K|), and the host table may differ from the
reference table by one fp32 ulp per tap where a host sin / cos differs in the last bit (2^-23 |K| per tap, i.e.
2 * 2^-24 * sum |x| |K| in all): NT + 2 <= NT + 4.  torch's own fp32 conv1d measures 3.5 .. 4.6 in units of
2^-24 * sum |x| |K| on the CPU.

Spectrogram bound: TOL = 4 x 5e-7.  5e-7 is torch's own fp32 stft against its float64 stft, max over bins of
|X32 - X64| / ||frame||_2, measured on the CPU on random input (3.6e-7 .. 5.7e-7 over T in {1025 .. 200000}, mono and
stereo); the factor 4 allows for a different FFT factorisation (packed real 1024-point radix-4 here).
    magnitude: |(10^(dB / 20) - 1e-8) - |X64|| <= TOL * ||frame||_2            for every bin
    dB:        |dB - dB64| <= 20 log10(1 + TOL * ||frame||_2 / (|X64| + 1e-8)) + 1e-4   for every bin, no exclusions
"""
import math

import numpy as np
import pytest
import torch

import audio_refs as R

pytestmark = pytest.mark.gpu

EINVAL = -1
SENTINEL = -12345.5
TOL = 4 * 5e-7


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _resample_raw(src, L, in_ch, fs, cs, sr, new, out_ch):
    """athd_resample into a buffer one sentinel row longer than needed -> (rc, buffer (out_ch + 1, L'))."""
    from athd import native
    need = native.lib.athd_resample_scratch_bytes(sr, new)
    assert need > 0
    n = native.lib.athd_resample_length(L, sr, new)
    assert n == R.resample_length(L, sr, new)
    out = torch.full((out_ch + 1, n), SENTINEL, dtype=torch.float32, device="cuda")
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = native.lib.athd_resample(src.data_ptr(), L, in_ch, fs, cs, sr, new, out.data_ptr(), out_ch,
                                  scratch.data_ptr(), need, _stream())
    torch.cuda.synchronize()
    return rc, out.cpu()


def _forms(x2):
    """x2 (2, L) CPU -> {form: (device source, in_ch, frame_stride, channel_stride, out_ch, planar CPU input)}."""
    L = x2.shape[1]
    return {
        "mono_to_stereo": (x2[0].contiguous().cuda(), 1, 1, 0, 2, x2[:1]),
        "interleaved": (x2.T.contiguous().cuda(), 2, 2, 1, 2, x2),
        "planar": (x2.contiguous().cuda(), 2, 1, L, 2, x2),
    }


def _lengths(sr):
    o = R.resample_params(sr, 44100)[0]
    return sorted({L for L in (1, o - 1, o, o + 1, 3 * o + 7, 20011) if L >= 1})


def _check(out, x_planar, sr, form):
    """The bound, the sentinel row and the mono duplication for one output buffer."""
    y, s = R.resample_ref(x_planar, sr, 44100)
    if x_planar.shape[0] == 1:
        assert torch.equal(out[0], out[1]), form
        y, s = y.expand(2, -1), s.expand(2, -1)
    assert torch.all(out[2] == SENTINEL), form
    bound = (R.live_taps(sr, 44100) + 4) * 2.0 ** -24 * s + 1e-30
    err = (out[:2].double() - y).abs()
    worst = (err / bound).max().item()
    print(f"resample {sr} {form} L={x_planar.shape[1]}: max err / bound = {worst:.3f}")
    assert torch.all(err <= bound), (form, worst)


@pytest.mark.parametrize("form", ["mono_to_stereo", "interleaved", "planar"])
@pytest.mark.parametrize("sr", [48000, 22050, 96000, 8000])
def test_resample_matches_reference(sr, form):
    for L in _lengths(sr):
        x2 = torch.randn(2, L, generator=torch.Generator().manual_seed(sr + L))
        src, in_ch, fs, cs, out_ch, x_planar = _forms(x2)[form]
        rc, out = _resample_raw(src, L, in_ch, fs, cs, sr, 44100, out_ch)
        assert rc == 0
        _check(out, x_planar, sr, f"{form}/L={L}")
        rc2, again = _resample_raw(src, L, in_ch, fs, cs, sr, 44100, out_ch)
        assert rc2 == 0 and torch.equal(out, again), (form, L)


def test_resample_many_chunks_per_workgroup():
    """22050 -> 44100 has 2048-sample chunks; past 2048 chunks a workgroup loops over several of them."""
    L = 2048 * 2100 + 5
    x = torch.randn(1, L, generator=torch.Generator().manual_seed(3))
    rc, out = _resample_raw(x[0].cuda(), L, 1, 1, 0, 22050, 44100, 2)
    assert rc == 0
    _check(out, x, 22050, "long mono")


@pytest.mark.parametrize("form", ["mono_to_stereo", "interleaved", "planar"])
def test_resample_identity_is_bit_equal(form):
    for L in (1, 255, 256, 257, 20011):
        x2 = torch.randn(2, L, generator=torch.Generator().manual_seed(L))
        src, in_ch, fs, cs, out_ch, x_planar = _forms(x2)[form]
        rc, out = _resample_raw(src, L, in_ch, fs, cs, 44100, 44100, out_ch)
        assert rc == 0
        assert torch.equal(out[:2], x_planar.expand(2, -1)), (form, L)
        assert torch.all(out[2] == SENTINEL)


def test_resample_refuses_unsupported_pair_and_bad_arguments():
    from athd import native
    assert native.lib.athd_resample_scratch_bytes(44101, 44100) == 0
    x = torch.zeros(2, 1000, device="cuda")
    out = torch.full((2, 1000), SENTINEL, device="cuda")
    scratch = torch.empty(65536, dtype=torch.uint8, device="cuda")
    args = (out.data_ptr(), 2, scratch.data_ptr(), 65536, _stream())
    assert native.lib.athd_resample(x.data_ptr(), 1000, 2, 1, 1000, 44101, 44100, *args) == EINVAL
    assert native.lib.athd_resample(x.data_ptr(), 0, 2, 1, 1000, 48000, 44100, *args) == EINVAL
    # 2 channels into 3 is neither a copy nor a mono duplication
    assert native.lib.athd_resample(x.data_ptr(), 1000, 2, 1, 1000, 48000, 44100, out.data_ptr(), 3,
                                    scratch.data_ptr(), 65536, _stream()) == EINVAL
    assert native.lib.athd_resample(x.data_ptr(), 1000, 2, 1, 1000, 48000, 44100, out.data_ptr(), 2,
                                    scratch.data_ptr(), 16, _stream()) == -5
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)


def test_app_resample_planar_tensor():
    from athd import app
    x = torch.randn(2, 4801, generator=torch.Generator().manual_seed(11))
    y = app.resample(x.cuda(), 48000, 44100).cpu()
    ref, s = R.resample_ref(x, 48000, 44100)
    assert y.shape == ref.shape
    assert torch.all((y.double() - ref).abs() <= (R.live_taps(48000, 44100) + 4) * 2.0 ** -24 * s + 1e-30)
    with pytest.raises(ValueError, match="not supported"):
        app.resample(x.cuda(), 44101, 44100)


# ------------------------------------------------------------------------------------------------- spectrogram
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("T", [1025, 2048, 5000, 20000])
def test_spectrogram_db_matches_float64_stft(T, C):
    from athd import app
    wav = torch.randn(C, T, generator=torch.Generator().manual_seed(T + C))
    got = app.create_spectrogram(wav.cuda()).cpu().double()
    assert tuple(got.shape) == (1025, 1 + T // 512)
    X, norm = R.stft_ref(wav)
    mag = X.abs()
    err = ((10.0 ** (got / 20.0) - 1e-8) - mag).abs() / norm[None]
    db_ref = 20 * torch.log10(mag + 1e-8)
    db_bound = 20 * torch.log10(1 + TOL * norm[None] / (mag + 1e-8)) + 1e-4
    db_err = (got - db_ref).abs()
    print(f"spectrogram T={T} C={C}: max mag err / ||frame|| = {err.max().item():.3e} (TOL {TOL:.1e}), "
          f"max dB err / bound = {(db_err / db_bound).max().item():.3f}")
    assert torch.all(err <= TOL)
    assert torch.all(db_err <= db_bound)


def test_spectrogram_refuses_short_input():
    from athd import native
    x = torch.zeros(2, 1024, device="cuda")
    out = torch.full((1025, 3), SENTINEL, device="cuda")
    assert native.lib.athd_spectrogram_db(x.data_ptr(), 2, 1024, out.data_ptr(), _stream()) == EINVAL
    assert native.lib.athd_spectrogram_db(x.data_ptr(), 0, 1024, out.data_ptr(), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)


def test_resample_and_spectrogram_replay_from_a_graph():
    """After one eager call for the rate pair both entry points only enqueue work on the stream: captured once,
    replayed on new input, equal to the eager result bit for bit."""
    from athd import native
    L, sr = 20011, 48000
    g = torch.Generator().manual_seed(21)
    x = torch.randn(L, 2, generator=g).cuda()                  # interleaved frames
    x_next = torch.randn(L, 2, generator=g).cuda()
    need = native.lib.athd_resample_scratch_bytes(sr, 44100)
    n = native.lib.athd_resample_length(L, sr, 44100)
    out = torch.empty(2, n, device="cuda")
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    spec = torch.empty(1025, 1 + n // 512, device="cuda")

    def run():
        assert native.lib.athd_resample(x.data_ptr(), L, 2, 2, 1, sr, 44100, out.data_ptr(), 2, scratch.data_ptr(),
                                        need, _stream()) == 0
        assert native.lib.athd_spectrogram_db(out.data_ptr(), 2, n, spec.data_ptr(), _stream()) == 0

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    x.copy_(x_next)
    out.fill_(SENTINEL)
    spec.fill_(SENTINEL)
    scratch.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got_out, got_spec = out.clone(), spec.clone()
    run()
    torch.cuda.synchronize()
    assert torch.equal(got_out, out) and torch.equal(got_spec, spec)
    assert not torch.any(got_out == SENTINEL) and not torch.any(got_spec == SENTINEL)


# --------------------------------------------------------------------------------------------------------- app
@pytest.fixture(scope="module")
def model_bf16(state_dict, text_table):
    from athd.model import AudioTextHTDemucs
    from athd.weights import STEMS
    m = AudioTextHTDemucs(dtype="bf16", text_table={s: text_table[i] for i, s in enumerate(STEMS)})
    m.load_state_dict(state_dict)
    return m.to("cuda").eval()


def test_process_audio_mono_48k_file(model_bf16, tmp_path):
    from athd import app
    from athd.benchmark import OurModel
    from athd.musdb import read_wav, write_wav
    sr, L = 48000, int(3.3 * 48000)
    t = np.arange(L) / sr
    rng = np.random.default_rng(5)
    x = (0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1000 * t) + 0.05 * rng.standard_normal(L))
    path = tmp_path / "mono48k.wav"
    write_wav(path, x.astype(np.float32)[:, None], sr)            # PCM16

    inp, out, spec_in, spec_out, status = app.process_audio(model_bf16, str(path), "vocals", segment_seconds=1.0,
                                                            overlap=0.1)
    assert status == "✓ Successfully separated 'vocals' from the mixture!"
    loaded, lsr = app.load_audio(path)
    assert lsr == 44100 and inp[0] == out[0] == 44100
    T = R.resample_length(L, sr, 44100)
    assert tuple(loaded.shape) == (2, T) and inp[1].shape == out[1].shape == (T, 2)
    assert np.array_equal(inp[1], loaded.T.cpu().numpy())

    samples, rate = read_wav(path)
    assert rate == sr and samples.shape == (L, 1)
    ref, s = R.resample_ref(torch.from_numpy(samples.T.copy()), sr, 44100)
    bound = (R.live_taps(sr, 44100) + 4) * 2.0 ** -24 * s + 1e-30
    lc = loaded.cpu()
    assert torch.equal(lc[0], lc[1])
    assert torch.all((lc.double() - ref.expand(2, -1)).abs() <= bound.expand(2, -1))

    want = OurModel(model_bf16, segment_seconds=1.0, overlap=0.1)._chunked_inference(loaded, "vocals")
    assert np.array_equal(out[1], want.T.cpu().numpy())
    assert torch.equal(spec_in, app.create_spectrogram(loaded))
    assert torch.equal(spec_out, app.create_spectrogram(want))
    assert tuple(spec_in.shape) == tuple(spec_out.shape) == (1025, 1 + T // 512)
    assert torch.isfinite(spec_out).all()


def test_process_audio_reports_failures_as_status(model_bf16, tmp_path):
    from athd import app
    assert app.process_audio(model_bf16, None, "vocals") == (None, None, None, None, "Please upload an audio file.")
    assert app.process_audio(model_bf16, "whatever.wav", "") == (None, None, None, None,
                                                                  "Please enter a text prompt.")
    res = app.process_audio(model_bf16, str(tmp_path / "missing.wav"), "vocals")
    assert res[:4] == (None, None, None, None) and res[4].startswith("Error: ")
