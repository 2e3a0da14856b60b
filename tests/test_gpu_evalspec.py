"""Evaluation spectrograms on the GPU: `athd_eval_spectrogram` (csrc/audio_io.hip), `athd/utils.py`, the
`plot_spectrograms` path of `athd/benchmark.py` and `athd/generate_spectrogram.py`, against the float64 restatement
and the interval bound of tests/evalspec_refs.py.

TOL = 4 x r with r = 1.84e-7 as measured and stated in tests/test_evalspec_refs.py (torch's own fp32 Hann stft
against its float64 stft over these inputs).  The share of bins whose interval is wide is capped at 1 %: wider than
0.1 dB on the randn, quiet and late inputs (late is scaled noise, so it takes the noise inputs' cap), wider than 1 dB
on the tone input.  The floor, the range, batching and graph replay are checked bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import evalspec_refs as E

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -5
SENTINEL = -12345.5
INF = float("inf")
TOL = E.TOL
WIDE_DB = {"randn": 0.1, "quiet": 0.1, "late": 0.1, "tone": 1.0}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw(x, power=2.0, to_db=1, top_db=80.0, want_range=True):
    """athd_eval_spectrogram on x (N, C, T) device -> (rc, out (N + 1, 1025, frames) with a sentinel slab after the
    output, range (N + 1, 2) with a sentinel pair after it)."""
    from athd import native
    N, C, T = x.shape
    F = native.lib.athd_spectrogram_frames(T)
    assert F == E.frames(T)
    out = torch.full((N + 1, 1025, F), SENTINEL, dtype=torch.float32, device="cuda")
    rng = torch.full((N + 1, 2), SENTINEL, dtype=torch.float32, device="cuda")
    need = native.lib.athd_eval_spectrogram_scratch_bytes(N)
    assert need > 0
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = native.lib.athd_eval_spectrogram(x.data_ptr(), N, C, T, C * T, power, to_db, top_db, out.data_ptr(),
                                          rng.data_ptr() if want_range else None, scratch.data_ptr(), need, _stream())
    torch.cuda.synchronize()
    return rc, out, rng


# ------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("T", [1025, 2048, 5000, 20000])
@pytest.mark.parametrize("kind,power", [("randn", 1.0), ("randn", 2.0), ("tone", 2.0), ("quiet", 1.0),
                                        ("quiet", 2.0), ("late", 1.0), ("late", 2.0)])
def test_matches_float64_restatement(kind, power, T, C):
    """3 frames in one partial group, 5 frames, one full + one partial group, 5 groups."""
    from athd import utils
    wav = E.make_input(kind, T, C)
    X, norm = E.stft_ref(wav)
    what = f"{kind} p={power:g} T={T} C={C}"
    got = utils.compute_spectrogram(wav.cuda(), power=power).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (1025, E.frames(T))
    E.check_db(got, X, norm, TOL, power, 80.0, WIDE_DB[kind], what)
    lin = utils.compute_spectrogram(wav, power=power, to_db=False).cpu()         # a CPU tensor is moved over
    E.check_power(lin, X, norm, TOL, power, what + " linear")
    if kind == "quiet" and power == 2.0:
        # |X|^2 is about 8e-12 on average, so all but a stray peak (e^-13 of the bins) sit on the 1e-10 clamp
        assert (got == -100.0).double().mean().item() > 0.99


def test_python_argument_checks():
    from athd import utils
    x = torch.zeros(2, 5000)
    for kw in ({"n_fft": 1024}, {"hop_length": 256}, {"power": 1.5}, {"power": 0.5}):
        with pytest.raises(ValueError):
            utils.compute_spectrogram(x, **kw)
    with pytest.raises(ValueError):
        utils.compute_spectrogram(torch.zeros(2, 1024))
    mono = E.make_input("randn", 5000, 1)
    assert torch.equal(utils.compute_spectrogram(mono[0]), utils.compute_spectrogram(mono))    # (T,) == (1, T)


# ------------------------------------------------------------------------------------------------------- floor
@pytest.mark.parametrize("kind,T", [("tone", 5000), ("tone", 20000), ("late", 5000), ("late", 20000)])
def test_floor_and_range_are_exact(kind, T):
    x = E.make_input(kind, T, 2).cuda()[None]
    rc_u, U, rng_u = _raw(x, top_db=INF)
    rc_g, G, rng_g = _raw(x, top_db=80.0)
    assert rc_u == 0 and rc_g == 0
    U, G = U[0], G[0]
    assert torch.equal(G, torch.maximum(U, U.max() - 80.0))
    assert torch.equal(rng_g[0], torch.stack([G.min(), G.max()]))
    assert torch.equal(rng_u[0], torch.stack([U.min(), U.max()]))
    assert torch.all(rng_g[1] == SENTINEL) and torch.all(rng_u[1] == SENTINEL)
    on_floor = (G == G.min()).double().mean().item()
    print(f"floor {kind} T={T}: range {rng_g[0].tolist()}, {100 * on_floor:.1f} % of bins on the floor")
    if kind == "tone":
        assert on_floor > 0.5
    else:
        # the maximum lies in the last frame group (a partial one at T = 5000) and still floors the first
        frame_of_max = int(U.argmax().item()) % U.shape[1]
        assert U.shape[1] > 8 and frame_of_max >= (U.shape[1] - 1) // 8 * 8
        assert (G[:, :8] > U[:, :8]).any()


# ---------------------------------------------------------------------------------------------------- batching
def _nine_signals(T=5000, C=2):
    kinds = ["randn", "tone", "quiet", "late", "randn", "tone", "quiet", "late", "randn"]
    return [E.make_input(k, T, C, seed=i // 4) for i, k in enumerate(kinds)]


def test_batch_equals_single_calls_and_honours_the_stride():
    from athd import native
    sigs = _nine_signals()
    N, (C, T) = len(sigs), sigs[0].shape
    F = E.frames(T)
    stride = C * T + 37
    buf = torch.full((N * stride,), 7.0, dtype=torch.float32, device="cuda")
    for i, s in enumerate(sigs):
        buf[i * stride:i * stride + C * T] = s.cuda().reshape(-1)
    need = native.lib.athd_eval_spectrogram_scratch_bytes(N)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

    def run():
        out = torch.full((N + 1, 1025, F), SENTINEL, dtype=torch.float32, device="cuda")
        rng = torch.full((N + 1, 2), SENTINEL, dtype=torch.float32, device="cuda")
        rc = native.lib.athd_eval_spectrogram(buf.data_ptr(), N, C, T, stride, 2.0, 1, 80.0, out.data_ptr(),
                                              rng.data_ptr(), scratch.data_ptr(), need, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        return out, rng

    out, rng = run()
    assert torch.all(out[N] == SENTINEL) and torch.all(rng[N] == SENTINEL)
    assert not torch.any(out[:N] == SENTINEL)
    for i, s in enumerate(sigs):
        rc, one, one_rng = _raw(s.cuda()[None])
        assert rc == 0
        assert torch.equal(out[i], one[0]), i
        assert torch.equal(rng[i], one_rng[0]), i
    scratch.fill_(0xAB)                                    # the scratch is initialised by every call
    out2, rng2 = run()
    assert torch.equal(out, out2) and torch.equal(rng, rng2)


def test_compute_spectrograms_batched_form():
    from athd import utils
    sigs = _nine_signals()
    specs, ranges = utils.compute_spectrograms(sigs)
    stacked, ranges2 = utils.compute_spectrograms(torch.stack(sigs).cuda())
    assert tuple(specs.shape) == (9, 1025, E.frames(5000)) and tuple(ranges.shape) == (9, 2)
    assert torch.equal(specs, stacked) and torch.equal(ranges, ranges2)
    for i, s in enumerate(sigs):
        one = utils.compute_spectrogram(s)
        assert torch.equal(specs[i], one)
        assert torch.equal(ranges[i], torch.stack([one.min(), one.max()]))


def test_range_can_be_left_out():
    x = E.make_input("tone", 5000, 2).cuda()[None]
    for top_db, to_db in ((80.0, 1), (INF, 1), (80.0, 0)):
        rc, with_range, _ = _raw(x, to_db=to_db, top_db=top_db)
        rc2, without, rng = _raw(x, to_db=to_db, top_db=top_db, want_range=False)
        assert rc == 0 and rc2 == 0
        assert torch.equal(with_range, without)
        assert torch.all(rng == SENTINEL)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing():
    from athd import native
    C, T, N = 2, 5000, 2
    x = torch.zeros(N, C, T, device="cuda")
    F = E.frames(T)
    out = torch.full((N, 1025, F), SENTINEL, dtype=torch.float32, device="cuda")
    rng = torch.full((N, 2), SENTINEL, dtype=torch.float32, device="cuda")
    scratch = torch.full((64,), 0x5A, dtype=torch.uint8, device="cuda")
    ok = dict(wav=x.data_ptr(), n=N, c=C, t=T, stride=C * T, power=2.0, to_db=1, top_db=80.0, out=out.data_ptr(),
              rng=rng.data_ptr(), scratch=scratch.data_ptr(), sbytes=64)

    def call(**kw):
        a = {**ok, **kw}
        return native.lib.athd_eval_spectrogram(a["wav"], a["n"], a["c"], a["t"], a["stride"], a["power"], a["to_db"],
                                                a["top_db"], a["out"], a["rng"], a["scratch"], a["sbytes"], _stream())

    assert native.lib.athd_eval_spectrogram_scratch_bytes(0) == 0
    cases = [dict(t=1024), dict(t=0), dict(c=0), dict(n=0), dict(n=-1), dict(power=1.5), dict(power=0.0),
             dict(power=float("nan")), dict(top_db=-1.0), dict(top_db=float("nan")), dict(wav=None), dict(out=None),
             dict(scratch=None), dict(stride=C * T - 1), dict(n=70000, sbytes=70000 * 8)]
    for kw in cases:
        assert call(**kw) == EINVAL, kw
    assert call(sbytes=native.lib.athd_eval_spectrogram_scratch_bytes(N) - 1) == EWORKSPACE
    assert call(sbytes=0) == EWORKSPACE
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL) and torch.all(rng == SENTINEL) and torch.all(scratch == 0x5A)
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.any(out == SENTINEL) and not torch.any(rng == SENTINEL)


# ------------------------------------------------------------------------------------------------------- graph
def test_replays_from_a_graph():
    """Both launches and the scratch initialisation are stream work from the first call: captured once after an
    eager call, replayed on new input, equal to the eager result bit for bit."""
    from athd import native
    sigs = _nine_signals()[:3]
    N, (C, T) = len(sigs), sigs[0].shape
    x = torch.stack(sigs).cuda()
    x_next = torch.stack([E.make_input(k, T, C, seed=5) for k in ("late", "randn", "tone")]).cuda()
    out = torch.empty(N, 1025, E.frames(T), device="cuda")
    rng = torch.empty(N, 2, device="cuda")
    need = native.lib.athd_eval_spectrogram_scratch_bytes(N)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

    def run():
        assert native.lib.athd_eval_spectrogram(x.data_ptr(), N, C, T, C * T, 2.0, 1, 80.0, out.data_ptr(),
                                                rng.data_ptr(), scratch.data_ptr(), need, _stream()) == 0

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    x.copy_(x_next)
    out.fill_(SENTINEL)
    rng.fill_(SENTINEL)
    scratch.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    got_out, got_rng = out.clone(), rng.clone()
    run()
    torch.cuda.synchronize()
    assert torch.equal(got_out, out) and torch.equal(got_rng, rng)
    assert not torch.any(got_out == SENTINEL) and not torch.any(got_rng == SENTINEL)


# -------------------------------------------------------------------------------- benchmark / generate_spectrogram
@pytest.fixture(scope="module")
def model_bf16(state_dict, text_table):
    from athd.model import AudioTextHTDemucs
    from athd.weights import STEMS
    m = AudioTextHTDemucs(dtype="bf16", text_table={s: text_table[i] for i, s in enumerate(STEMS)})
    m.load_state_dict(state_dict)
    return m.to("cuda").eval()


def _track(L=40000, seed=9):
    """A one-window track: mixture (2, L) = the sum of four synthetic stems."""
    from athd.weights import STEMS
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float32) / 44100.0
    stems = {}
    for i, s in enumerate(STEMS):
        tone = 0.1 * torch.sin(2 * math.pi * (110.0 * (i + 1)) * t)
        stems[s] = (tone[None] + 0.02 * torch.randn(2, L, generator=g)).contiguous()
    return sum(stems.values()), stems


def test_benchmark_plot_spectrograms_path(model_bf16, tmp_path):
    from athd import utils
    from athd.benchmark import OurModel, evaluate_model, evaluate_model_on_track
    from athd.weights import STEMS
    our = OurModel(model_bf16, segment_seconds=1.0, overlap=0.1)
    mixture, refs = _track()
    refs["bass"] = refs["bass"][:, :39000].contiguous()            # a shorter reference: trimmed per stem (:693-701)
    plain, _ = evaluate_model_on_track(our, mixture, refs, "Some Track - A Name")
    res, est = evaluate_model_on_track(our, mixture, refs, "Some Track - A Name", plot_spectrograms=True,
                                       output_dir=tmp_path)
    assert res == plain
    path = tmp_path / "spectrograms" / "Some_Track_-_A_Name" / "AudioTextHTDemucs_Ours_all_stems.npz"
    assert path.is_file()
    z = np.load(path)
    assert sorted(z.files) == sorted([f"{s}_{k}" for s in STEMS for k in ("estimated", "reference")]
                                     + ["vmin", "vmax", "extent"])
    lo, hi = [], []
    for s in STEMS:
        n = min(est[s].shape[-1], refs[s].shape[-1])
        for key, w in ((f"{s}_estimated", est[s][:, :n]), (f"{s}_reference", refs[s][:, :n])):
            want = utils.compute_spectrogram(w).cpu().numpy()
            assert z[key].dtype == np.float32 and np.array_equal(z[key], want), key
            lo.append(want.min())
            hi.append(want.max())
    assert z["vmin"] == min(lo) and z["vmax"] == max(hi)
    frames = z["vocals_estimated"].shape[1]
    assert frames == E.frames(40000)
    assert np.array_equal(z["extent"], np.array([0.0, frames * 512 / 44100, 0.0, 44100 / 2 / 1000]))

    # evaluate_model passes the two arguments through; without them nothing is written
    out2 = tmp_path / "second"
    r2 = evaluate_model(our, [("Other Track", mixture, refs)], log=None, plot_spectrograms=True, output_dir=out2)
    assert len(r2) == 1 and (out2 / "spectrograms" / "Other_Track" / "AudioTextHTDemucs_Ours_all_stems.npz").is_file()
    out3 = tmp_path / "third"
    assert len(evaluate_model(our, [("Other Track", mixture, refs)], log=None)) == 1 and not out3.exists()


def test_separation_spectrograms_data():
    from athd import utils
    mixture, stems = _track(L=5000)
    d = utils.separation_spectrograms(mixture, stems["drums"] * 0.5, stems["drums"], "drums")
    assert list(d["spectrograms"]) == ["Mixture", "Estimated (drums)", "Ground Truth (drums)"]
    arrays = [utils.compute_spectrogram(w) for w in (mixture, stems["drums"] * 0.5, stems["drums"])]
    for a, b in zip(d["spectrograms"].values(), arrays):
        assert torch.equal(a, b)
    assert d["vmin"] == min(a.min().item() for a in arrays) and d["vmax"] == max(a.max().item() for a in arrays)
    assert d["extent"] == [0.0, E.frames(5000) * 512 / 44100, 0.0, 22.05]
    assert d["suptitle"] == "Stem Separation: Drums"


def test_generate_spectrogram_process_track(model_bf16, tmp_path, capsys):
    from athd import generate_spectrogram as G
    from athd.benchmark import OurModel
    from athd.musdb import MusDBTracks, write_wav
    from athd.weights import STEMS
    assert len(G.TOP5_TRACKS) == 5 and "Tom McKenzie - Directions" in G.TOP5_TRACKS
    name = "The Band - It's A Song"
    mixture, stems = _track()
    root = tmp_path / "test"
    (root / name).mkdir(parents=True)
    write_wav(root / name / "mixture.wav", mixture.numpy().T, 44100)
    for s in STEMS:
        write_wav(root / name / f"{s}.wav", stems[s].numpy().T, 44100)
    tracks = MusDBTracks(root)
    our = OurModel(model_bf16, segment_seconds=1.0, overlap=0.1)

    missing = tmp_path / "missing_out"
    assert G.process_track("No Such Track", our, tracks, missing) is False
    assert "Track not found: " in capsys.readouterr().out
    assert not missing.exists()

    out = tmp_path / "out"
    assert G.process_track(name, our, tracks, out) is True
    safe = "The_Band_-_Its_A_Song"
    assert sorted(p.name for p in out.iterdir()) == sorted([f"{safe}_all_stems.npz"]
                                                           + [f"{safe}_{s}.npz" for s in STEMS])
    frames = E.frames(40000)
    allz = np.load(out / f"{safe}_all_stems.npz")
    for s in STEMS:
        z = np.load(out / f"{safe}_{s}.npz")
        assert list(z["titles"]) == ["Mixture", f"Estimated ({s})", f"Ground Truth ({s})"]
        for k in ("mixture", "estimated", "reference"):
            assert z[k].shape == (1025, frames) and z[k].dtype == np.float32 and np.isfinite(z[k]).all()
        assert np.array_equal(z["estimated"], allz[f"{s}_estimated"])
        assert np.array_equal(z["reference"], allz[f"{s}_reference"])
        assert z["vmin"] == min(z[k].min() for k in ("mixture", "estimated", "reference"))
        assert z["vmax"] == max(z[k].max() for k in ("mixture", "estimated", "reference"))


def test_generate_spectrogram_main(model_bf16, tmp_path, monkeypatch):
    """The command line: names or the default, directories from the arguments, the checkpoint path from the config
    (the loader itself is replaced: a checkpoint's CLAP tower cannot be built here)."""
    from athd import generate_spectrogram as G
    from athd import inference
    from athd.musdb import write_wav
    from athd.weights import STEMS
    name = "Tom McKenzie - Directions"
    mixture, stems = _track()
    root = tmp_path / "test"
    (root / name).mkdir(parents=True)
    write_wav(root / name / "mixture.wav", mixture.numpy().T, 44100)
    for s in STEMS:
        write_wav(root / name / f"{s}.wav", stems[s].numpy().T, 44100)
    cfg = tmp_path / "config.yaml"
    cfg.write_text("wandb:\n  checkpoint_dir: some/dir\n")
    asked = []
    monkeypatch.setattr(inference, "load_model", lambda path: asked.append(path) or model_bf16)
    out = tmp_path / "out"
    args = ["--test-dir", str(root), "--config", str(cfg), "--output-dir", str(out)]
    assert G.main(args) == 0                                                     # the reference's default track
    assert asked == ["some/dir/best_model.pt"]
    assert len(list(out.iterdir())) == 5 and (out / "Tom_McKenzie_-_Directions_all_stems.npz").is_file()
    assert G.main(["No Such Track"] + args) == 1
    assert len(list(out.iterdir())) == 5
