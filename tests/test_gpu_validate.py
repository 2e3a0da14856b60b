"""The validation twin on the GPU: `athd_loss_rows`, `athd_gather_segments`, athd/loss.py and athd/validate.py.

  1. `athd_loss_rows` against the float64 `loss_rows_ref` (tests/validate_refs.py): every dB value within 1e-5 dB, l1
     within 1e-9 relative.  fp64 accumulation of at most 2^21 terms has relative error <= 2^21 2^-53 ~ 2.3e-10; the
     SI-SDR noise term |e|^2 - 2 a <e,t> + a^2 |t|^2 amplifies that by at most 1e3 inside the +-30 dB clamp: 2.3e-7
     relative = 1e-6 dB, and 1e-5 dB leaves that a tenfold margin.  Shapes: tails, n = 2 (mod 4) and odd n (misaligned
     rows), one real 6 s segment, 70000 rows (past a 65535 grid limit); every case also from views that start one
     float into a larger allocation.  Families: five SNRs, a DC offset (where raw moments would cancel), clamps and
     silence.  No row's unclamped value lies within 0.01 dB of +-30 (asserted on the CPU side of each case; the
     70000 rows are 2000 repeats of 35 such rows).
  2. two calls give bit-equal tables; a call captured in a graph and replayed gives the eager table bit for bit.
  3. `athd_gather_segments` is bit-exact against `extract_segment`.
  4. `combined_loss` / `combined_L1_sdr_loss` reproduce the dicts the reference returned (tests/golden/loss_ref.npz).
  5. `validate` end to end on a two-track MUSDB18-HQ directory (16 items, batch_size 3) against `validate_ref` driving
     `model.forward` on the reference's own batches: every key within 1e-3 dB, the tolerance tests/test_gpu_dist.py
     uses for the same metrics through two batchings of the same f32 forward.  With the synthetic weights the CPU
     oracle puts every (segment, stem, prompt) of this case, the padded segment included, between -3.53 and -2.96 dB
     SDR and between -7.43 and -6.35 dB SI-SDR: more than 22 dB from either clamp.
"""
import os
import random

import numpy as np
import pytest
import torch

import validate_refs as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DB_TOL = 1e-5
L1_RTOL = 1e-9
SHAPES = [(1, 1), (3, 63), (5, 74), (4, 257), (5, 3002), (2, 60002), (1, 529200)]


def _check_table(got: np.ndarray, want: np.ndarray, what):
    db = np.abs(got[:, :3] - want[:, :3]).max()
    l1 = (np.abs(got[:, 3] - want[:, 3]) / np.maximum(np.abs(want[:, 3]), 1e-300)).max()
    print(f"loss_rows {what}: worst dB error {db:.3e} (<= {DB_TOL}), worst l1 relative error {l1:.3e} (<= {L1_RTOL})")
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert db <= DB_TOL, (what, db)
    assert l1 <= L1_RTOL, (what, l1)


def _offset_view(x: torch.Tensor) -> torch.Tensor:
    """The same values in a device view that starts one float into a larger allocation."""
    buf = torch.empty(x.numel() + 5, dtype=torch.float32, device="cuda")
    buf[1:1 + x.numel()] = x.reshape(-1).cuda()
    v = buf[1:1 + x.numel()].view(x.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("family", sorted(V.FAMILIES))
@pytest.mark.parametrize("rows,n", SHAPES)
def test_loss_rows_matches_float64(rows, n, family):
    from athd.loss import loss_rows
    est, tgt = V.FAMILIES[family](rows, n)
    assert V.clamp_margin(est, tgt) > 0.01
    want = V.loss_rows_ref(est, tgt)
    _check_table(loss_rows(est.cuda(), tgt.cuda()).cpu().numpy(), want, (rows, n, family, "aligned"))
    e1, t1 = _offset_view(est), _offset_view(tgt)
    _check_table(loss_rows(e1, t1).cpu().numpy(), want, (rows, n, family, "one float in"))
    # est and target misaligned differently: the scalar-load route of the same groups
    _check_table(loss_rows(e1, tgt.cuda()).cpu().numpy(), want, (rows, n, family, "est one float in"))


def test_loss_rows_70000_rows():
    from athd.loss import loss_rows
    base_e, base_t = V.snr_family(35, 3)                     # 35 does not divide 65536: a wrapped row index shows
    assert V.clamp_margin(base_e, base_t) > 0.01
    est, tgt = base_e.repeat(2000, 1), base_t.repeat(2000, 1)
    want = V.loss_rows_ref(est, tgt)
    _check_table(loss_rows(est.cuda(), tgt.cuda()).cpu().numpy(), want, (70000, 3, "snr", "aligned"))
    _check_table(loss_rows(_offset_view(est), _offset_view(tgt)).cpu().numpy(), want, (70000, 3, "snr", "one float in"))


def test_loss_rows_family_values():
    """The families are what they claim: the DC rows' float64 SI-SDR is ~19.1 dB and their SDRs ~20.0 / 10.5 / 0.9 dB;
    the clamp rows give +30 / (-30, +30) / 0 / 0 / (0, +30)."""
    from athd.loss import loss_rows
    e, t = V.dc_family(3, 3002)
    got = loss_rows(e.cuda(), t.cuda()).cpu().numpy()
    assert np.allclose(got[:, V.SISDR], 19.1, atol=0.5) and np.allclose(got[:, V.SDR], [20.0, 10.5, 0.9], atol=0.1)
    e, t = V.clamp_family(5, 3002)
    got = loss_rows(e.cuda(), t.cuda()).cpu().numpy()
    assert got[0, V.SDR] == 30.0 and got[0, V.SISDR] == 30.0 and got[0, V.L1] == 0.0
    assert got[1, V.SDR] == -30.0 and got[1, V.SISDR] == 30.0 and abs(got[1, V.NEW_SDR] + 32.2557) < 1e-3
    assert np.all(got[2, :3] == 0.0) and got[2, V.L1] == 0.0
    assert abs(got[3, V.SDR]) < 1e-12 and got[3, V.SISDR] == 0.0
    assert abs(got[4, V.SDR]) < 1e-12 and got[4, V.SISDR] == 30.0          # t - 2 t = -t: 0 dB; a pure gain: +30


def test_loss_rows_rejects_bad_arguments():
    from athd import native
    x = torch.zeros(16, device="cuda")
    s = torch.zeros(64, dtype=torch.float64, device="cuda")
    o = torch.zeros(4, dtype=torch.float64, device="cuda")
    call = lambda e, t, rows, n, sc, out: native.lib.athd_loss_rows(e, t, rows, n, sc, out, None)
    assert call(x.data_ptr(), x.data_ptr(), 0, 4, s.data_ptr(), o.data_ptr()) == -1
    assert call(x.data_ptr(), x.data_ptr(), 1, 0, s.data_ptr(), o.data_ptr()) == -1
    assert call(x.data_ptr(), x.data_ptr(), 1, 1 << 31, s.data_ptr(), o.data_ptr()) == -1
    assert call(None, x.data_ptr(), 1, 4, s.data_ptr(), o.data_ptr()) == -1
    assert call(x.data_ptr(), x.data_ptr(), 1, 4, None, o.data_ptr()) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,n", [(5, 3002), (2, 60002)])
def test_loss_rows_deterministic_and_capturable(rows, n):
    from athd.loss import loss_rows
    est, tgt = V.dc_family(rows, n, seed=4)
    est, tgt = _offset_view(est), _offset_view(tgt)
    a = loss_rows(est, tgt)
    b = loss_rows(est, tgt)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = loss_rows(est, tgt)
    c.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, c)


def _gather_case(length, S, seed):
    from athd.musdb import extract_segment
    from athd.validate import gather_segments
    rng = np.random.default_rng(seed)
    stems = rng.standard_normal((5, length, 2)).astype(np.float32)
    pairs = [(s, g) for s in range(5) for g in range(-(-length // S))]
    rng.shuffle(pairs)
    got = gather_segments(torch.from_numpy(stems).cuda(), [p[0] for p in pairs], [p[1] for p in pairs], S).cpu().numpy()
    assert got.shape == (len(pairs), 2, S)
    for r, (s, g) in enumerate(pairs):
        assert np.array_equal(got[r], extract_segment(stems, g, S)[s].T), (length, S, s, g)
    return got, pairs


def test_gather_segments_bit_exact():
    got, pairs = _gather_case(70001, 30000, 1)       # first, middle and a padded last segment (10001 real samples)
    last = pairs.index((3, 2))
    assert np.all(got[last][:, 10001:] == 0) and np.any(got[last][:, :10001] != 0)
    _gather_case(30000, 30000, 2)                    # exactly full: no pad
    _gather_case(20, 7, 3)


def test_gather_segments_out_of_range_rows_are_zero():
    from athd import native
    stems = torch.ones((2, 10, 2), device="cuda")
    src = torch.tensor([0, 2, -1, 1, 1], dtype=torch.int32, device="cuda")
    seg = torch.tensor([0, 0, 0, -1, 5], dtype=torch.int64, device="cuda")
    out = torch.full((5, 2, 4), 7.0, device="cuda")
    rc = native.lib.athd_gather_segments(stems.data_ptr(), 2, 10, src.data_ptr(), seg.data_ptr(), 5, 4, out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(out[0], torch.ones(2, 4, device="cuda")) and float(out[1:].abs().max()) == 0.0


def test_combined_losses_match_reference_fixture():
    from athd.loss import combined_L1_sdr_loss, combined_loss, new_sdr_metric, sdr_loss, sisdr_loss
    fx = np.load(os.path.join(GOLDEN, "loss_ref.npz"))
    est, tgt = torch.as_tensor(fx["loss_est"]).cuda(), torch.as_tensor(fx["loss_target"]).cuda()
    for name, fn in (("combined", combined_loss), ("combined_l1", combined_L1_sdr_loss)):
        keys = list(fx[f"{name}_keys"])
        cases = [(est[i:i + 1], tgt[i:i + 1], fx[f"{name}_rows"][i]) for i in range(len(est))]
        cases.append((est, tgt, fx[f"{name}_batch"]))
        for e, t, want in cases:
            total, metrics = fn(e, t)
            assert list(metrics) == keys and all(type(v) is float for v in metrics.values())
            assert total.device.type == "cuda" and total.dim() == 0
            got = np.array([float(total)] + [metrics[k] for k in keys])
            assert np.abs(got - want).max() <= 1e-5, (name, got, want)
    assert "metrics/new_sdr" not in combined_L1_sdr_loss(est, tgt)[1]
    got = new_sdr_metric(est, tgt)
    assert got.shape == (5,) and np.abs(got.cpu().numpy() - fx["new_sdr_batch"]).max() <= 1e-5
    assert abs(float(sdr_loss(est, tgt)) - float(fx["sdr_loss_batch"])) <= 1e-4        # the mean-only kernels, unchanged
    assert abs(float(sisdr_loss(est, tgt)) - float(fx["sisdr_loss_batch"])) <= 1e-4


# ------------------------------------------------------------------------------------------------ end to end
SEG = 30000
LENGTHS = [70001, 30000]
E2E_TOL = 1e-3


@pytest.fixture(scope="module")
def model_f32(state_dict):
    """Built as in tests/test_gpu_dist.py, with a seeded embedding for every prompt of STEM_PROMPTS."""
    from athd.model import AudioTextHTDemucs
    from athd.musdb import STEM_PROMPTS
    from athd.weights import synthetic_text_table
    prompts = [p for ps in STEM_PROMPTS.values() for p in ps]
    table = synthetic_text_table(len(prompts), seed=7)
    m = AudioTextHTDemucs(dtype="f32", text_table={p: table[i] for i, p in enumerate(prompts)})
    m.load_state_dict(state_dict)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from athd.musdb import HQ_FILES, MusDBTracks, write_wav
    from athd.synth import synthetic_mixture
    from athd.validate import SegmentDataset
    root = tmp_path_factory.mktemp("musdb") / "test"
    for t, L in enumerate(LENGTHS):
        d = root / f"Artist {t} - Song"
        d.mkdir(parents=True)
        parts = [synthetic_mixture(L, seed=900 + 10 * t + j) for j in range(4)]
        for f, x in zip(HQ_FILES, [sum(parts)] + parts):
            write_wav(d / f"{f}.wav", x, 44100, "FLOAT")
    ds = SegmentDataset(MusDBTracks(root), SEG)
    assert len(ds) == 16
    return ds


def _reference_batches(dataset, indices, batch_size, first_prompt=False):
    """The reference loader's batches at num_workers=0: `__getitem__` per index in order (one prompt draw each),
    collated in consecutive runs of batch_size."""
    from athd.musdb import STEM_PROMPTS
    items = [dataset[i] for i in indices]
    if first_prompt:
        for it in items:
            it["prompt"] = STEM_PROMPTS[it["stem_name"]][0]
    return [{"mixture": torch.stack([it["mixture"] for it in items[b:b + batch_size]]),
             "target": torch.stack([it["target"] for it in items[b:b + batch_size]]),
             "prompt": [it["prompt"] for it in items[b:b + batch_size]],
             "stem_name": [it["stem_name"] for it in items[b:b + batch_size]]}
            for b in range(0, len(items), batch_size)]


def _same(got, want, what):
    assert list(got) == list(want), what
    worst = max(abs(got[k] - want[k]) for k in want)
    print(f"validate {what}: worst key difference {worst:.3e} (<= {E2E_TOL}); sdr {got['sdr']:.4f} dB")
    assert worst <= E2E_TOL, (what, got, want)


@pytest.fixture(scope="module")
def forward(model_f32):
    return lambda mixture, prompts: model_f32.forward(mixture.cuda(), list(prompts))


def test_validate_random_prompts(model_f32, dataset, forward):
    from athd.validate import validate
    random.seed(5)
    batches = _reference_batches(dataset, range(16), 3)
    assert len(batches) == 6 and len(batches[-1]["prompt"]) == 1
    assert len({p for b in batches for p in b["prompt"]}) > 4          # the draws go beyond the first prompts
    want = V.validate_ref(forward, batches)
    random.seed(5)
    got = validate(model_f32, dataset, batch_size=3, prompts="random")
    assert set(got) == {"loss", "sdr", "sisdr", "sdr/drums", "sdr/bass", "sdr/other", "sdr/vocals"}
    _same(got, want, "random")
    random.seed(5)
    _same(validate(model_f32, dataset, batch_size=3, prompts="random", max_batch=2), want, "random, max_batch 2")


def test_validate_first_prompts(model_f32, dataset, forward):
    from athd.validate import validate
    want = V.validate_ref(forward, _reference_batches(dataset, range(16), 3, first_prompt=True))
    _same(validate(model_f32, dataset, batch_size=3, prompts="first"), want, "first")
    _same(validate(model_f32, dataset, batch_size=3, prompts="first", max_batch=1), want, "first, max_batch 1")


def test_validate_indices_subset_unordered_repeat(model_f32, dataset, forward):
    from athd.validate import validate
    idx = [13, 2, 7, 7, 0]
    random.seed(8)
    want = V.validate_ref(forward, _reference_batches(dataset, idx, 3))
    random.seed(8)
    _same(validate(model_f32, dataset, batch_size=3, indices=idx), want, "indices")
    want = V.validate_ref(forward, _reference_batches(dataset, idx, 3, first_prompt=True))
    _same(validate(model_f32, dataset, batch_size=3, indices=idx, prompts="first"), want, "indices, first")


def test_validate_l1_combination(model_f32, dataset, forward):
    from athd.validate import validate
    kw = dict(use_L1_cmb_loss=True, l1_sdr_weight=1.0, l1_weight=0.05)
    want = V.validate_ref(forward, _reference_batches(dataset, range(16), 3, first_prompt=True), **kw)
    got = validate(model_f32, dataset, batch_size=3, prompts="first", **kw)
    _same(got, want, "L1 combination")
    assert abs(got["loss"] + got["sdr"]) > 1e-6          # the L1 term is in the loss
    with pytest.raises(ValueError, match="l1_weight must be provided"):
        validate(model_f32, dataset, batch_size=3, use_L1_cmb_loss=True, l1_sdr_weight=1.0)


def test_cli_prints_reference_lines(model_f32, dataset, forward, tmp_path, capsys):
    """`python -m athd.validate`'s body on a config file: the reference's `Val - Loss ... SDR ...` and per-stem lines
    (`src/train.py:554-558`), the JSON, and the pct_test subset drawn on the VALIDATION dataset."""
    import json
    import re
    from athd.musdb import STEM_PROMPTS
    from athd.validate import main
    cfg = tmp_path / "config.yaml"
    cfg.write_text(f"data:\n  test_dir: '{dataset.tracks.root}'\n  segment_seconds: {SEG / 44100!r}\n"
                   f"  sample_rate: 44100\n  pct_test: 0.5\ntraining:\n  batch_size: 3\n"
                   f"  loss_weights: {{sdr: 0.9, sisdr: 0.1}}\n  use_L1_comb_loss: false\n"
                   f"  L1_comb_loss: {{sdr_weight: 1.0, l1_weight: 0.05}}\n")
    assert int(44100 * (SEG / 44100)) == SEG
    out = tmp_path / "val.json"
    argv = ["--checkpoint", "unused.pt", "--config", str(cfg), "--seed", "3", "--prompts", "first", "--dtype", "f32",
            "--output", str(out)]
    assert main(argv, model=model_f32) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    got = json.load(open(out))
    torch.manual_seed(3)
    idx = torch.randperm(16)[:8].tolist()
    want = V.validate_ref(forward, _reference_batches(dataset, idx, 3, first_prompt=True))
    _same(got, want, "cli, pct_test 0.5")
    at = lines.index(f"Val - Loss: {got['loss']:.4f}, SDR: {got['sdr']:.2f} dB")
    stems = [s for s in STEM_PROMPTS if f"sdr/{s}" in got]
    assert lines[at + 1:] == [f"  {s}: {got[f'sdr/{s}']:.2f} dB" for s in stems]
    assert re.fullmatch(r"Val - Loss: -?\d+\.\d{4}, SDR: -?\d+\.\d{2} dB", lines[at])
