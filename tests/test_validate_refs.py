"""CPU checks of the validation twin (athd/loss.py, athd/validate.py) that need no GPU:

  * the float64 restatements of tests/validate_refs.py reproduce what the reference's own `src/loss.py` functions and
    its own `validate` returned (tests/golden/loss_ref.npz, written by tests/golden/gen_loss_fixture.py), within the
    reference's fp32 arithmetic: |fp32 reference - float64| was measured at <= 1.7e-6 dB on these input families, the
    assertion is 1e-5 per value;
  * `validate_ref` and `athd.validate.reduce_rows` are the mean over batches of the batch means;
  * `SegmentDataset` is `segment_index` + `extract_segment` + transposition;
  * the modules import, and the header and `native.EXPORTED` carry the three new names.
"""
import os
import random

import numpy as np
import pytest
import torch

import validate_refs as V
from conftest import GOLDEN, REPO

TOL = 1e-5


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "loss_ref.npz"))


@pytest.fixture(scope="module")
def loss_table(fx):
    return V.loss_rows_ref(fx["loss_est"], fx["loss_target"])


def test_fixture_inputs_are_the_seeded_inputs(fx):
    est, tgt = V.loss_fixture_inputs()
    assert np.array_equal(fx["loss_est"], est.numpy()) and np.array_equal(fx["loss_target"], tgt.numpy())
    assert os.path.getsize(os.path.join(GOLDEN, "loss_ref.npz")) < 200 * 1024
    # one row per SNR, none near a clamp
    assert np.allclose(V.loss_rows_ref(est, tgt)[:, V.NEW_SDR], V.SNRS_DB, atol=1e-3)
    assert V.clamp_margin(est, tgt) > 0.01


def test_row_functions_match_reference(fx, loss_table):
    t = loss_table
    assert np.abs(-t[:, V.SDR] - fx["sdr_loss_rows"]).max() <= TOL
    assert np.abs(-t[:, V.SISDR] - fx["sisdr_loss_rows"]).max() <= TOL
    assert np.abs(t[:, V.NEW_SDR] - fx["new_sdr_rows"]).max() <= TOL
    assert np.abs(t[:, V.NEW_SDR] - fx["new_sdr_batch"]).max() <= TOL
    assert abs(-t[:, V.SDR].mean() - float(fx["sdr_loss_batch"])) <= TOL
    assert abs(-t[:, V.SISDR].mean() - float(fx["sisdr_loss_batch"])) <= TOL


@pytest.mark.parametrize("name,fn,keys", [("combined", V.combined_loss_ref, V.COMBINED_KEYS),
                                           ("combined_l1", V.combined_l1_ref, V.COMBINED_L1_KEYS)])
def test_combined_match_reference(fx, loss_table, name, fn, keys):
    assert tuple(fx[f"{name}_keys"]) == tuple(keys)
    cases = [(loss_table[i:i + 1], fx[f"{name}_rows"][i]) for i in range(len(loss_table))]
    cases.append((loss_table, fx[f"{name}_batch"]))
    for table, want in cases:
        total, metrics = fn(table)
        assert tuple(metrics) == tuple(keys)
        got = np.array([total] + [metrics[k] for k in keys])
        assert np.abs(got - want).max() <= TOL, (name, got, want)


@pytest.mark.parametrize("tag,kw", [("cmb", {}),
                                    ("l1", dict(use_L1_cmb_loss=True, l1_sdr_weight=1.0, l1_weight=0.05))])
def test_validate_ref_matches_reference(fx, tag, kw):
    batches = V.make_batches(fx["val_mixture"], fx["val_target"], list(fx["val_stems"]))
    assert len(batches) == 6 and len(batches[-1]["prompt"]) == 1
    got = V.validate_ref(V.StubModel(fx["val_noise"]).eval(), batches, **kw)
    want = dict(zip(fx[f"validate_{tag}_keys"], fx[f"validate_{tag}_vals"]))
    assert list(got) == list(want)
    for k in want:
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])


def test_reduce_rows_matches_reference(fx):
    """athd.validate's regrouping of a per-item table gives the reference's dict too."""
    from athd.validate import _weights, reduce_rows
    stems = list(fx["val_stems"])
    est = V.StubModel(fx["val_noise"]).eval()(torch.as_tensor(fx["val_mixture"]), None)
    table = V.loss_rows_ref(est, fx["val_target"])
    for tag, l1 in (("cmb", False), ("l1", True)):
        w1, w2 = _weights(l1, 1.0, 0.05, 0.9, 0.1)
        got = reduce_rows(table, stems, 3, l1, w1, w2)
        want = dict(zip(fx[f"validate_{tag}_keys"], fx[f"validate_{tag}_vals"]))
        assert list(got) == list(want)
        assert max(abs(got[k] - want[k]) for k in want) <= TOL


def test_mean_of_batch_means_not_mean_of_items():
    """3 items, batch_size 2: batches {20 dB, 20 dB} and {0 dB}: the mean of batch means is 10 dB, the mean of items
    13.3 dB."""
    g = torch.Generator().manual_seed(5)
    t = torch.randn(3, 2, 400, generator=g)
    z = torch.randn(3, 2, 400, generator=g)
    z = z / z.reshape(3, -1).norm(dim=1)[:, None, None] * t.reshape(3, -1).norm(dim=1)[:, None, None]
    est = t + z * torch.tensor([0.1, 0.1, 1.0])[:, None, None]
    batches = V.make_batches(est, t, ["drums", "bass", "drums"], batch_size=2)
    got = V.validate_ref(lambda mixture, prompts: mixture, batches)
    items = V.loss_rows_ref(est, t)[:, V.SDR]
    of_batches = (items[:2].mean() + items[2]) / 2
    assert abs(items.mean() - of_batches) > 0.1
    assert abs(got["sdr"] - of_batches) < 1e-9
    assert abs(got["sdr/drums"] - (items[0] + items[2]) / 2) < 1e-9 and abs(got["sdr/bass"] - items[1]) < 1e-9
    assert "sdr/vocals" not in got
    from athd.validate import reduce_rows
    mine = reduce_rows(V.loss_rows_ref(est, t), ["drums", "bass", "drums"], 2, False, 0.9, 0.1)
    assert abs(mine["sdr"] - of_batches) < 1e-9 and abs(mine["loss"] - got["loss"]) < 1e-9


def test_validate_l1_without_weight_raises():
    from athd.validate import _weights
    with pytest.raises(ValueError, match="l1_weight must be provided"):
        V.validate_ref(None, [], use_L1_cmb_loss=True)
    with pytest.raises(ValueError, match="l1_weight must be provided"):
        _weights(True, 1.0, None, 0.9, 0.1)


def test_segment_dataset_items(tmp_path):
    from athd.musdb import STEM_PROMPTS, MusDBTracks, extract_segment, segment_index
    from athd.validate import SegmentDataset
    rng = np.random.default_rng(3)
    lengths = [2500, 2000]                      # S = 1000: a padded last segment, and an exactly full last one
    arrays = [rng.standard_normal((5, L, 2)).astype(np.float32) for L in lengths]
    for i, a in enumerate(arrays):
        np.save(tmp_path / f"track{i}.stem.npy", a)
    ds = SegmentDataset(MusDBTracks(tmp_path), 1000)
    assert ds.index_map == segment_index(lengths, 1000) and len(ds) == 4 * 3 + 4 * 2
    seen = set()
    random.seed(1)
    for idx, (fi, si, seg) in enumerate(ds.index_map):
        item = ds[idx]
        want = extract_segment(arrays[fi], seg, 1000)
        assert item["mixture"].shape == (2, 1000) and item["mixture"].dtype == torch.float32
        assert np.array_equal(item["mixture"].numpy(), want[0].T)
        assert np.array_equal(item["target"].numpy(), want[si + 1].T)
        assert (item["stem_name"], item["file_idx"], item["segment_idx"]) == (ds.stem_names[si], fi, seg)
        assert item["prompt"] in STEM_PROMPTS[item["stem_name"]]
        seen.add((fi, seg))
    assert {(0, 0), (0, 1), (0, 2), (1, 1)} <= seen          # first, middle, padded last, exactly full last
    assert np.all(ds[2]["mixture"].numpy()[:, 500:] == 0) and np.any(ds[2]["mixture"].numpy()[:, :500] != 0)
    # the prompt draws are those of the reference's __getitem__: one random.choice per item from the global random
    random.seed(9)
    got = [ds[i]["prompt"] for i in range(len(ds))]
    random.seed(9)
    assert got == [random.choice(STEM_PROMPTS[ds.stem_names[si]]) for _, si, _ in ds.index_map]


def test_modules_import_and_abi_names():
    import re
    import athd.loss
    import athd.validate
    from athd import native
    assert athd.loss.sdr_loss is __import__("athd.inference", fromlist=["x"]).sdr_loss
    assert callable(athd.validate.validate) and callable(athd.validate.main)
    header = open(os.path.join(REPO, "include", "athd.h")).read()
    for name in ("athd_loss_rows_scratch_bytes", "athd_loss_rows", "athd_gather_segments"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in native.EXPORTED and hasattr(native.lib, name)
    assert native.lib.athd_loss_rows_scratch_bytes(0, 5) == 0
    assert native.lib.athd_loss_rows_scratch_bytes(1, 1 << 31) == 0
    assert native.lib.athd_loss_rows_scratch_bytes((1 << 20) + 1, 5) == 0
    assert native.lib.athd_loss_rows_scratch_bytes(3, 63) >= 8 * 8 * 3            # 5 + 3 sums per row at least
