"""CPU checks of the training ends (athd/loss.py `loss_with_grad`, athd/train_data.py, athd/train.py) that need no GPU:

  * the float64 autograd restatement of tests/train_refs.py reproduces the gradients the reference's own
    `combined_loss` / `combined_L1_sdr_loss` gave in f32 (tests/golden/train_ref.npz, written by
    tests/golden/gen_train_fixture.py) within 4 a per row, a = the fixture's worst gap of those f32 gradients to float64
    autograd of the reference itself (recorded: 4.4e-7 of a row's largest |gradient|);
  * the fixture's inputs are the seeded inputs;
  * `TrainSegmentDataset.__getitem__` and `draw` reproduce the items and plans the reference's dataset produced, bit
    for bit, and leave Python's `random` in the same state;
  * the header and `native.EXPORTED` carry the four new names.
"""
import os
import random
import re

import numpy as np
import pytest
import torch

import train_refs as R
from conftest import GOLDEN, REPO


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "train_ref.npz"))


@pytest.fixture(scope="module")
def dataset(fx, tmp_path_factory):
    from athd.musdb import MusDBTracks
    from athd.train_data import TrainSegmentDataset
    root = tmp_path_factory.mktemp("train_tracks")
    for i, length in enumerate(fx["track_lengths"]):
        np.save(root / f"track{i}.stem.npy", R.train_track(int(length)))
    return TrainSegmentDataset(MusDBTracks(root), int(fx["segment_samples"]))


@pytest.mark.parametrize("loss", sorted(R.LOSSES))
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_restatement_matches_reference_gradients(fx, loss, family):
    a = float(fx["a"])
    assert 0.0 < a < 1e-6                          # f32 autograd of an n-term loss: a few 2^-24
    for rows, n in R.FIXTURE_SHAPES:
        est, tgt = R.FAMILIES[family](rows, n)
        assert R.clamp_margin(est, tgt) > 0.01
        mine = R.grad64(est, tgt, loss)
        want = fx[f"grad_{loss}_{family}_{rows}x{n}"].astype(np.float64)
        scale = np.abs(mine).max(axis=1)
        if n > 1000:
            mine = mine[:, ::R.LONG_STRIDE]
            assert np.all(np.abs(fx[f"gmax_{loss}_{family}_{rows}x{n}"] - scale) <= 4 * a * scale)
        assert want.shape == mine.shape
        gap = R.row_gap(want, mine, scale)
        print(f"{loss} {family} {rows}x{n}: reference f32 gradient within {gap:.3e} of the restatement (<= {4 * a:.3e})")
        assert gap <= 4 * a, (loss, family, rows, n, gap)


def test_fixture_is_small_and_seeded(fx):
    assert os.path.getsize(os.path.join(GOLDEN, "train_ref.npz")) < 200 * 1024
    assert sorted(int(v) for v in fx["track_lengths"]) == sorted(R.TRACK_LENGTHS)
    assert int(fx["segment_samples"]) == R.SEGMENT and int(fx["items_seed"]) == R.ITEMS_SEED
    assert min(fx["track_lengths"]) < R.SEGMENT                                  # a track shorter than one segment
    assert float(fx["a"]) == float(fx["a_values"].max()) and len(fx["a_cases"]) == 2 * 3 * len(R.FIXTURE_SHAPES)
    gained, swapped = fx["plan_gain"] != 1.0, fx["plan_swap"]
    assert {(bool(g), bool(s)) for g, s in zip(gained, swapped)} == {(False, False), (False, True), (True, False),
                                                                     (True, True)}


def test_items_and_plans_match_reference(fx, dataset):
    from athd.musdb import segment_index
    ds = dataset
    n = len(fx["item_prompt"])
    assert len(ds) == n == 20 and ds.index_map == segment_index([int(v) for v in fx["track_lengths"]], R.SEGMENT)
    random.seed(R.ITEMS_SEED)
    items = [ds[i] for i in range(n)]
    assert random.random() == float(fx["random_after"])
    random.seed(R.ITEMS_SEED)
    plans = [ds.draw(i) for i in range(n)]
    assert random.random() == float(fx["random_after"])
    for i, (item, plan) in enumerate(zip(items, plans)):
        assert item["mixture"].dtype == torch.float32 and item["mixture"].shape == (2, R.SEGMENT)
        assert np.array_equal(item["mixture"].numpy(), fx["item_mixture"][i]), i
        assert np.array_equal(item["target"].numpy(), fx["item_target"][i]), i
        assert (item["prompt"], item["stem_name"]) == (str(fx["item_prompt"][i]), str(fx["item_stem"][i]))
        assert (item["file_idx"], item["segment_idx"]) == (int(fx["item_file"][i]), int(fx["item_segment"][i]))
        assert (plan.start, plan.gain, plan.swap) == (int(fx["plan_start"][i]), float(fx["plan_gain"][i]),
                                                      bool(fx["plan_swap"][i])), i
        assert (plan.file_idx, plan.stem_idx, plan.segment_idx) == ds.index_map[i] and plan.prompt == item["prompt"]
        # the numpy restatement the GPU test compares the kernel with gives the reference's items too
        stems = R.train_track(int(fx["track_lengths"][plan.file_idx]))
        for key, src in (("item_mixture", 0), ("item_target", plan.stem_idx + 1)):
            assert np.array_equal(R.train_segment_ref(stems, src, plan.start, plan.gain, plan.swap, R.SEGMENT),
                                  fx[key][i]), (i, key)


def test_fixed_grid_without_augmentation_is_the_validation_dataset(dataset):
    from athd.train_data import TrainSegmentDataset
    from athd.validate import SegmentDataset
    a = TrainSegmentDataset(dataset.tracks, R.SEGMENT, random_segments=False, augment=False)
    b = SegmentDataset(dataset.tracks, R.SEGMENT)
    random.seed(4)
    mine = [a[i] for i in range(len(a))]
    state = random.getstate()
    random.seed(4)
    theirs = [b[i] for i in range(len(b))]
    assert random.getstate() == state
    for x, y in zip(mine, theirs):
        assert list(x) == list(y) and x["prompt"] == y["prompt"]
        assert torch.equal(x["mixture"], y["mixture"]) and torch.equal(x["target"], y["target"])


def test_train_epoch_rejects_before_touching_the_model():
    from athd.train import train_epoch
    args = dict(model=None, dataloader=[], optimizer=None, scaler=None, device="cuda", use_amp=False, grad_clip=1.0,
                sdr_weight=0.9, sisdr_weight=0.1, epoch=0, log_every=0)
    with pytest.raises(ValueError, match="wandb"):
        train_epoch(use_L1_cmb_loss=False, l1_sdr_weight=None, l1_weight=None, use_wandb=True, **args)


def test_modules_import_and_abi_names():
    import athd.train
    import athd.train_data
    from athd import loss, native
    assert callable(athd.train.train_epoch) and callable(loss.loss_with_grad)
    header = open(os.path.join(REPO, "include", "athd.h")).read()
    for name in ("athd_loss_grad_scratch_bytes", "athd_loss_grad_coef", "athd_loss_grad_apply",
                 "athd_gather_train_segments"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in native.EXPORTED and hasattr(native.lib, name)
    for rows, n in ((0, 5), (1, 1 << 31), ((1 << 20) + 1, 5), (3, 63), (2, 60002)):
        assert native.lib.athd_loss_grad_scratch_bytes(rows, n) == native.lib.athd_loss_rows_scratch_bytes(rows, n)
