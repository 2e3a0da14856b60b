"""Scoring a checkpoint on the validation split: the reference's `validate()` and its `val_dataset`.

Mirrors `src/train.py` / `src/dataloader.py`:
  * `SegmentDataset`  <- `MusDBStemDataset(random_segments=False, augment=False)` (`train.py:435-441`,
                         `dataloader.py:37-169`): the index map, `__getitem__`'s dict, and a device path that uploads a
                         track's (5, L, 2) array once and cuts mixtures / targets with `athd_gather_segments`
  * `validate`        <- `validate()` (`train.py:132-202`): `loss`, `sdr`, `sisdr` = the mean over batches of the batch
                         means, `sdr/{stem}` = the mean over that stem's items
  * `main`            <- the validation part of `train()` (`train.py:308-345, 435-473, 543-558`) as a CLI

Every number `validate` returns is a function of the per-item row table of athd/loss.py, so items run in whatever
grouping suits the device (one track resident at a time, `max_batch` segments per forward, with `prompts="first"` one
encoder pass per segment for all of its stems) and are regrouped into the reference's batches afterwards.

One deliberate deviation: with `pct_test < 1` the reference builds `Subset(train_dataset, val_idxs)`
(`train.py:452`), a subset of the TRAINING dataset; the CLI takes `torch.randperm(len(val_dataset))[:int(len *
pct_test)]` on the validation dataset.
"""
from __future__ import annotations

import argparse
import json
import random
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import native
from .loss import SDR, combined_from_rows, combined_l1_from_rows, loss_rows
from .musdb import STEM_NAMES, STEM_PROMPTS, MusDBTracks, extract_segment, segment_index


class SegmentDataset:
    """The reference's `val_dataset`: every (file, stem, segment) of a split in index-map order."""

    def __init__(self, tracks: MusDBTracks, segment_samples: int):
        self.tracks = tracks
        self.segment_samples = int(segment_samples)
        self.stem_names = list(STEM_NAMES)
        self.index_map = segment_index(tracks.lengths(), self.segment_samples)
        self._host = (None, None)          # (file_idx, (5, L, 2) array): one track at a time
        self._dev = (None, None)           # (file_idx, (5, L, 2) device tensor): one track at a time

    def __len__(self) -> int:
        return len(self.index_map)

    def _stems(self, file_idx: int) -> np.ndarray:
        if self._host[0] != file_idx:
            self._host = (None, None)
            self._host = (file_idx, self.tracks.load_stems(file_idx))
        return self._host[1]

    def __getitem__(self, idx: int) -> Dict:
        """`dataloader.py:136-169` with augment=False: draws one prompt from Python's global `random`."""
        file_idx, stem_idx, seg_idx = self.index_map[idx]
        stems = extract_segment(self._stems(file_idx), seg_idx, self.segment_samples)
        return {"mixture": torch.from_numpy(np.ascontiguousarray(stems[0].T)).float(),
                "target": torch.from_numpy(np.ascontiguousarray(stems[stem_idx + 1].T)).float(),
                "prompt": random.choice(STEM_PROMPTS[self.stem_names[stem_idx]]),
                "stem_name": self.stem_names[stem_idx], "file_idx": file_idx, "segment_idx": seg_idx}

    def device_stems(self, file_idx: int, device) -> torch.Tensor:
        """(5, L, 2) float32 of track `file_idx` on `device`, uploaded once; the previous track is released."""
        device = torch.device(device)
        if self._dev[0] != file_idx or self._dev[1].device != device:
            self._dev = (None, None)
            self._dev = (file_idx, torch.from_numpy(np.ascontiguousarray(self._stems(file_idx))).to(device))
        return self._dev[1]

    def gather(self, file_idx: int, src: Sequence[int], seg: Sequence[int], device) -> torch.Tensor:
        """(rows, 2, segment_samples) on `device`: row r = source src[r] (0 = mixture, stem + 1 = a stem) and segment
        seg[r] of track `file_idx`, zero-padded past the track's end (athd_gather_segments on the current stream)."""
        stems = self.device_stems(file_idx, device)
        return gather_segments(stems, src, seg, self.segment_samples)


def gather_segments(stems: torch.Tensor, src: Sequence[int], seg: Sequence[int], segment_samples: int) -> torch.Tensor:
    """`athd_gather_segments`: stems (n_src, L, 2) float32 on the device -> (rows, 2, segment_samples)."""
    if stems.dim() != 3 or stems.shape[2] != 2 or stems.dtype != torch.float32 or not stems.is_contiguous() \
            or stems.device.type != "cuda":
        raise ValueError("stems must be a contiguous float32 (n_src, L, 2) device tensor")
    rows = len(src)
    if rows == 0 or len(seg) != rows:
        raise ValueError("src and seg must be non-empty and of equal length")
    n_src, length = int(stems.shape[0]), int(stems.shape[1])
    if min(src) < 0 or max(src) >= n_src or min(seg) < 0:
        raise ValueError(f"src must lie in [0, {n_src}) and seg be non-negative")
    src_d = torch.tensor(list(src), dtype=torch.int32).to(stems.device)
    seg_d = torch.tensor(list(seg), dtype=torch.int64).to(stems.device)
    out = torch.empty((rows, 2, int(segment_samples)), dtype=torch.float32, device=stems.device)
    rc = native.lib.athd_gather_segments(stems.data_ptr(), n_src, length, src_d.data_ptr(), seg_d.data_ptr(), rows,
                                         int(segment_samples), out.data_ptr(),
                                         torch.cuda.current_stream(stems.device).cuda_stream)
    if rc != 0:
        raise native.AthdError(f"athd_gather_segments failed ({rc})")
    return out


def _weights(use_L1_cmb_loss, l1_sdr_weight, l1_weight, sdr_weight, sisdr_weight):
    """`train.py:154-164`."""
    if use_L1_cmb_loss:
        if l1_weight is None:
            raise ValueError("l1_weight must be provided when using L1 combination loss.")
        return l1_sdr_weight, l1_weight
    return sdr_weight, sisdr_weight


def reduce_rows(table: np.ndarray, stem_names: Sequence[str], batch_size: int, use_L1_cmb_loss: bool, weight1: float,
                weight2: float) -> Dict[str, float]:
    """The bookkeeping of `train.py:147-202` on the row table (N, 4) of the items in loader order: batches are
    consecutive runs of `batch_size` rows, the last one ragged."""
    loss_function = combined_l1_from_rows if use_L1_cmb_loss else combined_from_rows
    total_loss = total_sdr = total_sisdr = 0.0
    num_batches = 0
    for b0 in range(0, len(table), batch_size):
        metrics = loss_function(table[b0:b0 + batch_size], weight1, weight2)
        total_loss += metrics["loss/total"]
        total_sdr += metrics["metrics/sdr"]
        total_sisdr += metrics["metrics/sisdr"]
        num_batches += 1
    out = {"loss": total_loss / num_batches, "sdr": total_sdr / num_batches, "sisdr": total_sisdr / num_batches}
    for name in STEM_PROMPTS:
        vals = [float(table[i, SDR]) for i, s in enumerate(stem_names) if s == name]
        if vals:
            out[f"sdr/{name}"] = sum(vals) / len(vals)
    return out


@torch.no_grad()
def item_rows(model, dataset: SegmentDataset, indices: Sequence[int], prompts="random",
              max_batch: int = 64) -> torch.Tensor:
    """(len(indices), 4) float64 device row table {sdr, sisdr, new_sdr, l1} of the model's estimate for every item.
    prompts="random": one `random.choice` per item in the order of `indices` (the draws of the reference's loader at
    num_workers=0), items through `model.forward`.  prompts="first": each stem's first prompt, items grouped by
    (file, segment) through `model.forward_prompts`."""
    if prompts not in ("random", "first"):
        raise ValueError("prompts must be 'random' or 'first'")
    if max_batch < 1:
        raise ValueError("max_batch must be positive")
    items = [dataset.index_map[int(i)] for i in indices]
    names = dataset.stem_names
    if prompts == "random":
        text = [random.choice(STEM_PROMPTS[names[si]]) for _, si, _ in items]
    else:
        firsts = [STEM_PROMPTS[s][0] for s in names]
    if model.device is None:
        model.to("cuda")
    dev = model.device
    table = torch.empty((len(items), 4), dtype=torch.float64, device=dev)
    by_file: Dict[int, List[int]] = {}
    for pos, (fi, _, _) in enumerate(items):
        by_file.setdefault(fi, []).append(pos)
    for fi, positions in by_file.items():                     # one track on the device at a time
        if prompts == "random":
            for b0 in range(0, len(positions), max_batch):
                pos = positions[b0:b0 + max_batch]
                seg = [items[p][2] for p in pos]
                mixture = dataset.gather(fi, [0] * len(pos), seg, dev)
                target = dataset.gather(fi, [items[p][1] + 1 for p in pos], seg, dev)
                estimated = model.forward(mixture, [text[p] for p in pos])
                table[torch.tensor(pos, device=dev)] = loss_rows(estimated, target)
        else:
            segs = sorted({items[p][2] for p in positions})
            for b0 in range(0, len(segs), max_batch):
                chunk = segs[b0:b0 + max_batch]
                where = {s: j for j, s in enumerate(chunk)}
                pos = [p for p in positions if items[p][2] in where]
                mixture = dataset.gather(fi, [0] * len(chunk), chunk, dev)
                target = dataset.gather(fi, [items[p][1] + 1 for p in pos], [items[p][2] for p in pos], dev)
                out = model.forward_prompts(mixture, firsts)                              # (segments, 4, 2, S)
                pick = torch.tensor([where[items[p][2]] * len(firsts) + items[p][1] for p in pos], device=dev)
                estimated = out.reshape(len(chunk) * len(firsts), 2, -1)[pick]
                table[torch.tensor(pos, device=dev)] = loss_rows(estimated, target)
    return table


@torch.no_grad()
def validate(model, dataset: SegmentDataset, batch_size: int = 8, indices: Optional[Sequence[int]] = None,
             use_L1_cmb_loss: bool = False, l1_sdr_weight: Optional[float] = None, l1_weight: Optional[float] = None,
             sdr_weight: float = 0.9, sisdr_weight: float = 0.1, prompts="random",
             max_batch: int = 64) -> Dict[str, float]:
    """`validate()` of `src/train.py:132-202` over `dataset` (or its items `indices`, in that order; repeats
    allowed) with the reference's batches of `batch_size`: {"loss", "sdr", "sisdr", "sdr/{stem}"}."""
    model.eval()
    weight1, weight2 = _weights(use_L1_cmb_loss, l1_sdr_weight, l1_weight, sdr_weight, sisdr_weight)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    indices = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    if not indices:
        raise ValueError("validate: no items")
    table = item_rows(model, dataset, indices, prompts, max_batch).cpu().numpy()      # one device-to-host copy
    stem_names = [dataset.stem_names[dataset.index_map[i][1]] for i in indices]
    return reduce_rows(table, stem_names, batch_size, use_L1_cmb_loss, weight1, weight2)


def main(argv=None, model=None) -> int:
    """`python -m athd.validate --checkpoint PATH [--config config.yaml] [--pct-test F] [--seed K] [--prompts
    random|first] [--dtype bf16|f32] [--output FILE.json]`.  `model`: an already loaded model to score instead of
    `load_model(--checkpoint)` (for callers that hold one)."""
    ap = argparse.ArgumentParser(prog="python -m athd.validate",
                                 description="Score a checkpoint on the validation split (src/train.py validate()).")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--config", default="config.yaml")
    ap.add_argument("--pct-test", type=float, default=None, help="overrides data.pct_test")
    ap.add_argument("--seed", type=int, default=None, help="seeds Python's random (prompts) and torch (the subset)")
    ap.add_argument("--prompts", choices=("random", "first"), default="random")
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--output", default=None, help="write the result dict as JSON")
    args = ap.parse_args(argv)

    from .inference import load_config, load_model
    cfg = load_config(args.config)
    data_cfg, training_cfg = cfg.get("data", {}), cfg.get("training", {})
    test_dir = data_cfg.get("test_dir", "../data/test")
    sample_rate = data_cfg.get("sample_rate", 44100)
    segment_seconds = data_cfg.get("segment_seconds", 6.0)
    pct_test = data_cfg.get("pct_test", 1.0) if args.pct_test is None else args.pct_test
    batch_size = training_cfg.get("batch_size", 4)
    use_L1_cmb_loss = training_cfg.get("use_L1_comb_loss", False)
    l1_cfg, w_cfg = training_cfg.get("L1_comb_loss", {}), training_cfg.get("loss_weights", {})
    segment_samples = int(sample_rate * segment_seconds)

    if args.seed is not None:
        random.seed(args.seed)
        torch.manual_seed(args.seed)
    dataset = SegmentDataset(MusDBTracks(test_dir, sample_rate=sample_rate), segment_samples)
    print(f"Found {len(dataset.tracks)} tracks, total dataset items: {len(dataset)}")
    indices = None
    if 0.0 < pct_test < 1.0:
        indices = torch.randperm(len(dataset))[:int(len(dataset) * pct_test)].tolist()
    if model is None:
        model = load_model(args.checkpoint, "cuda", dtype=args.dtype)
    val_metrics = validate(model, dataset, batch_size=batch_size, indices=indices, use_L1_cmb_loss=use_L1_cmb_loss,
                           l1_sdr_weight=l1_cfg.get("sdr_weight", 1.0), l1_weight=l1_cfg.get("l1_weight", 0.05),
                           sdr_weight=w_cfg.get("sdr", 0.9), sisdr_weight=w_cfg.get("sisdr", 0.1),
                           prompts=args.prompts)
    print(f"Val - Loss: {val_metrics['loss']:.4f}, SDR: {val_metrics['sdr']:.2f} dB")
    for stem_name in STEM_PROMPTS:
        if f"sdr/{stem_name}" in val_metrics:
            print(f"  {stem_name}: {val_metrics[f'sdr/{stem_name}']:.2f} dB")
    if args.output:
        with open(args.output, "w") as f:
            json.dump(val_metrics, f, indent=2)
    return 0


if __name__ == "__main__":
    sys.exit(main())
