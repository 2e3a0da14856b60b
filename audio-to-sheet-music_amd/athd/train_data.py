"""Training batches: the reference's `train_dataset`, cut, gained and channel-swapped on the device.

Mirrors `src/dataloader.py`:
  * `TrainSegmentDataset`     <- `MusDBStemDataset(random_segments=True, augment=True)` (`train.py:425-433`,
                                 `dataloader.py:86-169`): the index map of `SegmentDataset`, `__getitem__`'s dict, and
                                 the draws of Python's global `random` in the reference's order
  * `draw`                    <- the random part of `__getitem__` alone: a plan (file, stem, start, gain, swap, prompt)
                                 that touches no audio
  * `gather`                  <- the audio part for any number of plans of one track: mixtures and targets in one
                                 launch of `athd_gather_train_segments` each, from the track uploaded once
  * `gather_train_segments`   <- the launch itself

The reference multiplies the float64 array that stempeg returns by the gain and then calls `.float()`
(`dataloader.py:123-134, 152-153`).  Tracks here are float32 (`MusDBTracks.load_stems`), so the fp64 product rounded once
is bit-equal to the reference whenever its samples are f32-representable, which every PCM file qualifies for
(DESIGN.md §4); `__getitem__` (host) and `gather` (device) both compute `(float)((double)x * gain)`.
"""
from __future__ import annotations

import random
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from . import native
from .musdb import STEM_PROMPTS, MusDBTracks
from .validate import SegmentDataset


class Plan(NamedTuple):
    """What `__getitem__` decides before it touches audio.  `gain` is 1.0 and `swap` False where the reference leaves
    the arrays alone."""
    file_idx: int
    stem_idx: int
    segment_idx: int
    start: int
    gain: float
    swap: bool
    prompt: str


class TrainSegmentDataset(SegmentDataset):
    """The reference's `train_dataset`: the index map of `SegmentDataset`; each item a random window of its track
    (`random_segments`) with a random gain and channel swap (`augment`)."""

    def __init__(self, tracks: MusDBTracks, segment_samples: int, random_segments: bool = True, augment: bool = True):
        super().__init__(tracks, segment_samples)
        self.random_segments = bool(random_segments)
        self.augment = bool(augment)
        self._lengths = list(tracks.lengths())

    def draw(self, idx: int) -> Plan:
        """The draws of `__getitem__` (`dataloader.py:136-169`) from Python's global `random`, in its order:
        `randint(0, total - seg)` only when random_segments and total > seg (`:90-100`); `random() < 0.5` and then
        `uniform(0.7, 1.3)`; `random() < 0.3` (`:123-134`); the prompt's `choice` (`:160`)."""
        file_idx, stem_idx, seg_idx = self.index_map[idx]
        total, seg = self._lengths[file_idx], self.segment_samples
        if self.random_segments:
            start = random.randint(0, total - seg) if total > seg else 0
        else:
            start = seg_idx * seg
        gain, swap = 1.0, False
        if self.augment:
            if random.random() < 0.5:
                gain = random.uniform(0.7, 1.3)
            swap = random.random() < 0.3
        prompt = random.choice(STEM_PROMPTS[self.stem_names[stem_idx]])
        return Plan(file_idx, stem_idx, seg_idx, start, gain, swap, prompt)

    def cut(self, plan: Plan, src: int) -> torch.Tensor:
        """(2, segment_samples) float32 on the host: source `src` of the plan's track, windowed, gained and swapped."""
        stems = self._stems(plan.file_idx)
        x = stems[src, plan.start:plan.start + self.segment_samples, :]
        x = np.pad(x, ((0, self.segment_samples - x.shape[0]), (0, 0)), mode="constant")
        if plan.gain != 1.0:
            x = (x.astype(np.float64) * plan.gain).astype(np.float32)
        if plan.swap:
            x = x[:, ::-1]
        return torch.from_numpy(np.ascontiguousarray(x.T, dtype=np.float32))

    def __getitem__(self, idx: int) -> Dict:
        plan = self.draw(idx)
        return {"mixture": self.cut(plan, 0), "target": self.cut(plan, plan.stem_idx + 1), "prompt": plan.prompt,
                "stem_name": self.stem_names[plan.stem_idx], "file_idx": plan.file_idx,
                "segment_idx": plan.segment_idx}

    def gather(self, file_idx: int, plans: Sequence[Plan], device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mixtures, targets), each (len(plans), 2, segment_samples) on `device`, for plans of track `file_idx`: one
        launch of athd_gather_train_segments each on the current stream, the track uploaded once (`device_stems`)."""
        if any(p.file_idx != file_idx for p in plans):
            raise ValueError("gather: every plan must belong to track file_idx")
        stems = self.device_stems(file_idx, device)
        start, gain, swap = [p.start for p in plans], [p.gain for p in plans], [p.swap for p in plans]
        mixtures = gather_train_segments(stems, [0] * len(plans), start, gain, swap, self.segment_samples)
        targets = gather_train_segments(stems, [p.stem_idx + 1 for p in plans], start, gain, swap, self.segment_samples)
        return mixtures, targets

    def batch(self, indices: Sequence[int], device) -> Dict:
        """The collated batch of `collate_fn` (`dataloader.py:172-179`) for `indices`, drawn in that order and cut on
        the device: {"mixture", "target" (len, 2, S) on `device`, "prompt", "stem_name"}."""
        plans = [self.draw(int(i)) for i in indices]
        mixture = torch.empty((len(plans), 2, self.segment_samples), dtype=torch.float32, device=device)
        target = torch.empty_like(mixture)
        by_file: Dict[int, List[int]] = {}
        for pos, p in enumerate(plans):
            by_file.setdefault(p.file_idx, []).append(pos)
        for fi, pos in by_file.items():
            m, t = self.gather(fi, [plans[k] for k in pos], device)
            at = torch.tensor(pos, device=m.device)
            mixture[at], target[at] = m, t
        return {"mixture": mixture, "target": target, "prompt": [p.prompt for p in plans],
                "stem_name": [self.stem_names[p.stem_idx] for p in plans]}


def gather_train_segments(stems: torch.Tensor, src: Sequence[int], start: Sequence[int], gain: Sequence[float],
                          swap: Sequence[bool], segment_samples: int) -> torch.Tensor:
    """`athd_gather_train_segments`: stems (n_src, L, 2) float32 on the device -> (rows, 2, segment_samples); row r is
    source src[r] from sample start[r], times gain[r] in fp64 rounded once, channels exchanged where swap[r]."""
    if stems.dim() != 3 or stems.shape[2] != 2 or stems.dtype != torch.float32 or not stems.is_contiguous() \
            or stems.device.type != "cuda":
        raise ValueError("stems must be a contiguous float32 (n_src, L, 2) device tensor")
    rows = len(src)
    if rows == 0 or len(start) != rows or len(gain) != rows or len(swap) != rows:
        raise ValueError("src, start, gain and swap must be non-empty and of equal length")
    n_src, length = int(stems.shape[0]), int(stems.shape[1])
    if min(src) < 0 or max(src) >= n_src or min(start) < 0:
        raise ValueError(f"src must lie in [0, {n_src}) and start be non-negative")
    dev = stems.device
    src_d = torch.tensor(list(src), dtype=torch.int32).to(dev)
    start_d = torch.tensor(list(start), dtype=torch.int64).to(dev)
    gain_d = torch.tensor(list(gain), dtype=torch.float64).to(dev)
    swap_d = torch.tensor([1 if s else 0 for s in swap], dtype=torch.uint8).to(dev)
    out = torch.empty((rows, 2, int(segment_samples)), dtype=torch.float32, device=dev)
    rc = native.lib.athd_gather_train_segments(stems.data_ptr(), n_src, length, src_d.data_ptr(), start_d.data_ptr(),
                                               gain_d.data_ptr(), swap_d.data_ptr(), rows, int(segment_samples),
                                               out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise native.AthdError(f"athd_gather_train_segments failed ({rc})")
    return out
