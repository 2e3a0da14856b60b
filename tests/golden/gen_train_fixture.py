"""Generator of tests/golden/train_ref.npz: the reference's own f32 autograd gradients of `combined_loss` and
`combined_L1_sdr_loss` (`src/loss.py`) and its own training items (`MusDBStemDataset(random_segments=True,
augment=True).__getitem__`, `src/dataloader.py:86-169`) on the seeded inputs of tests/train_refs.py.  Run once by hand
where the reference checkout is available; never run by a test:

    python tests/golden/gen_train_fixture.py --reference /path/to/reference/checkout

`src/dataloader.py` imports stempeg and soundfile at its top; where they are not installed they are satisfied by
stand-ins, and stempeg's two entry points the dataset calls (`Info`, `read_stems`) always are, so that the "files" are
the seeded tracks of tests/train_refs.py handed over as float64 arrays, the dtype stempeg returns.  The dataset's
`random` is wrapped by a recorder that forwards every call to Python's global `random` and keeps the results: the plans
(start, gain, swap) are read off the reference's own draws.

The file holds arrays only:
  grad_<loss>_<family>_<rows>x<n>  float32   the reference's `est.grad` after `total.backward()` on f32 inputs, for
                                             loss in {combined (0.9 / 0.1), combined_l1 (1.0 / 0.05)}, every family of
                                             tests/validate_refs.py and (rows, n) in (3, 74), (4, 257), (5, 3002); of
                                             the last only columns 0::5 (the file stays under 200 KB), with
  gmax_<loss>_<family>_5x3002      float64   each row's largest |gradient| over ALL its columns
  a                                float64   the worst gap of those f32 gradients (all columns) to float64 autograd of
                                             the same reference functions, as a fraction of the row's largest
                                             |float64 gradient|
  a_cases, a_values                          the same figure per case
  track_lengths (2,), segment_samples, items_seed
  item_mixture, item_target (20, 2, 256) float32, item_prompt, item_stem (20,) str, item_file, item_segment (20,)
                                             `dataset[i]` for i = 0..19 in order after `random.seed(items_seed)`
  plan_start (20,) int64, plan_gain (20,) float64 (1.0 = not applied), plan_swap (20,) bool
  random_after                     float64   `random.random()` drawn after the 20 items
"""
import argparse
import importlib
import importlib.machinery
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _stand_in(name: str):
    try:
        return importlib.import_module(name)
    except ImportError:
        mod = types.ModuleType(name)
        mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
        sys.modules[name] = mod
        return mod


class _RecordingRandom:
    """Forwards to Python's global `random` and keeps (name, result) of every call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(random, name)

        def call(*args):
            out = fn(*args)
            self.calls.append((name, out))
            return out
        return call


def _gradients(ref_loss, arrays):
    import train_refs as R
    worst, cases, values = 0.0, [], []
    for loss, (w1, w2) in R.LOSSES.items():
        fn = ref_loss.combined_loss if loss == "combined" else ref_loss.combined_L1_sdr_loss
        for family in sorted(R.FAMILIES):
            for rows, n in R.FIXTURE_SHAPES:
                est, tgt = R.FAMILIES[family](rows, n)
                assert R.clamp_margin(est, tgt) > 0.01
                grads = []
                for dtype in (torch.float32, torch.float64):
                    e = est.to(dtype)[:, None, :].requires_grad_(True)       # (batch, channels, time), as it expects
                    total, _ = fn(e, tgt.to(dtype)[:, None, :], w1, w2)
                    total.backward()
                    grads.append(e.grad.double().numpy()[:, 0, :])
                g32, g64 = grads
                gap = R.row_gap(g32, g64)
                key = f"{loss}_{family}_{rows}x{n}"
                cases.append(key)
                values.append(gap)
                worst = max(worst, gap)
                if n > 1000:
                    arrays[f"gmax_{key}"] = np.abs(g32).max(axis=1)
                    g32 = g32[:, ::R.LONG_STRIDE]
                arrays[f"grad_{key}"] = g32.astype(np.float32)
                print(f"{key}: f32 autograd within {gap:.3e} of float64 autograd")
    arrays.update(a=np.array(worst), a_cases=np.array(cases), a_values=np.array(values))
    print(f"a = {worst:.3e}")


def _items(ref_dl, arrays):
    import train_refs as R
    stempeg = sys.modules["stempeg"]
    with tempfile.TemporaryDirectory() as root:
        for i in range(len(R.TRACK_LENGTHS)):
            open(os.path.join(root, f"track{i}.stem.mp4"), "wb").close()
        length_of = lambda path: R.TRACK_LENGTHS[int(os.path.basename(str(path))[5])]

        class Info:
            def __init__(self, path):
                self.n = length_of(path)

            def duration(self, _):
                return self.n / 44100.0

            def sample_rate(self, _):
                return 44100

        stempeg.Info = Info
        stempeg.read_stems = lambda path: (R.train_track(length_of(path)).astype(np.float64), 44100)
        ds = ref_dl.MusDBStemDataset(root, R.SEGMENT, random_segments=True, augment=True)
        lengths = [length_of(f) for f in ds.files]
        n_items = len(ds)
        rec = _RecordingRandom()
        ref_dl.random = rec
        random.seed(R.ITEMS_SEED)
        items, plans = [], []
        for i in range(n_items):
            rec.calls.clear()
            items.append(ds[i])
            calls = list(rec.calls)
            start = calls.pop(0)[1] if calls[0][0] == "randint" else 0
            assert calls.pop(0)[0] == "random"
            gain = calls.pop(0)[1] if calls[0][0] == "uniform" else 1.0
            name, u = calls.pop(0)
            assert name == "random" and [c[0] for c in calls] == ["choice"], calls
            plans.append((start, gain, u < 0.3))
        after = random.random()
        ref_dl.random = random
    assert items[0]["mixture"].dtype == torch.float32
    combos = {(p[1] != 1.0, p[2]) for p in plans}
    assert len(combos) == 4, f"seed {R.ITEMS_SEED} does not reach every gain / swap combination: {combos}"
    arrays.update(track_lengths=np.array(lengths), segment_samples=np.array(R.SEGMENT),
                  items_seed=np.array(R.ITEMS_SEED),
                  item_mixture=np.stack([it["mixture"].numpy() for it in items]),
                  item_target=np.stack([it["target"].numpy() for it in items]),
                  item_prompt=np.array([it["prompt"] for it in items]),
                  item_stem=np.array([it["stem_name"] for it in items]),
                  item_file=np.array([it["file_idx"] for it in items]),
                  item_segment=np.array([it["segment_idx"] for it in items]),
                  plan_start=np.array([p[0] for p in plans], dtype=np.int64),
                  plan_gain=np.array([p[1] for p in plans], dtype=np.float64),
                  plan_swap=np.array([p[2] for p in plans], dtype=bool), random_after=np.array(after))
    print(f"{n_items} items of tracks {lengths}: starts {[p[0] for p in plans]}")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="directory of the reference checkout (holds src/)")
    ap.add_argument("--out", default=os.path.join(HERE, "train_ref.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    _stand_in("stempeg")
    _stand_in("soundfile")
    ref_loss = importlib.import_module("src.loss")
    ref_dl = importlib.import_module("src.dataloader")

    arrays = {}
    _gradients(ref_loss, arrays)
    _items(ref_dl, arrays)
    np.savez_compressed(args.out, **arrays)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out}: {size} bytes")
    assert size < 200 * 1024, size
    return 0


if __name__ == "__main__":
    sys.exit(main())
