"""Float64 restatements for the training ends (athd/loss.py `loss_with_grad`, athd/train_data.py, athd/train.py) and the
seeded inputs of tests/test_train_refs.py, tests/test_gpu_train.py and tests/golden/gen_train_fixture.py; a helper
module, not a test file.

  * `total64` / `grad64`: the two combined losses of `src/loss.py:90-162` written out in torch float64, the gradient by
    torch autograd.  Nothing here uses the closed form the kernel evaluates (include/athd.h), so the kernel's algebra
    is checked against something independent.
  * `train_segment_ref`: the window, gain and channel swap of `src/dataloader.py:86-134` in numpy float64, rounded once.
  * `train_epoch_ref`: the loop of `src/train.py:23-129` with the loss above in place of the library's.
  * the input families of tests/validate_refs.py (imported, not edited) and the fixture's tracks.
"""
import numpy as np
import torch

from validate_refs import DELTA, FAMILIES, clamp_margin  # noqa: F401  (re-exported for the tests)

LOSSES = {"combined": (0.9, 0.1), "combined_l1": (1.0, 0.05)}        # the reference's default weights
FIXTURE_SHAPES = [(3, 74), (4, 257), (5, 3002)]
LONG_STRIDE = 5            # the fixture keeps columns 0::5 of the (5, 3002) gradients (and each row's largest |g|)
TRACK_LENGTHS = (1000, 100)
SEGMENT = 256
ITEMS_SEED = 1


# ---------------------------------------------------------------------------------------------- the losses
def total64(est: torch.Tensor, tgt: torch.Tensor, kind: str, w1: float, w2: float) -> torch.Tensor:
    """`combined_loss` (kind "combined": w1 sdr_loss + w2 sisdr_loss) or `combined_L1_sdr_loss` ("combined_l1":
    w1 sdr_loss + w2 l1) in float64 on est's device, differentiable by autograd."""
    e = est.double().reshape(est.shape[0], -1)
    t = tgt.double().reshape(tgt.shape[0], -1)
    sdr = 10 * torch.log10(((t ** 2).sum(-1) + DELTA) / (((t - e) ** 2).sum(-1) + DELTA))
    sdr_loss = -sdr.clamp(min=-30, max=30).mean()
    if kind == "combined_l1":
        return w1 * sdr_loss + w2 * (e - t).abs().mean()
    assert kind == "combined", kind
    ec = e - e.mean(-1, keepdim=True)
    tc = t - t.mean(-1, keepdim=True)
    s = ((ec * tc).sum(-1, keepdim=True) / ((tc ** 2).sum(-1, keepdim=True) + DELTA)) * tc
    sisdr = 10 * torch.log10(((s ** 2).sum(-1) + DELTA) / (((ec - s) ** 2).sum(-1) + DELTA))
    return w1 * sdr_loss + w2 * (-sisdr.clamp(min=-30, max=30).mean())


def grad64(est, tgt, kind: str, w1=None, w2=None, upstream: float = 1.0) -> np.ndarray:
    """d (upstream * total64) / d est as a float64 array of est's shape (autograd on the CPU)."""
    d1, d2 = LOSSES[kind]
    e = torch.as_tensor(est).detach().cpu().double().requires_grad_(True)
    total = total64(e, torch.as_tensor(tgt).detach().cpu(), kind, d1 if w1 is None else w1, d2 if w2 is None else w2)
    (total * upstream).backward()
    return e.grad.numpy()


def row_gap(got: np.ndarray, want: np.ndarray, scale: np.ndarray = None) -> float:
    """The worst |got - want| of any row as a fraction of that row's largest |want| (or of `scale`, one value per
    row); rows whose scale is zero must be exactly zero in `got` and do not enter."""
    got, want = np.asarray(got, np.float64).reshape(len(got), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    scale = np.abs(want).max(axis=1) if scale is None else np.asarray(scale, np.float64)
    worst = 0.0
    for r in range(len(want)):
        if scale[r] == 0.0:
            assert not np.any(got[r]), f"row {r}: the float64 gradient is zero, the result is not"
        else:
            worst = max(worst, float(np.abs(got[r] - want[r]).max() / scale[r]))
    return worst


def with_ties(est: torch.Tensor, tgt: torch.Tensor):
    """est with every third element of its row 0 set to the target's: sign(0) = 0 under the L1 term."""
    e = est.clone()
    e[0, ::3] = tgt[0, ::3]
    return e, tgt


# ------------------------------------------------------------------------------------------------ segments
def train_segment_ref(stems: np.ndarray, src: int, start: int, gain: float, swap: bool, seg: int) -> np.ndarray:
    """(2, seg) float32: frames [start, start + seg) of stems[src] (zero past the end), times gain in float64 rounded
    once, channels exchanged if swap; a src outside the stems or a negative start gives zeros."""
    out = np.zeros((seg, 2), dtype=np.float64)
    if 0 <= src < stems.shape[0] and start >= 0:
        x = stems[src, start:start + seg, :].astype(np.float64)
        out[:x.shape[0]] = x * gain
    if swap:
        out = out[:, ::-1]
    return np.ascontiguousarray(out.T).astype(np.float32)


def train_track(length: int) -> np.ndarray:
    """The fixture's track of `length` frames: (5, length, 2) float32, seeded by the length."""
    g = torch.Generator().manual_seed(7700 + length)
    return (0.3 * torch.randn(5, length, 2, generator=g)).numpy()


# --------------------------------------------------------------------------------------------- the step loop
def train_epoch_ref(model, batches, optimizer, kind: str, w1: float, w2: float, grad_clip: float) -> dict:
    """`train_epoch` without AMP, the loss and its gradient by `total64` and autograd; the returned means are those of
    the float64 batch metrics."""
    model.train()
    tot = {"loss": 0.0, "sdr": 0.0, "sisdr": 0.0}
    for batch in batches:
        optimizer.zero_grad()
        est = model(batch["mixture"], batch["prompt"])
        loss = total64(est, batch["target"], kind, w1, w2)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
        optimizer.step()
        with torch.no_grad():
            tot["loss"] += float(loss)
            tot["sdr"] += -float(total64(est, batch["target"], "combined", 1.0, 0.0))
            tot["sisdr"] += -float(total64(est, batch["target"], "combined", 0.0, 1.0))
    return {k: v / len(batches) for k, v in tot.items()}
