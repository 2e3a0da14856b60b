"""Float64 restatements of the reference's `src/loss.py` row metrics and of `validate()` (`src/train.py:132-202`), and
the seeded inputs of tests/test_validate_refs.py, tests/test_gpu_validate.py and tests/golden/gen_loss_fixture.py; a
helper module, not a test file.

Row table columns (athd/loss.py, `athd_loss_rows`): {sdr, sisdr, new_sdr, l1} per row of (rows, n):
  sdr     = clamp(10 log10((sum t^2 + 1e-8) / (sum (t-e)^2 + 1e-8)), -30, 30)
  sisdr   = zero-mean e and t, a = <e,t> / (|t|^2 + 1e-8), clamp(10 log10((|a t|^2 + 1e-8) / (|e - a t|^2 + 1e-8)))
  new_sdr = the ratio of sdr, not clamped
  l1      = mean |e - t|
"""
import numpy as np
import torch

SDR, SISDR, NEW_SDR, L1 = 0, 1, 2, 3
DELTA = 1e-8
SNRS_DB = (25.0, 10.0, 0.0, -10.0, -25.0)
STEM_NAMES = ("drums", "bass", "other", "vocals")
COMBINED_KEYS = ("loss/total", "loss/sdr", "loss/sisdr", "metrics/sdr", "metrics/sisdr", "metrics/new_sdr")
COMBINED_L1_KEYS = COMBINED_KEYS[:5]


# ---------------------------------------------------------------------------------------------- restatements
def _rows64(est, tgt):
    e = torch.as_tensor(est).double().reshape(len(est), -1)
    t = torch.as_tensor(tgt).double().reshape(len(tgt), -1)
    raw = 10 * torch.log10(((t ** 2).sum(-1) + DELTA) / (((t - e) ** 2).sum(-1) + DELTA))
    ec = e - e.mean(-1, keepdim=True)
    tc = t - t.mean(-1, keepdim=True)
    a = (ec * tc).sum(-1, keepdim=True) / ((tc ** 2).sum(-1, keepdim=True) + DELTA)
    s = a * tc
    si = 10 * torch.log10(((s ** 2).sum(-1) + DELTA) / (((ec - s) ** 2).sum(-1) + DELTA))
    return raw, si, (e - t).abs().mean(-1)


def loss_rows_ref(est, tgt) -> np.ndarray:
    """(rows, 4) float64 from est / tgt of equal shape (rows, ...), every operation in float64."""
    raw, si, l1 = _rows64(est, tgt)
    return torch.stack([raw.clamp(-30, 30), si.clamp(-30, 30), raw, l1], dim=1).numpy()


def clamp_margin(est, tgt) -> float:
    """The smallest distance in dB of a row's unclamped SDR or SI-SDR from +-30 (the clamp decision is in doubt
    below the tolerance of a comparison)."""
    raw, si, _ = _rows64(est, tgt)
    return float(torch.cat([raw, si]).abs().sub(30.0).abs().min())


def combined_loss_ref(table: np.ndarray, sdr_weight: float = 0.9, sisdr_weight: float = 0.1):
    """(total, metrics) of `combined_loss` (`src/loss.py:90-127`) from the row table of one batch."""
    sdr, sisdr = -float(table[:, SDR].mean()), -float(table[:, SISDR].mean())
    total = sdr_weight * sdr + sisdr_weight * sisdr
    return total, {"loss/total": total, "loss/sdr": sdr, "loss/sisdr": sisdr, "metrics/sdr": -sdr,
                   "metrics/sisdr": -sisdr, "metrics/new_sdr": float(table[:, NEW_SDR].mean())}


def combined_l1_ref(table: np.ndarray, sdr_weight: float = 1.0, l1_weight: float = 0.05):
    """(total, metrics) of `combined_L1_sdr_loss` (`src/loss.py:130-162`): L1 over the batch = the mean of the rows'
    means, as rows have equal length."""
    sdr, sisdr = -float(table[:, SDR].mean()), -float(table[:, SISDR].mean())
    total = sdr_weight * sdr + l1_weight * float(table[:, L1].mean())
    return total, {"loss/total": total, "loss/sdr": sdr, "loss/sisdr": sisdr, "metrics/sdr": -sdr,
                   "metrics/sisdr": -sisdr}


def validate_ref(forward, batches, use_L1_cmb_loss=False, l1_sdr_weight=None, l1_weight=None, sdr_weight=0.9,
                 sisdr_weight=0.1) -> dict:
    """`validate()` of `src/train.py:132-202` in float64: `forward(mixture, prompts)` per batch of `batches` (dicts
    with mixture, target, prompt, stem_name); loss / sdr / sisdr = the mean over batches of the batch means."""
    if use_L1_cmb_loss:
        if l1_weight is None:
            raise ValueError("l1_weight must be provided when using L1 combination loss.")
        fn, w1, w2 = combined_l1_ref, l1_sdr_weight, l1_weight
    else:
        fn, w1, w2 = combined_loss_ref, sdr_weight, sisdr_weight
    tot = {"loss": 0.0, "sdr": 0.0, "sisdr": 0.0}
    stems = {s: [0.0, 0] for s in STEM_NAMES}
    for batch in batches:
        est = forward(batch["mixture"], batch["prompt"])
        table = loss_rows_ref(torch.as_tensor(est).cpu(), torch.as_tensor(batch["target"]).cpu())
        _, m = fn(table, w1, w2)
        tot["loss"] += m["loss/total"]
        tot["sdr"] += m["metrics/sdr"]
        tot["sisdr"] += m["metrics/sisdr"]
        for i, s in enumerate(batch["stem_name"]):
            stems[s][0] += float(table[i, SDR])
            stems[s][1] += 1
    out = {k: v / len(batches) for k, v in tot.items()}
    for s, (v, c) in stems.items():
        if c:
            out[f"sdr/{s}"] = v / c
    return out


# ---------------------------------------------------------------------------------------------------- inputs
def _gen(seed, *shape):
    return torch.Generator().manual_seed(seed * 1000003 + sum(int(s) * (31 ** i) for i, s in enumerate(shape)))


def snr_family(rows: int, n: int, seed: int = 0):
    """t = 0.1 randn, e = t + noise scaled to the SNRs 25, 10, 0, -10, -25 dB (cycled over the rows)."""
    g = _gen(seed + 1, rows, n)
    t = 0.1 * torch.randn(rows, n, generator=g)
    z = torch.randn(rows, n, generator=g)
    snr = torch.tensor([SNRS_DB[i % len(SNRS_DB)] for i in range(rows)])
    scale = t.norm(dim=1) / z.norm(dim=1).clamp_min(1e-30) * 10 ** (-snr / 20)
    return t + z * scale[:, None], t


def dc_family(rows: int, n: int, seed: int = 0):
    """t = 0.01 randn + 0.5, e = 0.9 t + 0.001 randn + {0, 0.2, -0.4} (cycled over the rows)."""
    g = _gen(seed + 2, rows, n)
    t = 0.01 * torch.randn(rows, n, generator=g) + 0.5
    off = torch.tensor([(0.0, 0.2, -0.4)[i % 3] for i in range(rows)])
    return 0.9 * t + 0.001 * torch.randn(rows, n, generator=g) + off[:, None], t


def clamp_family(rows: int, n: int, seed: int = 0):
    """Rows cycle through e = t, e = -40 t, e = t = 0, e = 0 and e = 2 t (t = 0.1 randn)."""
    g = _gen(seed + 3, rows, n)
    t = 0.1 * torch.randn(rows, n, generator=g)
    e = t.clone()
    for i in range(rows):
        k = i % 5
        if k == 1:
            e[i] = -40.0 * t[i]
        elif k == 2:
            e[i] = 0.0
            t[i] = 0.0
        elif k == 3:
            e[i] = 0.0
        elif k == 4:
            e[i] = 2.0 * t[i]
    return e, t


FAMILIES = {"snr": snr_family, "dc": dc_family, "clamp": clamp_family}


def loss_fixture_inputs():
    """The fixture's loss inputs: est, target (5, 2, 750), one row per SNR."""
    e, t = snr_family(5, 1500, seed=11)
    return e.reshape(5, 2, 750), t.reshape(5, 2, 750)


VAL_ITEMS, VAL_BATCH, VAL_T = 16, 3, 256


def validate_fixture_inputs():
    """16 items for the reference's `validate`: mixture, target (16, 2, 256), stem names, prompts, and the stub model's
    noise bank (16, 2, 256).  The stub returns 0.8 mixture + 0.05 noise, so targets are mixtures scaled per item to
    spread the SDRs."""
    g = _gen(21, VAL_ITEMS, VAL_T)
    mixture = torch.randn(VAL_ITEMS, 2, VAL_T, generator=g)
    gain = torch.linspace(0.5, 1.1, VAL_ITEMS)[:, None, None]
    target = gain * mixture + 0.02 * torch.randn(VAL_ITEMS, 2, VAL_T, generator=g)
    noise = torch.randn(VAL_ITEMS, 2, VAL_T, generator=g)
    stems = [STEM_NAMES[(i * 3 + i // 5) % 4] for i in range(VAL_ITEMS)]
    return mixture, target, noise, stems


def make_batches(mixture, target, stems, batch_size=VAL_BATCH):
    """The loader's batches (`collate_fn`, `dataloader.py:172-179`): consecutive runs, the last one ragged."""
    mixture, target = torch.as_tensor(mixture), torch.as_tensor(target)
    return [{"mixture": mixture[i:i + batch_size], "target": target[i:i + batch_size],
             "prompt": list(stems[i:i + batch_size]), "stem_name": list(stems[i:i + batch_size])}
            for i in range(0, len(stems), batch_size)]


class StubModel:
    """A callable with `.eval()`: call k returns 0.8 mixture + 0.05 noise[rows of call k] (rows handed out in order;
    `.eval()` rewinds)."""

    def __init__(self, noise):
        self.noise = torch.as_tensor(noise)
        self.at = 0

    def eval(self):
        self.at = 0
        return self

    def __call__(self, mixture, prompts):
        b = mixture.shape[0]
        out = 0.8 * mixture + 0.05 * self.noise[self.at:self.at + b].to(mixture.device, mixture.dtype)
        self.at += b
        return out
