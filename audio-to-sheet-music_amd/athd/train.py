"""Training the head: the reference's `src/train.py` around the native step.

Mirrors `src/train.py` by name:
  * `train_epoch`      <- `train_epoch` (`:23-129`).  The batches come from athd/train_data.py, the loss value and its
                          gradient with respect to the estimate from athd/loss.py (`athd_loss_grad_coef` /
                          `athd_loss_grad_apply`), the model's forward and backward from whatever `model(mixture,
                          prompts)` is (`athd.head.HeadTrainer`: the frozen native encoder, then the head with its
                          `native_*` stages).  With an optimizer that sets `fused_clip` (`athd.optim.HeadAdamW`) the clip,
                          the AMP unscale and skip, and the update are one call of `athd_head_step`; every other optimizer
                          takes the reference's lines: `clip_grad_norm_`, then `optimizer.step()` or the scaler's.
  * `save_checkpoint`  <- `:205-236`, the same dict and the same three files; `athd.inference.load_model` reads them
  * `load_checkpoint`  <- `:239-267`
  * `train`            <- `train()` (`:274-605`): the same config keys and defaults, datasets, subsets, optimizer,
                          cosine schedule, scaler, resume, epoch loop, validation, best-SDR tracking and checkpoints
  * `main`             <- `python -m athd.train --config config.yaml`

What is not mirrored: wandb and spectrogram logging (`use_wandb: true` raises), and the pretrained
downloads: the model to start from is `model=` or the checkpoint `training.init_checkpoint`.  Two deliberate deviations:
the validation subset is taken from the validation set (the reference builds `Subset(train_dataset, val_idxs)`,
`:452`; athd/validate.py), and a run that resumes at or past its last epoch returns empty final metrics where the
reference fails on an unbound name.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, Iterable, Iterator, Optional, Sequence, Union

import torch

from .loss import combined_L1_sdr_loss, combined_loss


def train_epoch(model, dataloader: Iterable[Dict], optimizer: torch.optim.Optimizer, scaler, device, use_amp: bool,
                use_L1_cmb_loss: bool, l1_sdr_weight: Optional[float], l1_weight: Optional[float], grad_clip: float,
                sdr_weight: float, sisdr_weight: float, epoch: int, log_every: int,
                use_wandb: bool = False) -> Dict[str, float]:
    """Train for one epoch (`src/train.py:23-129`): {"loss", "sdr", "sisdr"} = the means over the batches of the batch
    metrics.  `dataloader` yields dicts with "mixture", "target" (tensors, moved to `device`) and "prompt"."""
    if use_wandb:
        raise ValueError("use_wandb=True: wandb and spectrogram logging are not part of athd.train")
    model.train()

    total_loss = 0.0
    total_sdr = 0.0
    total_sisdr = 0.0
    num_batches = 0

    if use_L1_cmb_loss:
        loss_function = combined_L1_sdr_loss
        weight1 = l1_sdr_weight
        if l1_weight is None:
            raise ValueError("l1_weight must be provided when using L1 combination loss.")
        weight2 = l1_weight
        print("**Using L1 + SDR combination loss for training")
    else:
        loss_function = combined_loss
        weight1 = sdr_weight
        weight2 = sisdr_weight

    amp = bool(use_amp) and torch.device(device).type == "cuda"
    # an optimizer that clips inside its step (athd.optim.HeadAdamW: one athd_head_step call, gradients left as they are)
    fused_clip = bool(getattr(optimizer, "fused_clip", False))
    for batch_idx, batch in enumerate(dataloader):
        mixture = batch["mixture"].to(device)
        target = batch["target"].to(device)
        prompts = batch["prompt"]

        optimizer.zero_grad()

        if amp:
            with torch.autocast("cuda"):
                estimated = model(mixture, prompts)
                loss, metrics = loss_function(estimated, target, weight1, weight2)
            scaler.scale(loss).backward()
            if fused_clip:
                scaler.step(optimizer, grad_clip=grad_clip)
            else:
                scaler.unscale_(optimizer)
                torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
                scaler.step(optimizer)
            scaler.update()
        else:
            estimated = model(mixture, prompts)
            loss, metrics = loss_function(estimated, target, weight1, weight2)
            loss.backward()
            if fused_clip:
                optimizer.step(grad_clip=grad_clip)
            else:
                torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
                optimizer.step()

        total_loss += metrics["loss/total"]
        total_sdr += metrics["metrics/sdr"]
        total_sisdr += metrics["metrics/sisdr"]
        num_batches += 1

        if log_every and batch_idx % log_every == 0:
            print(f"Epoch {epoch + 1} [{batch_idx}] loss: {metrics['loss/total']:.4f}, "
                  f"SDR: {metrics['metrics/sdr']:.2f}")

    return {
        "loss": total_loss / num_batches,
        "sdr": total_sdr / num_batches,
        "sisdr": total_sisdr / num_batches,
    }


def model_state_dict(model) -> Dict[str, torch.Tensor]:
    """What a checkpoint's `model_state_dict` holds: every tensor of the native model behind a `HeadTrainer`
    (`model.model`, reference key names) with the head's keys replaced by the head's current values, on the CPU.  A
    model without a native half contributes its own `state_dict()` alone."""
    native = getattr(model, "model", None)
    sd = {k: torch.as_tensor(v).clone() for k, v in getattr(native, "_weights", {}).items()}
    sd.update({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    return sd


CHECKPOINT_KEYS = ("epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "metrics")
RULE = "=" * 60


def save_checkpoint(model, optimizer: torch.optim.Optimizer, scheduler, epoch: int, metrics: Dict[str, float],
                    checkpoint_dir: str, is_best: bool = False):
    """The reference's checkpoint (`src/train.py:205-236`): one dict with CHECKPOINT_KEYS, written as
    `checkpoint_epoch_{epoch}.pt`, as `best_model.pt` when `is_best`, and as `latest.pt`, with the reference's two
    printed lines.  `model` is a `HeadTrainer`; the files hold tensors and plain Python values only, so
    `athd.inference.load_model` reads them with `weights_only=True`."""
    folder = Path(checkpoint_dir)
    folder.mkdir(parents=True, exist_ok=True)
    values = (epoch, model_state_dict(model), optimizer.state_dict(), scheduler.state_dict(), metrics)
    checkpoint = dict(zip(CHECKPOINT_KEYS, values))
    targets = [(folder / f"checkpoint_epoch_{epoch}.pt", "Saved checkpoint to {}")]
    if is_best:
        targets.append((folder / "best_model.pt", "Saved best model to {}"))
    targets.append((folder / "latest.pt", None))
    for path, message in targets:
        torch.save(checkpoint, path)
        if message:
            print(message.format(path))


def load_checkpoint(model, optimizer: Optional[torch.optim.Optimizer], scheduler, checkpoint_path: str) -> int:
    """Load a checkpoint and return its epoch (`src/train.py:239-267`).

    The head is loaded non-strictly: keys it does not have (the frozen half, `clap.*`) are ignored.  Optimizer and
    scheduler state that does not fit is skipped with the reference's message.  A checkpoint the reference wrote is such
    a case: its `optimizer_state_dict` indexes all of the model's parameters, not the head's 50, so its group does not
    match and the optimizer starts fresh (`HeadAdamW.load_state_dict` changes nothing when it refuses)."""
    checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    model.load_state_dict(checkpoint["model_state_dict"], strict=False)
    for what, target in (("optimizer", optimizer), ("scheduler", scheduler)):
        try:
            target.load_state_dict(checkpoint[f"{what}_state_dict"])
        except Exception:
            print(f"Skipping {what} state...")
    epoch = checkpoint["epoch"]
    print(f"Loaded checkpoint from epoch {epoch}")
    return epoch


def cosine_schedule(optimizer: torch.optim.Optimizer, epochs: int, learning_rate: float):
    """The schedule of `train()` (`src/train.py:483-487`): one cosine half-wave over the run, from `learning_rate` down
    to a hundredth of it, stepped once per epoch"""
    return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=epochs, eta_min=learning_rate * 0.01)


# (section, key, default) of every config value `train()` reads: the reference's keys and defaults (`src/train.py:315-353`).
# Three sub-sections of `training` are addressed as "training.optimizer" and so on.  `num_workers` and `save_every` are
# not read: batches are cut on the GPU, and the reference saves every epoch whatever `save_every` says.
_REQUIRED = object()
CONFIG = {
    "train_dir": ("data", "train_dir", "../data/train"), "test_dir": ("data", "test_dir", "../data/test"),
    "pct_train": ("data", "pct_train", 1.0), "pct_test": ("data", "pct_test", 1.0),
    "sample_rate": ("data", "sample_rate", 44100), "segment_seconds": ("data", "segment_seconds", 6.0),
    "model_dim": ("model", "model_dim", 384), "text_dim": ("model", "text_dim", 512), "n_heads": ("model", "n_heads", 8),
    "device": ("model", "device", None),
    "batch_size": ("training", "batch_size", 4), "epochs": ("training", "num_epochs", 10),
    "use_amp": ("training", "use_amp", False), "resume_from": ("training", "resume_from", None),
    "init_checkpoint": ("training", "init_checkpoint", None),
    "use_L1_cmb_loss": ("training", "use_L1_comb_loss", False),
    "learning_rate": ("training.optimizer", "lr", 1e-4), "weight_decay": ("training.optimizer", "weight_decay", 1e-5),
    "grad_clip": ("training.optimizer", "grad_clip", 1.0),
    "l1_sdr_weight": ("training.L1_comb_loss", "sdr_weight", 1.0), "l1_weight": ("training.L1_comb_loss", "l1_weight", 0.05),
    "sdr_weight": ("training.loss_weights", "sdr", 0.9), "sisdr_weight": ("training.loss_weights", "sisdr", 0.1),
    "checkpoint_dir": ("wandb", "checkpoint_dir", "../checkpoints"), "use_wandb": ("wandb", "use_wandb", True),
    "log_every": ("wandb", "log_every", 50), "validate_every": ("wandb", "validate_every", 1),
}


def read_config(cfg: dict) -> SimpleNamespace:
    """The values of CONFIG out of a loaded config.  As in the reference the four top-level sections and the three
    sub-sections of `training` must exist (a missing one is a KeyError); every key inside them has a default."""
    out = SimpleNamespace()
    for name, (section, key, default) in CONFIG.items():
        node = cfg
        for part in section.split("."):
            node = node[part]
        setattr(out, name, node.get(key, default))
    out.learning_rate, out.weight_decay = float(out.learning_rate), float(out.weight_decay)
    out.segment_samples = int(out.sample_rate * out.segment_seconds)
    return out


def _batches(dataset, indices: Sequence[int], batch_size: int, device) -> Iterator[Dict]:
    """One epoch of the reference's `train_loader` (`shuffle=True, drop_last=True`): a fresh `torch.randperm` order,
    each batch drawn and cut on the device by `TrainSegmentDataset.batch`"""
    order = torch.randperm(len(indices)).tolist()
    for b0 in range(0, len(order) - batch_size + 1, batch_size):
        yield dataset.batch([indices[i] for i in order[b0:b0 + batch_size]], device)


def _subset(n_items: int, fraction: float) -> Optional[list]:
    """`torch.randperm(n)[:int(n * fraction)]` for a fraction strictly between 0 and 1, else None (all items)"""
    if not 0.0 < fraction < 1.0:
        return None
    return torch.randperm(n_items)[:int(n_items * fraction)].tolist()


def _resume(c: SimpleNamespace, trainer, optimizer, scheduler) -> int:
    """The epoch to start at: after `resume_from` if it is set (and exists), else after `checkpoint_dir/latest.pt` if
    there is one, else 0 (`src/train.py:496-508`)"""
    if c.resume_from is not None:
        path, found = Path(c.resume_from), "Resuming from {}"
    else:
        path, found = Path(c.checkpoint_dir) / "latest.pt", "Found latest checkpoint at {}"
    if not path.exists():
        return 0
    print(found.format(path))
    return load_checkpoint(trainer, optimizer, scheduler, str(path)) + 1


def train(config: Union[str, Path, dict], *, model=None, tokenizer=None, text_table=None, native: bool = True,
          dtype: str = "bf16", seed: Optional[int] = None):
    """The training job (`src/train.py:274-605`).  `config`: a YAML path or the loaded dict (CONFIG).  `model`: a loaded
    `AudioTextHTDemucs` to train the head of; without it `training.init_checkpoint` is loaded through `load_model`
    (`dtype`, `tokenizer=` / `text_table=` as there).  `native=True` trains with every native stage of the head (the
    four `native_*` options) and `HeadAdamW`; `native=False` with the torch stages and `torch.optim.AdamW`.  `seed`
    seeds Python's `random` (the cut, gain, swap and prompt of every batch) and `torch.manual_seed` (the subsets and
    the order of the items), as `athd.validate --seed` does; None leaves both generators as they are.

    Returns {"final_train_metrics", "final_val_metrics", "best_sdr"}.  With `native=True` every forward and backward
    kernel of the head and the update step are the library's and repeat bit for bit, so two runs from the same model,
    data, config and `seed` write the same bits into their checkpoints; nothing here sets a torch switch for that
    (`torch.backends.cudnn.deterministic` is left alone).  `native=False` leaves the gradients to torch's autograd,
    whose convolution gradients differ from run to run unless the caller sets that switch."""
    import random

    from .head import HeadTrainer
    from .inference import load_config, load_model
    from .musdb import STEM_PROMPTS, MusDBTracks
    from .optim import HeadAdamW
    from .train_data import TrainSegmentDataset
    from .validate import SegmentDataset, validate

    if seed is not None:
        random.seed(int(seed))
        torch.manual_seed(int(seed))
    c = read_config(config if isinstance(config, dict) else load_config(config))
    if c.use_wandb:
        raise ValueError("wandb.use_wandb is true (the reference's default): wandb logging is not part of athd.train; "
                         "set wandb.use_wandb: false")
    if (c.model_dim, c.text_dim, c.n_heads) != (384, 512, 8):
        raise ValueError("the native path is built for model_dim=384, text_dim=512, n_heads=8")
    device = c.device if c.device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
    if torch.device(device).type != "cuda" or not torch.cuda.is_available():       # the native path has no CPU side
        raise RuntimeError(f"athd.train needs a CUDA device (got device={device!r}, "
                           f"cuda available: {torch.cuda.is_available()})")

    banner = ["Audio-Text HTDemucs Training", RULE, f"Device: {device}", f"Train directory: {c.train_dir}",
              f"Test directory: {c.test_dir}", f"Segment length: {c.segment_seconds}s ({c.segment_samples} samples)",
              f"Batch size: {c.batch_size}", f"Epochs: {c.epochs}", f"Learning rate: {c.learning_rate}"]
    print("\n".join([RULE] + banner + [RULE]))

    if model is None:
        if c.init_checkpoint is None:
            raise ValueError("athd.train starts from a checkpoint: pass model= or set training.init_checkpoint "
                             "(--init-checkpoint); there is no pretrained download")
        print(f"Loading {c.init_checkpoint}...")
        model = load_model(str(c.init_checkpoint), device, dtype=dtype, text_table=text_table, tokenizer=tokenizer,
                           native_text=tokenizer is not None and text_table is None)
    elif model.device is None:
        model.to(device)
    device = model.device                                   # with its index: where the batches are cut

    print("Building AudioTextHTDemucs model...")
    trainer = HeadTrainer(model, native_output=native, native_cond=native, native_decoders=native, native_proj=native)
    # the frozen half has no torch parameters: it is counted over the tensors the native model holds
    trainable = sum(p.numel() for p in trainer.parameters() if p.requires_grad)
    head_names = set(trainer.state_dict())
    frozen = sum(int(v.size) for k, v in model._weights.items() if k not in head_names)
    print(f"Total parameters: {frozen + trainable:,}")
    print(f"Trainable parameters: {trainable:,}")

    print("Creating datasets...")
    train_dataset = TrainSegmentDataset(MusDBTracks(c.train_dir, sample_rate=c.sample_rate), c.segment_samples,
                                        random_segments=True, augment=True)
    val_dataset = SegmentDataset(MusDBTracks(c.test_dir, sample_rate=c.sample_rate), c.segment_samples)
    # (the validation subset comes from the validation set: the module docstring)
    train_items = _subset(len(train_dataset), c.pct_train) or list(range(len(train_dataset)))
    val_items = _subset(len(val_dataset), c.pct_test)

    adamw = HeadAdamW if native else torch.optim.AdamW
    optimizer = adamw(trainer.parameters(), lr=c.learning_rate, weight_decay=c.weight_decay, betas=(0.9, 0.999))
    scheduler = cosine_schedule(optimizer, c.epochs, c.learning_rate)
    scaler = torch.amp.GradScaler("cuda") if c.use_amp else None
    loss_args = dict(use_L1_cmb_loss=c.use_L1_cmb_loss, l1_sdr_weight=c.l1_sdr_weight, l1_weight=c.l1_weight,
                     sdr_weight=c.sdr_weight, sisdr_weight=c.sisdr_weight)

    best_sdr = -float("inf")
    first_epoch = _resume(c, trainer, optimizer, scheduler)
    print("\nStarting training...")
    train_metrics: Dict[str, float] = {}
    val_metrics: Dict[str, float] = {}
    for number in range(first_epoch + 1, c.epochs + 1):                     # epochs are printed and saved from 1
        print("\n".join(["", RULE, f"Epoch {number}/{c.epochs}", f"Learning rate: {scheduler.get_last_lr()[0]:.2e}",
                         RULE]))
        train_metrics = train_epoch(trainer, _batches(train_dataset, train_items, c.batch_size, device), optimizer,
                                    scaler, device, c.use_amp, grad_clip=c.grad_clip, epoch=number - 1,
                                    log_every=c.log_every, **loss_args)
        print(f"Train - Loss: {train_metrics['loss']:.4f}, SDR: {train_metrics['sdr']:.2f} dB")
        scheduler.step()

        val_metrics, is_best = {}, False
        if number % c.validate_every == 0:
            # the head's weights go into the native model, which scores the split on the inference path
            trainer.sync()
            val_metrics = validate(model, val_dataset, batch_size=c.batch_size, indices=val_items, **loss_args)
            print(f"Val - Loss: {val_metrics['loss']:.4f}, SDR: {val_metrics['sdr']:.2f} dB")
            for stem in STEM_PROMPTS:
                if f"sdr/{stem}" in val_metrics:
                    print(f"  {stem}: {val_metrics[f'sdr/{stem}']:.2f} dB")
            if val_metrics["sdr"] > best_sdr:
                best_sdr, is_best = val_metrics["sdr"], True
                print(f"New best SDR: {best_sdr:.2f} dB")
        save_checkpoint(trainer, optimizer, scheduler, number, {**train_metrics, **val_metrics}, c.checkpoint_dir, is_best)

    print("\n".join(["", RULE, "Training complete!", f"Best validation SDR: {best_sdr:.2f} dB", RULE]))
    return {"final_train_metrics": train_metrics, "final_val_metrics": val_metrics, "best_sdr": best_sdr}


def main(argv=None) -> int:
    """`python -m athd.train --config config.yaml [--init-checkpoint PATH] [--epochs N] [--no-native] [--dtype
    f32|bf16] [--seed K]`: `train()` on the config, with the three overrides."""
    ap = argparse.ArgumentParser(prog="python -m athd.train",
                                 description="Train the head on the frozen native encoder (src/train.py train()).")
    ap.add_argument("--config", default="config.yaml")
    ap.add_argument("--init-checkpoint", default=None, help="overrides training.init_checkpoint")
    ap.add_argument("--epochs", type=int, default=None, help="overrides training.num_epochs")
    ap.add_argument("--no-native", action="store_true", help="torch head stages and torch.optim.AdamW")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="bf16", help="the frozen half's context")
    ap.add_argument("--seed", type=int, default=None, help="seeds random and torch.manual_seed; with the native stages (no --no-native) a run repeats bit for bit")
    args = ap.parse_args(argv)

    from .inference import load_config
    cfg = load_config(args.config)
    training_cfg = cfg.setdefault("training", {})
    if args.init_checkpoint is not None:
        training_cfg["init_checkpoint"] = args.init_checkpoint
    if args.epochs is not None:
        training_cfg["num_epochs"] = args.epochs
    train(cfg, native=not args.no_native, dtype=args.dtype, seed=args.seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
