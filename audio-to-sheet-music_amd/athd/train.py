"""The step loop of training: the reference's `train_epoch` (`src/train.py:23-129`) around the native loss.

The batches come from athd/train_data.py and the loss value and its gradient with respect to the estimate from
athd/loss.py (`athd_loss_grad_coef` / `athd_loss_grad_apply`).  Everything between those two ends stays torch's: the
model's forward and backward (any `model(mixture, prompts)` that autograd can differentiate), `clip_grad_norm_`, the
optimizer and the AMP scaler.  wandb and spectrogram logging are not mirrored.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

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
            scaler.unscale_(optimizer)
            torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
            scaler.step(optimizer)
            scaler.update()
        else:
            estimated = model(mixture, prompts)
            loss, metrics = loss_function(estimated, target, weight1, weight2)
            loss.backward()
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
