"""The reference's `src/loss.py` by name, on the device (the metrics `validate` of `src/train.py:132-202`
reads).

  * `loss_rows`             <- every per-row quantity of `src/loss.py` in one call of `athd_loss_rows`:
                               (rows, 4) float64 = {sdr, sisdr, new_sdr, l1}
  * `new_sdr_metric`        <- `:71-87`
  * `combined_loss`         <- `:90-127`
  * `combined_L1_sdr_loss`  <- `:130-162`
  * `sdr_loss`, `sisdr_loss` <- `:9-68`, re-exported from athd/inference.py unchanged (mean-only kernels)
  * `loss_with_grad`        <- the `total` of the two combined losses as a scalar that back-propagates to `estimated`
                               (`loss.backward()` of `src/train.py:78, 88`): `athd_loss_grad_coef` in the forward,
                               `athd_loss_grad_apply` in the backward.  `combined_loss` / `combined_L1_sdr_loss` take it
                               only when `estimated.requires_grad` with grad mode on; the value has the same bits.

Everything is a function of the row table: a batch's sdr_loss is minus the mean of its rows' clamped `sdr`, its
sisdr_loss minus the mean of the clamped `sisdr`, new_sdr the mean of the unclamped column and L1 the mean of the `l1`
column (rows have equal length).  The table is accumulated in fp64 with a fixed summation order: the same bits on every
run.  The metric dicts come from ONE device-to-host copy of the table, not one `.item()` per key.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import native
from .inference import sdr_loss, sisdr_loss  # noqa: F401  (src/loss.py:9-68, the mean-only kernels)

SDR, SISDR, NEW_SDR, L1 = 0, 1, 2, 3


def loss_rows(estimated: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(rows, 4) float64 device tensor {sdr, sisdr, new_sdr, l1} of `estimated` / `target` flattened to
    (shape[0], -1) as the reference does (`src/loss.py:15-16`); enqueued on the current stream (athd_loss_rows)."""
    if estimated.dim() < 1 or estimated.shape[0] != target.shape[0] or estimated.numel() != target.numel():
        raise ValueError("estimated and target must have the same rows and size")
    if estimated.device.type != "cuda" or target.device != estimated.device:
        raise ValueError("estimated and target must be on the same HIP device (there is no CPU path)")
    rows = estimated.shape[0]
    est = estimated.reshape(rows, -1).float().contiguous()
    tgt = target.reshape(rows, -1).float().contiguous()
    n = est.shape[1]
    nbytes = int(native.lib.athd_loss_rows_scratch_bytes(rows, n))
    if nbytes == 0:
        raise ValueError(f"loss_rows: rows must be in [1, 2^20] and the row length in [1, 2^31), got ({rows}, {n})")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=est.device)
    out = torch.empty((rows, 4), dtype=torch.float64, device=est.device)
    rc = native.lib.athd_loss_rows(est.data_ptr(), tgt.data_ptr(), rows, n, scratch.data_ptr(), out.data_ptr(),
                                   torch.cuda.current_stream(est.device).cuda_stream)
    if rc != 0:
        raise native.AthdError(f"athd_loss_rows failed ({rc})")
    return out


def new_sdr_metric(estimated: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """`src/loss.py:71-87`: the unclamped SDR per batch item, (batch,) float32 on the device."""
    return loss_rows(estimated, target)[:, NEW_SDR].float()


def combined_from_rows(table: np.ndarray, sdr_weight: float = 0.9, sisdr_weight: float = 0.1) -> Dict[str, float]:
    """The metric dict of `combined_loss` (`:118-125`) from a host copy of the row table of one batch."""
    sdr = -float(np.mean(table[:, SDR]))
    sisdr = -float(np.mean(table[:, SISDR]))
    return {"loss/total": sdr_weight * sdr + sisdr_weight * sisdr, "loss/sdr": sdr, "loss/sisdr": sisdr,
            "metrics/sdr": -sdr, "metrics/sisdr": -sisdr, "metrics/new_sdr": float(np.mean(table[:, NEW_SDR]))}


def combined_l1_from_rows(table: np.ndarray, sdr_weight: float = 1.0, l1_weight: float = 0.05) -> Dict[str, float]:
    """The metric dict of `combined_L1_sdr_loss` (`:154-160`) from a host copy of the row table of one batch."""
    sdr = -float(np.mean(table[:, SDR]))
    sisdr = -float(np.mean(table[:, SISDR]))
    return {"loss/total": sdr_weight * sdr + l1_weight * float(np.mean(table[:, L1])), "loss/sdr": sdr,
            "loss/sisdr": sisdr, "metrics/sdr": -sdr, "metrics/sisdr": -sisdr}


def _combined_total(table: torch.Tensor, sdr_weight: float, sisdr_weight: float) -> torch.Tensor:
    return (-(sdr_weight * table[:, SDR].mean() + sisdr_weight * table[:, SISDR].mean())).float()


def _combined_l1_total(table: torch.Tensor, sdr_weight: float, l1_weight: float) -> torch.Tensor:
    return (-sdr_weight * table[:, SDR].mean() + l1_weight * table[:, L1].mean()).float()


class _LossWithGrad(torch.autograd.Function):
    """total(table) of a contiguous float32 (rows, n) pair with d total / d est by `athd_loss_grad_apply`.  `total_of`
    maps the row table to the scalar and must be the function the three weights describe:
    -(w_sdr mean sdr + w_sisdr mean sisdr) + w_l1 mean l1."""

    @staticmethod
    def forward(ctx, est, tgt, w_sdr, w_sisdr, w_l1, total_of):
        rows, n = est.shape
        nbytes = int(native.lib.athd_loss_grad_scratch_bytes(rows, n))
        if nbytes == 0:
            raise ValueError(f"loss_with_grad: rows must be in [1, 2^20] and the row length in [1, 2^31), got "
                             f"({rows}, {n})")
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=est.device)
        table = torch.empty((rows, 4), dtype=torch.float64, device=est.device)
        coef = torch.empty((rows, 8), dtype=torch.float64, device=est.device)
        rc = native.lib.athd_loss_grad_coef(est.data_ptr(), tgt.data_ptr(), rows, n, scratch.data_ptr(),
                                            table.data_ptr(), coef.data_ptr(),
                                            torch.cuda.current_stream(est.device).cuda_stream)
        if rc != 0:
            raise native.AthdError(f"athd_loss_grad_coef failed ({rc})")
        ctx.save_for_backward(est, tgt, coef)
        ctx.weights = (float(w_sdr), float(w_sisdr), float(w_l1))
        ctx.mark_non_differentiable(table)
        return total_of(table), table

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_total, _grad_table):
        est, tgt, coef = ctx.saved_tensors
        rows, n = est.shape
        upstream = grad_total.to(device=est.device, dtype=torch.float32).contiguous()      # a device scalar: no sync
        grad = torch.empty_like(est)
        rc = native.lib.athd_loss_grad_apply(est.data_ptr(), tgt.data_ptr(), rows, n, coef.data_ptr(), *ctx.weights,
                                             upstream.data_ptr(), grad.data_ptr(),
                                             torch.cuda.current_stream(est.device).cuda_stream)
        if rc != 0:
            raise native.AthdError(f"athd_loss_grad_apply failed ({rc})")
        return grad, None, None, None, None, None


def loss_with_grad(estimated: torch.Tensor, target: torch.Tensor, w_sdr: float, w_sisdr: float, w_l1: float,
                   _total_of=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(total, table): total = -(w_sdr mean sdr + w_sisdr mean sisdr) + w_l1 mean l1 over the rows of `loss_rows`' table,
    a float32 device scalar that back-propagates to `estimated` through `athd_loss_grad_apply` (the losses of
    `src/loss.py:90-162` are its two corners); `table` is the (rows, 4) float64 row table, the bits of `loss_rows`.
    The casts to contiguous float32 rows are torch ops outside the Function: autograd carries the gradient back
    through them to a half-precision or non-contiguous `estimated`.  No gradient is built for `target`."""
    if target.requires_grad:
        raise ValueError("loss_with_grad: target must not require grad (no gradient is built for it)")
    if estimated.dim() < 1 or estimated.shape[0] != target.shape[0] or estimated.numel() != target.numel():
        raise ValueError("estimated and target must have the same rows and size")
    if estimated.device.type != "cuda" or target.device != estimated.device:
        raise ValueError("estimated and target must be on the same HIP device (there is no CPU path)")
    rows = estimated.shape[0]
    est = estimated.reshape(rows, -1).float().contiguous()
    tgt = target.reshape(rows, -1).float().contiguous()
    if _total_of is None:
        def _total_of(table):
            return (-(w_sdr * table[:, SDR].mean() + w_sisdr * table[:, SISDR].mean())
                    + w_l1 * table[:, L1].mean()).float()
    return _LossWithGrad.apply(est, tgt, w_sdr, w_sisdr, w_l1, _total_of)


def combined_loss(estimated: torch.Tensor, target: torch.Tensor, sdr_weight: float = 0.9,
                  sisdr_weight: float = 0.1) -> Tuple[torch.Tensor, Dict[str, float]]:
    """`src/loss.py:90-127`: (total, metrics); `total` a device scalar, the metrics Python floats.  When `estimated`
    requires grad (and grad mode is on) `total` back-propagates to it (`loss_with_grad`), with the same bits."""
    if estimated.requires_grad and torch.is_grad_enabled():
        total, table = loss_with_grad(estimated, target, sdr_weight, sisdr_weight, 0.0,
                                      lambda t: _combined_total(t, sdr_weight, sisdr_weight))
    else:
        table = loss_rows(estimated, target)
        total = _combined_total(table, sdr_weight, sisdr_weight)
    return total, combined_from_rows(table.cpu().numpy(), sdr_weight, sisdr_weight)


def combined_L1_sdr_loss(estimated: torch.Tensor, target: torch.Tensor, sdr_weight: float = 1.0,
                         l1_weight: float = 0.05) -> Tuple[torch.Tensor, Dict[str, float]]:
    """`src/loss.py:130-162`: (total, metrics) without `metrics/new_sdr`, as in the reference; differentiable as
    `combined_loss` is."""
    if estimated.requires_grad and torch.is_grad_enabled():
        total, table = loss_with_grad(estimated, target, sdr_weight, 0.0, l1_weight,
                                      lambda t: _combined_l1_total(t, sdr_weight, l1_weight))
    else:
        table = loss_rows(estimated, target)
        total = _combined_l1_total(table, sdr_weight, l1_weight)
    return total, combined_l1_from_rows(table.cpu().numpy(), sdr_weight, l1_weight)
