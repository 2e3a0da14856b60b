"""The optimizer of head training: `clip_grad_norm_` + `torch.optim.AdamW.step` (`src/train.py:80-95, 476-481`) as one
call of `athd_head_step` (include/athd.h, csrc/head_step.hip).

`HeadAdamW` is a `torch.optim.Optimizer`: schedulers, `zero_grad`, `state_dict` / `load_state_dict` and
`torch.amp.GradScaler.step` work on it as on `torch.optim.AdamW`, and a state dict saved by one loads into the other over
the same parameters.  What differs from torch, all of it deliberate (include/athd.h):
  * `step(grad_clip=...)` clips inside the step; the gradients are read, never rewritten;
  * a non-finite gradient norm skips the step (reported in `last_stats[2]`) instead of poisoning the parameters;
  * one step counter serves all parameters (torch keeps one per parameter; they are equal whenever every parameter has
    had a gradient in every step).  A parameter whose first gradient arrives later joins with zero moments and the
    shared count.
There is no fallback: what the kernel does not cover (CPU or non-float32 parameters, several groups, amsgrad, more than
64 tensors with a gradient) raises.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import native

_UNSUPPORTED = {"amsgrad": False, "maximize": False, "capturable": False, "differentiable": False, "fused": None,
                "foreach": None}


class HeadAdamW(torch.optim.Optimizer):
    """`torch.optim.AdamW(params, lr, betas, eps, weight_decay)` for one group of float32 CUDA parameters on one device,
    at most 64 of them with a gradient per step.

    `state[p]` holds `exp_avg` and `exp_avg_sq`, 16-byte-aligned slices of one flat buffer created zero at the
    parameter's first step; the step counter is one device int32.  `step` enqueues on the current stream and never
    synchronises; `last_stats` is the device tensor {norm, coef, skipped, counter} of the last step.

    `fused_clip`: `athd.train.train_epoch` hands `grad_clip` to `step` instead of calling `clip_grad_norm_`.
    `_step_supports_amp_scaling`: `GradScaler.step` hands over `grad_scale` / `found_inf` as device tensors and leaves
    the unscale and the skip to the kernel (no host synchronisation)."""

    fused_clip = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 **unsupported):
        for k, v in unsupported.items():
            if k not in _UNSUPPORTED:
                raise TypeError(f"HeadAdamW: unexpected argument {k!r}")
            if (v is not None) if _UNSUPPORTED[k] is None else bool(v):      # fused / foreach: any choice at all
                raise ValueError(f"HeadAdamW does not support {k}={v!r}; use torch.optim.AdamW for it")
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= float(eps):
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= float(betas[0]) < 1.0 and 0.0 <= float(betas[1]) < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= float(weight_decay):
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        params = list(params)
        if len(params) > 1 and all(isinstance(g, dict) for g in params):
            raise ValueError("HeadAdamW takes one parameter group")
        # torch.optim.AdamW's group keys, so that the two optimizers' state dicts are interchangeable
        probe = torch.optim.AdamW([torch.zeros(1, requires_grad=True)])
        defaults = dict(probe.defaults)
        defaults.update(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                        weight_decay=float(weight_decay))
        self._step_count_dev = None           # the shared int32 counter, made with the first state
        self._loaded_step = 0
        self._ws = None
        self.last_stats = None
        super().__init__(params, defaults)
        self._step_supports_amp_scaling = True

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("HeadAdamW takes one parameter group")
        super().add_param_group(param_group)
        self._check_params(self.param_groups[0]["params"])

    @staticmethod
    def _check_params(params):
        """what athd_head_step covers: float32 CUDA tensors on one device"""
        devices = {p.device for p in params}
        for p in params:
            if p.dtype != torch.float32:
                raise ValueError(f"HeadAdamW needs float32 parameters, got {p.dtype}")
            if p.device.type != "cuda":
                raise ValueError(f"HeadAdamW needs CUDA parameters, got one on {p.device}")
        if len(devices) > 1:
            raise ValueError(f"HeadAdamW needs all parameters on one device, got {sorted(map(str, devices))}")

    # ------------------------------------------------------------------ state
    @property
    def device(self) -> torch.device:
        return self.param_groups[0]["params"][0].device

    def _counter(self) -> torch.Tensor:
        if self._step_count_dev is None:
            self._step_count_dev = torch.full((1,), int(self._loaded_step), dtype=torch.int32, device=self.device)
        return self._step_count_dev

    def _make_state(self, params: List[torch.Tensor], values: Dict[int, tuple] = None):
        """Moments for `params` as slices of one new flat buffer (each slice starts at a multiple of four elements of a
        fresh allocation: 16-byte aligned), zero or copied from `values[id(p)] = (exp_avg, exp_avg_sq)`"""
        pad = lambda n: -(-n // 4) * 4
        flat = torch.zeros(sum(2 * pad(p.numel()) for p in params), dtype=torch.float32, device=self.device)
        at = 0
        for p in params:
            n = p.numel()
            m = flat[at:at + n].view(p.shape)
            v = flat[at + pad(n):at + pad(n) + n].view(p.shape)
            at += 2 * pad(n)
            if values is not None:
                m.copy_(values[id(p)][0])
                v.copy_(values[id(p)][1])
            self.state[p] = {"exp_avg": m, "exp_avg_sq": v}

    def step_count(self) -> int:
        """The counter's value (one device read)"""
        return int(self._loaded_step if self._step_count_dev is None else self._step_count_dev.item())

    def state_dict(self):
        """torch.optim.AdamW's layout: every parameter's "step" is a CPU float32 scalar (one device read here)"""
        sd = super().state_dict()
        if sd["state"]:
            t = float(self.step_count())
            sd["state"] = {k: {"step": torch.tensor(t, dtype=torch.float32), **v} for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        steps = {float(v["step"]) for v in state_dict["state"].values() if "step" in v}
        if len(steps) > 1:
            raise ValueError(f"HeadAdamW keeps one step counter, the state dict has several: {sorted(steps)}")
        for v in state_dict["state"].values():
            if "exp_avg" not in v or "exp_avg_sq" not in v or "max_exp_avg_sq" in v:
                raise ValueError("HeadAdamW loads torch.optim.AdamW state without amsgrad: exp_avg and exp_avg_sq")
        # everything that can be refused is refused before anything is loaded: a failed call leaves the optimizer as it was
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"HeadAdamW takes one parameter group, the state dict has {len(groups)}")
        for k, v in _UNSUPPORTED.items():
            got = groups[0].get(k, v)
            if got != v and not (v is None and got is False):
                raise ValueError(f"HeadAdamW does not support {k}={got!r} (from the loaded state dict)")
        super().load_state_dict(state_dict)
        group = self.param_groups[0]
        loaded = [p for p in group["params"] if p in self.state and "exp_avg" in self.state[p]]
        values = {id(p): (self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in loaded}
        for p in list(self.state):
            del self.state[p]
        if loaded:
            self._make_state(loaded, values)
        self._loaded_step = int(steps.pop()) if steps else 0
        self._step_count_dev = None

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None, grad_clip=None):
        """One `athd_head_step` on the current stream over the parameters that have a gradient.  grad_clip: the
        `max_norm` of `clip_grad_norm_` (None or <= 0: no clipping).  Under `GradScaler.step` the scaler's `grad_scale`
        and `found_inf` are read from the attributes it sets."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        live = [p for p in group["params"] if p.grad is not None and p.numel() > 0]
        if not live:
            return loss
        if len(live) > native.STEP_MAX_TENSORS:
            raise RuntimeError(f"HeadAdamW: {len(live)} tensors have a gradient, athd_head_step takes at most "
                               f"{native.STEP_MAX_TENSORS}")
        dev = self.device
        grads = []
        for p in live:
            g = p.grad
            if g.is_sparse or g.dtype != torch.float32 or g.device != dev:
                raise RuntimeError(f"HeadAdamW needs dense float32 gradients on {dev}, got {g.dtype} on {g.device}")
            if not p.is_contiguous():
                raise RuntimeError("HeadAdamW needs contiguous parameters")
            grads.append(g if g.is_contiguous() else g.contiguous())
        fresh = [p for p in live if p not in self.state or "exp_avg" not in self.state[p]]
        if fresh:
            self._make_state(fresh)
        table = native.step_table([(p.data_ptr(), g.data_ptr(), self.state[p]["exp_avg"].data_ptr(),
                                    self.state[p]["exp_avg_sq"].data_ptr(), p.numel()) for p, g in zip(live, grads)])
        nbytes = native.head_step_workspace_bytes(table)
        if nbytes == 0:
            raise RuntimeError("HeadAdamW: athd_head_step refuses these tensors (more than 4096 chunks of 4096 elements)")
        if self._ws is None or self._ws.numel() * 8 < nbytes:
            self._ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        if self.last_stats is None:
            self.last_stats = torch.zeros(4, dtype=torch.float32, device=dev)
        b1, b2 = group["betas"]
        hp = native.StepHparams(float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                float(group["weight_decay"]), float(grad_clip) if grad_clip is not None else 0.0)
        scalars = []
        for name in ("grad_scale", "found_inf"):
            t = getattr(self, name, None)
            if t is not None:
                t = t.to(device=dev, dtype=torch.float32).reshape(-1)
                if t.numel() != 1:
                    raise RuntimeError(f"HeadAdamW: {name} must hold one value")
            scalars.append(t)
        with torch.cuda.device(dev):
            native.head_step(table, hp, *[None if t is None else t.data_ptr() for t in scalars],
                             self._counter().data_ptr(), self.last_stats.data_ptr(), self._ws.data_ptr(),
                             self._ws.numel() * 8, torch.cuda.current_stream(dev).cuda_stream)
        return loss
