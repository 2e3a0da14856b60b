"""The host side of the training job (athd/train.py `save_checkpoint`, `load_checkpoint`, the schedule), no GPU: a tiny
stand-in trainer with `torch.optim.AdamW` on the CPU.

  1. `save_checkpoint` writes `checkpoint_epoch_{n}.pt`, `latest.pt` and `best_model.pt` with the reference's five keys,
     readable with `weights_only=True`; `model_state_dict` holds the native half's tensors with the head's keys replaced
     by the head's current values.
  2. `load_checkpoint` returns the epoch and restores optimizer and scheduler: a run resumed after epoch 1 ends with the
     same parameters as an uninterrupted 2-epoch run, bit for bit.
  3. State that does not fit is skipped with the reference's messages.
  4. The learning rates of `train()`'s schedule (`cosine_schedule`) over 3 epochs are the closed form of a cosine from lr
     to lr / 100; `read_config` returns the reference's defaults and refuses a missing section.
  5. `train()` refuses wandb logging and a machine without CUDA.
"""
import math

import numpy as np
import pytest
import torch

KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "metrics"}
LR, EPOCHS = 1e-2, 2


class _Native:
    """what `save_checkpoint` reads of the native model: its tensors by reference key"""

    def __init__(self):
        self._weights = {"htdemucs.encoder.0.conv.weight": np.arange(6, dtype=np.float32).reshape(2, 3),
                         "lin.weight": np.zeros((2, 3), dtype=np.float32)}        # stale: the head's value must win


class _Trainer(torch.nn.Module):
    """a stand-in for `HeadTrainer`: `model` is a plain attribute, `state_dict()` the head's keys"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.lin = torch.nn.Linear(3, 2)
        object.__setattr__(self, "model", _Native())


def _epoch(trainer, opt, epoch):
    """three deterministic steps"""
    for i in range(3):
        x = torch.full((4, 3), 0.1 * (epoch * 3 + i + 1))
        opt.zero_grad()
        trainer.lin(x).pow(2).sum().backward()
        opt.step()


def _new():
    trainer = _Trainer()
    opt = torch.optim.AdamW(trainer.parameters(), lr=LR, weight_decay=1e-2, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=EPOCHS, eta_min=LR * 0.01)
    return trainer, opt, sched


def test_checkpoint_files_and_resume(tmp_path, capsys):
    from athd.train import load_checkpoint, save_checkpoint
    # the uninterrupted run
    trainer, opt, sched = _new()
    for e in range(EPOCHS):
        _epoch(trainer, opt, e)
        sched.step()
    want = {k: v.clone() for k, v in trainer.state_dict().items()}
    # epoch 1, saved
    trainer, opt, sched = _new()
    _epoch(trainer, opt, 0)
    sched.step()
    save_checkpoint(trainer, opt, sched, 1, {"loss": 1.5, "sdr": -2.0}, str(tmp_path), is_best=True)
    out = capsys.readouterr().out
    assert f"Saved checkpoint to {tmp_path / 'checkpoint_epoch_1.pt'}" in out
    assert f"Saved best model to {tmp_path / 'best_model.pt'}" in out
    for name in ("checkpoint_epoch_1.pt", "latest.pt", "best_model.pt"):
        ck = torch.load(tmp_path / name, map_location="cpu", weights_only=True)
        assert set(ck) == KEYS and ck["epoch"] == 1 and ck["metrics"] == {"loss": 1.5, "sdr": -2.0}
        sd = ck["model_state_dict"]
        assert set(sd) == {"htdemucs.encoder.0.conv.weight", "lin.weight", "lin.bias"}
        assert torch.equal(sd["lin.weight"], trainer.lin.weight.detach()) and bool(sd["lin.weight"].any())
        assert torch.equal(sd["htdemucs.encoder.0.conv.weight"], torch.arange(6.).reshape(2, 3))
    save_checkpoint(trainer, opt, sched, 7, {}, str(tmp_path / "b"))
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["checkpoint_epoch_7.pt", "latest.pt"]
    # resumed in fresh objects
    trainer, opt, sched = _new()
    with torch.no_grad():
        for p in trainer.parameters():
            p.zero_()
    assert load_checkpoint(trainer, opt, sched, str(tmp_path / "latest.pt")) == 1
    out = capsys.readouterr().out
    assert "Loaded checkpoint from epoch 1" in out and "Skipping" not in out
    assert sched.last_epoch == 1 and opt.param_groups[0]["lr"] == sched.get_last_lr()[0]
    _epoch(trainer, opt, 1)
    sched.step()
    for k, v in trainer.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_load_checkpoint_skips_state_that_does_not_fit(tmp_path, capsys):
    from athd.train import load_checkpoint, save_checkpoint
    trainer, opt, sched = _new()
    _epoch(trainer, opt, 0)
    # an optimizer over other parameters (as a checkpoint the reference wrote indexes all of the model's)
    other = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(2)) for _ in range(5)], lr=LR)

    class Sched:
        def state_dict(self):
            return {"last_epoch": 1}

    save_checkpoint(trainer, other, Sched(), 3, {}, str(tmp_path))
    capsys.readouterr()

    class Refuses:
        def load_state_dict(self, sd):
            raise KeyError("no such schedule")

    fresh, fopt, _ = _new()
    assert load_checkpoint(fresh, fopt, Refuses(), str(tmp_path / "latest.pt")) == 3
    out = capsys.readouterr().out
    assert "Skipping optimizer state..." in out and "Skipping scheduler state..." in out
    assert torch.equal(fresh.lin.weight, trainer.lin.weight)              # the head was loaded all the same
    assert not fopt.state                                                 # and the optimizer starts fresh


def test_cosine_schedule_over_three_epochs():
    p = [torch.nn.Parameter(torch.zeros(1))]
    lr, epochs = 3e-4, 3
    from athd.train import cosine_schedule
    opt = torch.optim.AdamW(p, lr=lr)
    sched = cosine_schedule(opt, epochs, lr)                              # what train() builds
    got = []
    for _ in range(epochs):
        got.append(sched.get_last_lr()[0])
        opt.step()
        sched.step()
    want = [lr * 0.01 + (lr - lr * 0.01) * (1 + math.cos(math.pi * e / epochs)) / 2 for e in range(epochs)]
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert np.isclose(sched.get_last_lr()[0], lr * 0.01, rtol=1e-9)


def test_read_config_defaults(tmp_path):
    from athd.train import read_config
    c = read_config(_config(tmp_path))
    assert (c.batch_size, c.epochs, c.learning_rate, c.weight_decay, c.grad_clip) == (4, 10, 1e-4, 1e-5, 1.0)
    assert (c.sample_rate, c.segment_seconds, c.segment_samples, c.pct_train, c.pct_test) == (44100, 6.0, 264600, 1.0, 1.0)
    assert (c.sdr_weight, c.sisdr_weight, c.l1_sdr_weight, c.l1_weight, c.use_L1_cmb_loss) == (0.9, 0.1, 1.0, 0.05, False)
    assert (c.use_amp, c.resume_from, c.device, c.log_every, c.validate_every) == (False, None, None, 50, 1)
    cfg = _config(tmp_path)
    cfg["training"]["optimizer"] = {"lr": "3e-4"}                         # YAML reads 3e-4 as a string
    cfg["wandb"].pop("use_wandb")
    c = read_config(cfg)
    assert c.learning_rate == 3e-4 and c.use_wandb is True               # the reference's default
    del cfg["training"]["loss_weights"]
    with pytest.raises(KeyError):
        read_config(cfg)


def _config(tmp_path, **wandb):
    return {"data": {"train_dir": str(tmp_path), "test_dir": str(tmp_path)}, "model": {},
            "training": {"optimizer": {}, "L1_comb_loss": {}, "loss_weights": {}},
            "wandb": dict({"checkpoint_dir": str(tmp_path / "ck"), "use_wandb": False}, **wandb)}


def test_train_refusals(tmp_path):
    from athd.train import train
    with pytest.raises(ValueError, match="wandb"):
        train(_config(tmp_path, use_wandb=True))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="CUDA"):
            train(_config(tmp_path))
    cfg = _config(tmp_path)
    cfg["model"]["device"] = "cpu"
    with pytest.raises(RuntimeError, match="CUDA"):
        train(cfg)
