"""Head training's update step on the GPU (include/athd.h `athd_head_step`; athd/optim.py `HeadAdamW`; athd/train.py
`train_epoch`, `save_checkpoint`, `train`).

Kernel level, through ctypes on buffers with guard bands round every parameter, moment and gradient (tensor set and
regimes of tests/head_step_refs.py, K = 3 steps): bands intact, gradients unchanged, bit-equal across runs and under one
graph capture plus replay, displacement / m / v within ALLOW = 4 times the gap of torch's own float32 step on the same
GPU to the float64 reference (tests/test_head_step_refs.py shows that float32 reaches that and planted defects do not),
the reported norm within 2^-22 relative, a coefficient of exactly 1 where the clip is inactive, the counter at 3.
Misaligned pointers give the same bits; 1 and 64 tensors; 65 tensors and n = 0 are refused with nothing written.  The
skip (found_inf, a non-finite norm) writes nothing; a power-of-two grad_scale is exact.

`HeadAdamW` against torch's step and through `state_dict` both ways; three `train_epoch` steps at CASE_SHORT against the
float64 CPU loop; one autocast step under `GradScaler`; `train()` for two epochs with checkpoints and a resume.
"""
import functools

import numpy as np
import pytest
import torch

import head_refs as H
import head_step_refs as R
from test_gpu_head_output import _new_model, _rows, _wav, CASE_SHORT
from test_gpu_parity import _report

pytestmark = pytest.mark.gpu

K = 3
ALIGNED, MISALIGNED = 64, 61          # guard elements in front of a buffer: 256 bytes, or 4 bytes past a 16-byte boundary


@pytest.fixture(scope="module")
def kt():
    import ktest
    return ktest


def _native():
    from athd import native
    return native


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _refs(regime, sizes=tuple(R.SIZES), steps=K):
    """(case, ref64, the gaps of torch's float32 step on this GPU to it), computed once"""
    c = R.case(regime, sizes)
    want = R.ref64(c, steps)
    a = R.gaps(R.torch_step(c, steps, torch.float32, "cuda")[0], want, c["p0"])
    return c, want, a


class Run:
    """K calls of athd_head_step on guarded buffers"""

    def __init__(self, kt, c, steps=K, misaligned=(), hp=None, grad_scale=None, found_inf=None, grad_factor=1.0):
        native = _native()
        g = lambda i: MISALIGNED if i in misaligned else ALIGNED
        self.p = [kt.Buf(x, "f32", g(i), output=True) for i, x in enumerate(c["p0"])]
        self.m = [kt.Buf(np.zeros_like(x), "f32", g(i), output=True) for i, x in enumerate(c["p0"])]
        self.v = [kt.Buf(np.zeros_like(x), "f32", g(i), output=True) for i, x in enumerate(c["p0"])]
        self.grad_host = [[np.float32(grad_factor) * x for x in c["grads"][k]] for k in range(steps)]
        self.g = [[kt.Buf(x, "f32", g(i)) for i, x in enumerate(gs)] for gs in self.grad_host]
        for i in range(len(self.p)):
            for b in (self.p[i], self.m[i], self.v[i], self.g[0][i]):
                assert b.ptr % 16 == (4 if i in misaligned else 0)
        self.tables = [native.step_table([(self.p[i].ptr, self.g[k][i].ptr, self.m[i].ptr, self.v[i].ptr, self.p[i].n)
                                          for i in range(len(self.p))]) for k in range(steps)]
        self.hp = native.StepHparams(*[dict(R.HP, **(hp or {}))[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay",
                                                                             "max_norm")])
        self.nws = native.head_step_workspace_bytes(self.tables[0])
        # the workspace is not initialised by the caller: NaN bytes
        self.ws = torch.full((max(self.nws, 8),), 0xFF, dtype=torch.uint8, device="cuda")
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stats = torch.full((4,), -5.0, dtype=torch.float32, device="cuda")
        f = lambda x: None if x is None else torch.tensor([x], dtype=torch.float32, device="cuda")
        self.grad_scale, self.found_inf = f(grad_scale), f(found_inf)

    def call(self, k, n_tensors=None, table=None):
        native, ptr = _native(), lambda t: None if t is None else t.data_ptr()
        table = self.tables[k] if table is None else table
        return native.lib.athd_head_step(table, len(table) if n_tensors is None else n_tensors, self.hp,
                                         ptr(self.grad_scale), ptr(self.found_inf), self.step.data_ptr(),
                                         self.stats.data_ptr(), self.ws.data_ptr(), self.nws, _stream())

    def launch(self, graph=False):
        if graph:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, capture_error_mode="thread_local"):
                for k in range(len(self.tables)):
                    assert self.call(k) == 0
            gr.replay()
        else:
            for k in range(len(self.tables)):
                assert self.call(k) == 0
        return self

    def result(self, kt):
        kt.sync()
        out = {}
        for name, bufs in (("p", self.p), ("m", self.m), ("v", self.v)):
            out[name] = []
            for b in bufs:
                raw, bands = b.host()
                assert bands, "guard band of %s overwritten" % name
                out[name].append(raw)
        for gs, hs in zip(self.g, self.grad_host):
            for b, h in zip(gs, hs):
                raw, bands = b.host()
                assert bands and np.array_equal(raw.view(np.uint32), h.view(np.uint32)), "a gradient was written"
        out["stats"] = self.stats.cpu().numpy()
        out["step"] = int(self.step.item())
        return out


def _same_bits(a, b, what):
    for name in ("p", "m", "v"):
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: %s[%d] differs" % (what, name, i)
    assert np.array_equal(a["stats"].view(np.uint32), b["stats"].view(np.uint32)) and a["step"] == b["step"], what


def _f64(r):
    return {k: [x.astype(np.float64) for x in r[k]] for k in ("p", "m", "v")}


def _check_gaps(tag, got, want, a, p0):
    g = R.gaps(_f64(got), want, p0)
    ratio = {k: g[k] / a[k] for k in g}
    _report("head_step/" + tag, {"ratio_to_torch_f32_gap": ratio, "a": a})
    print(tag, "gap / a:", ratio, "a:", a)
    assert all(a[k] > 0 for k in a) and max(ratio.values()) <= R.ALLOW, (ratio, a)


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_kernel_steps(kt, regime):
    c, want, a = _refs(regime)
    runs = [Run(kt, c).launch(graph=(i == 3)).result(kt) for i in range(4)]       # three eager runs, one graph replay
    _same_bits(runs[0], runs[1], "second launch")
    _same_bits(runs[0], runs[2], "third launch")
    _same_bits(runs[0], runs[3], "graph replay")
    got = runs[0]
    _check_gaps(regime, got, want, a, c["p0"])
    norm, coef, skipped, t = got["stats"]
    assert abs(float(norm) - want["norm"][-1]) <= 2.0 ** -22 * want["norm"][-1], (norm, want["norm"][-1])
    assert skipped == 0.0 and t == float(K) and got["step"] == K
    if regime == "inactive":
        assert coef == 1.0
    else:
        assert abs(float(coef) - want["coef"][-1]) <= 2.0 ** -22 * want["coef"][-1]
    if regime == "active":
        assert coef < 0.01


def test_misaligned_pointers_give_the_same_bits(kt):
    c, want, a = _refs("active")
    base = Run(kt, c).launch().result(kt)
    got = Run(kt, c, misaligned=(5, 8)).launch().result(kt)               # 4095 and 8195 elements
    _same_bits(base, got, "misaligned")


@pytest.mark.parametrize("sizes", [(4097,), (5,) * 64], ids=["1-tensor", "64-tensors"])
def test_tensor_counts(kt, sizes):
    c, want, a = _refs("active", sizes)
    got = Run(kt, c).launch().result(kt)
    _check_gaps("%d-tensors" % len(sizes), got, want, a, c["p0"])
    assert got["step"] == K and got["stats"][2] == 0.0


def test_refused_calls_write_nothing(kt):
    native = _native()
    c = R.case("active", (5,) * 65)
    run = Run(kt, c, steps=1)
    assert run.nws == 0                                                   # 65 tensors
    before = run.result(kt)
    assert run.call(0) == -1
    ok = native.step_table([(run.p[i].ptr, run.g[0][i].ptr, run.m[i].ptr, run.v[i].ptr, 5) for i in range(64)])
    run.nws = native.head_step_workspace_bytes(ok)
    assert run.nws == 64 * 8
    assert run.call(0, n_tensors=0, table=ok) == -1
    zero = native.step_table([(run.p[0].ptr, run.g[0][0].ptr, run.m[0].ptr, run.v[0].ptr, 5),
                              (run.p[1].ptr, run.g[0][1].ptr, run.m[1].ptr, run.v[1].ptr, 0)])
    assert native.head_step_workspace_bytes(zero) == 0 and run.call(0, table=zero) == -1      # n = 0
    null = native.step_table([(run.p[0].ptr, None, run.m[0].ptr, run.v[0].ptr, 5)])
    assert run.call(0, table=null) == -1                                  # a null pointer
    odd = native.step_table([(run.p[0].ptr + 2, run.g[0][0].ptr, run.m[0].ptr, run.v[0].ptr, 4)])
    assert run.call(0, table=odd) == -1                                   # not 4-byte aligned
    run.nws -= 1
    assert run.call(0, table=ok) == -5                                    # a short workspace
    _same_bits(before, run.result(kt), "refused calls")
    assert before["step"] == 0 and np.all(before["stats"] == -5.0)


# ---------------------------------------------------------------------------------------------------- skip semantics
def test_found_inf_skips(kt):
    c = R.case("active")
    run = Run(kt, c, found_inf=1.0)
    before = {k: [b.host()[0] for b in getattr(run, k)] for k in ("p", "m", "v")}
    got = run.launch().result(kt)
    for k in before:
        for x, y in zip(before[k], got[k]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
    assert got["step"] == 0 and got["stats"][2] == 1.0 and got["stats"][3] == 0.0
    assert np.isfinite(got["stats"][0]) and got["stats"][0] > 1.0        # the norm is reported all the same


def test_non_finite_norm_skips(kt):
    c = R.case("active")
    grads = [[x.copy() for x in gs] for gs in c["grads"]]
    grads[0][7][4096] = np.inf                                            # the lone element of a tensor's second chunk
    run = Run(kt, {"p0": c["p0"], "grads": grads}, steps=1)
    before = {k: [b.host()[0] for b in getattr(run, k)] for k in ("p", "m", "v")}
    got = run.launch().result(kt)
    for k in before:
        for x, y in zip(before[k], got[k]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
    assert got["step"] == 0 and got["stats"][2] == 1.0 and np.isinf(got["stats"][0])


def test_power_of_two_grad_scale_is_exact(kt):
    c = R.case("inactive")
    base = Run(kt, c).launch().result(kt)
    got = Run(kt, c, grad_scale=8.0, grad_factor=8.0).launch().result(kt)
    _same_bits(base, got, "grad_scale = 8")


# ---------------------------------------------------------------------------------------------------- HeadAdamW
def _params(c):
    return [torch.nn.Parameter(torch.tensor(x).cuda()) for x in c["p0"]]


def _set_grads(params, c, k):
    for p, g in zip(params, c["grads"][k]):
        p.grad = torch.tensor(g).cuda()


def _state(params, opt):
    f = lambda xs: [x.detach().double().cpu().numpy() for x in xs]
    return {"p": f(params), "m": f([opt.state[p]["exp_avg"] for p in params]),
            "v": f([opt.state[p]["exp_avg_sq"] for p in params])}


def test_head_adamw_against_torch_and_state_dict_round_trip():
    from athd.optim import HeadAdamW
    hp = R.HP
    c, want, a = _refs("active")
    params = _params(c)
    idle = torch.nn.Parameter(torch.full((7,), 0.25, device="cuda"))      # never has a gradient
    opt = HeadAdamW(params + [idle], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"],
                    weight_decay=hp["weight_decay"])
    for k in range(K):
        _set_grads(params, c, k)
        opt.step(grad_clip=hp["max_norm"])
        for p, g in zip(params, c["grads"][k]):
            assert torch.equal(p.grad.cpu(), torch.tensor(g))             # gradients are read-only
    g = R.gaps(_state(params, opt), want, c["p0"])
    print("HeadAdamW gap / a:", {k: g[k] / a[k] for k in g})
    assert all(g[k] <= R.ALLOW * a[k] for k in g), (g, a)
    assert torch.equal(idle.detach().cpu(), torch.full((7,), 0.25)) and idle not in opt.state
    assert opt.step_count() == K and opt.last_stats.cpu().tolist()[2:] == [0.0, float(K)]
    for p in params:
        assert opt.state[p]["exp_avg"].data_ptr() % 16 == 0 and opt.state[p]["exp_avg_sq"].data_ptr() % 16 == 0
    # -> torch.optim.AdamW over copies of the parameters -> a fresh HeadAdamW; each takes the fourth step
    _, want4, a4 = _refs("active", tuple(R.SIZES), K + 1)
    sd = opt.state_dict()
    assert all(v["step"].device.type == "cpu" and float(v["step"]) == K for v in sd["state"].values())
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in params + [idle]]
    topt = torch.optim.AdamW(tparams, lr=1.0, foreach=False)
    topt.load_state_dict(sd)
    hparams = [torch.nn.Parameter(p.detach().clone()) for p in params + [idle]]
    hopt = HeadAdamW(hparams, lr=1.0)
    hopt.load_state_dict(topt.state_dict())
    assert hopt.param_groups[0]["lr"] == hp["lr"] and hopt.step_count() == K
    _set_grads(tparams[:-1], c, K)
    torch.nn.utils.clip_grad_norm_(tparams, hp["max_norm"], foreach=False)
    topt.step()
    _set_grads(hparams[:-1], c, K)
    hopt.step(grad_clip=hp["max_norm"])
    for name, ps, o in (("torch", tparams, topt), ("native", hparams, hopt)):
        g = R.gaps(_state(ps[:-1], o), want4, c["p0"])
        print(name, "fourth step gap / a:", {k: g[k] / a4[k] for k in g})
        assert all(g[k] <= R.ALLOW * a4[k] for k in g), (name, g, a4)
    assert hopt.step_count() == K + 1


def test_head_adamw_refuses_too_many_tensors():
    from athd.optim import HeadAdamW
    params = [torch.nn.Parameter(torch.zeros(2, device="cuda")) for _ in range(65)]
    opt = HeadAdamW(params)
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="at most 64"):
        opt.step()
    params[0].grad = None
    opt.step()                                                            # 64 live tensors are fine
    assert opt.step_count() == 1 and not bool(params[0].any()) and bool(params[1].any())


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model(state_dict, text_table):
    return _new_model(state_dict, text_table, "f32")


NATIVE = dict(native_output=True, native_cond=True, native_decoders=True)
LR, WD = 1e-3, 1e-2


def _batches3():
    from athd.synth import synthetic_batch
    B, T, _ = CASE_SHORT
    prompts = [["bass", "vocals"], ["drums", "other"], ["vocals", "drums"]]
    return [{"mixture": torch.as_tensor(synthetic_batch(B, T, seed0=300 + i)),
             "target": 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=400 + i)), "prompt": prompts[i]}
            for i in range(3)]


def test_train_epoch_with_head_adamw(model, state_dict, text_table, oracle_model):
    from athd.head import HeadTrainer, TrainableHead
    from athd.optim import HeadAdamW
    from athd.train import train_epoch
    from train_refs import train_epoch_ref
    batches = _batches3()

    def run():
        trainer = HeadTrainer(model, **NATIVE)
        p0 = {k: v.detach().clone() for k, v in trainer.head.state_dict().items()}
        opt = HeadAdamW(trainer.parameters(), lr=LR, weight_decay=WD)
        got = train_epoch(trainer, batches, opt, None, "cuda", False, False, None, None, 1.0, 0.9, 0.1, 0, 0)
        return got, p0, {k: v.detach().clone() for k, v in trainer.head.state_dict().items()}, opt

    got, p0, p1, opt = run()

    class Ref64(torch.nn.Module):                     # the float64 CPU loop of tests/test_gpu_head_cond.py, with AdamW
        def __init__(self):
            super().__init__()
            self.head = TrainableHead().double()
            self.head.load_state_dict(H.head_state(state_dict), strict=True)

        def forward(self, mixture, prompts):
            return self.head(H.oracle_features(oracle_model, mixture)[0], _rows(text_table, prompts).double())

    ref = Ref64()
    want = train_epoch_ref(ref, batches, torch.optim.AdamW(ref.parameters(), lr=LR, weight_decay=WD), "combined", 0.9,
                           0.1, 1.0)
    _report("head_train_epoch_head_adamw", {"got": got, "want": want})
    print("train_epoch:", got, want)
    for k in ("loss", "sdr", "sisdr"):
        assert abs(got[k] - want[k]) <= 1e-3, (k, got[k], want[k])
    assert len(p1) == 50 and opt.step_count() == 3
    for k in p1:
        assert bool(torch.isfinite(p1[k]).all()) and not torch.equal(p1[k], p0[k]), k           # all 50 moved
    # the dead tensors: exact-zero gradients, so m = v = 0, the Adam term is 0 and only the decay moves them
    for k in H.DEAD:
        w = p0[k].double() * (1.0 - LR * WD) ** 3
        ulp = torch.maximum(w.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64, device=w.device)).log2().floor()
        assert bool(((p1[k].double() - w).abs() <= 2.0 * torch.exp2(ulp - 23)).all()), k


def test_train_epoch_repeats_bit_equal(model):
    """Three steps twice from the same start give the same bits.  What is left to torch's autograd (`freq_out` /
    `time_out`, the attention vector) runs under `torch.backends.cudnn.deterministic`, torch's own switch for
    reproducible convolution gradients: without it torch's gradient of `time_out.weight` differs from run to run on an
    MI355X (no other gradient does, and none with the switch), and the metrics of two runs differed in the ninth digit
    (loss 5.694029979 against 5.694029975); every kernel of this library is bit-equal run to run (the tests above)."""
    from athd.head import HeadTrainer
    from athd.optim import HeadAdamW
    from athd.train import train_epoch
    batches = _batches3()
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        runs = []
        for _ in range(2):
            trainer = HeadTrainer(model, **NATIVE)
            opt = HeadAdamW(trainer.parameters(), lr=LR, weight_decay=WD)
            got = train_epoch(trainer, batches, opt, None, "cuda", False, False, None, None, 1.0, 0.9, 0.1, 0, 0)
            runs.append((got, {k: v.detach().clone() for k, v in trainer.head.state_dict().items()}))
    finally:
        torch.backends.cudnn.deterministic = saved
    print("repeat:", runs[0][0], runs[1][0])
    assert runs[0][0] == runs[1][0]
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k


def test_autocast_step_under_grad_scaler(model):
    from athd.head import HeadTrainer
    from athd.optim import HeadAdamW
    from athd.train import train_epoch
    trainer = HeadTrainer(model, **NATIVE)
    p0 = {k: v.detach().clone() for k, v in trainer.head.state_dict().items()}
    opt = HeadAdamW(trainer.parameters(), lr=LR, weight_decay=WD)
    scaler = torch.amp.GradScaler("cuda", init_scale=16.0)                # (tests/test_gpu_train.py: why 16)
    got = train_epoch(trainer, _batches3()[:1], opt, scaler, "cuda", True, False, None, None, 1.0, 0.9, 0.1, 0, 0)
    assert all(np.isfinite(v) for v in got.values())
    for k, v in trainer.head.state_dict().items():
        assert bool(torch.isfinite(v).all()) and not torch.equal(v, p0[k]), k
    assert scaler.get_scale() == 16.0                                     # the step was not skipped
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    norm, coef, skipped, t = opt.last_stats.cpu().tolist()
    assert skipped == 0.0 and t == 1.0 and np.isfinite(norm) and 0.0 < coef <= 1.0


def _write_split(root, n_tracks, n, seed):
    from athd.musdb import HQ_FILES, write_wav
    rng = np.random.default_rng(seed)
    for i in range(n_tracks):
        d = root / ("track%d" % i)
        d.mkdir(parents=True)
        stems = 0.1 * rng.standard_normal((4, n, 2)).astype(np.float32)
        for name, x in zip(HQ_FILES, [stems.sum(0)] + list(stems)):
            write_wav(d / (name + ".wav"), x, 44100)


def test_train_job(model, state_dict, text_table, tmp_path, capsys):
    from athd.inference import load_model
    from athd.train import train
    from athd.weights import STEMS
    _write_split(tmp_path / "train", 2, 5000, 1)
    _write_split(tmp_path / "test", 1, 5000, 2)
    cfg = {"data": {"train_dir": str(tmp_path / "train"), "test_dir": str(tmp_path / "test"), "sample_rate": 44100,
                    "segment_seconds": 0.0929, "pct_train": 0.25, "pct_test": 0.5},
           "model": {},
           "training": {"batch_size": 2, "num_epochs": 2, "optimizer": {"lr": 1e-3, "weight_decay": 1e-2, "grad_clip": 1.0},
                        "L1_comb_loss": {}, "loss_weights": {}},
           "wandb": {"use_wandb": False, "checkpoint_dir": str(tmp_path / "ck"), "log_every": 1}}
    assert int(44100 * 0.0929) == 4096
    # every prompt the datasets can draw has a row (the four stem names keep the shared table's rows); its own model,
    # since train() syncs the head into it
    from athd.model import AudioTextHTDemucs
    from athd.musdb import STEM_PROMPTS
    from athd.weights import synthetic_text_table
    prompts = sorted({p for ps in STEM_PROMPTS.values() for p in ps} - set(STEMS))
    extra = synthetic_text_table(len(prompts), seed=11)
    table = {s: text_table[i] for i, s in enumerate(STEMS)}
    table.update({p: extra[i] for i, p in enumerate(prompts)})
    m = AudioTextHTDemucs(dtype="f32", text_table=table)
    m.load_state_dict(state_dict)
    m.to("cuda").eval()
    torch.manual_seed(5)
    out = train(cfg, model=m)
    text = capsys.readouterr().out
    assert set(out) == {"final_train_metrics", "final_val_metrics", "best_sdr"}
    assert all(np.isfinite(v) for v in out["final_train_metrics"].values())
    assert all(np.isfinite(v) for v in out["final_val_metrics"].values()) and np.isfinite(out["best_sdr"])
    assert set(out["final_train_metrics"]) == {"loss", "sdr", "sisdr"}
    assert {"loss", "sdr", "sisdr"} < set(out["final_val_metrics"])      # plus sdr/{stem} of the stems drawn
    assert "Epoch 2/2" in text and "Training complete!" in text and "Trainable parameters: 2,983,804" in text
    ck = tmp_path / "ck"
    assert sorted(p.name for p in ck.iterdir()) == ["best_model.pt", "checkpoint_epoch_1.pt", "checkpoint_epoch_2.pt",
                                                    "latest.pt"]
    # latest.pt through load_model: the same forward as the trained, synced model, bit for bit
    loaded = load_model(str(ck / "latest.pt"), "cuda", dtype="f32", text_table=table)
    wav = _wav().cuda()
    assert torch.equal(loaded(wav, ["bass", "vocals"]), m(wav, ["bass", "vocals"]))
    assert not torch.equal(m(wav, ["bass", "vocals"]), model(wav, ["bass", "vocals"]))         # and it did train
    # a second call on the same directory resumes at epoch 2 and runs no step
    again = train(cfg, model=m)
    text = capsys.readouterr().out
    assert "Found latest checkpoint" in text and "Loaded checkpoint from epoch 2" in text and "Skipping" not in text
    assert "Epoch 1/2" not in text and "Epoch 2/2" not in text and again["final_train_metrics"] == {}
    assert sorted(p.name for p in ck.iterdir()) == ["best_model.pt", "checkpoint_epoch_1.pt", "checkpoint_epoch_2.pt",
                                                    "latest.pt"]
