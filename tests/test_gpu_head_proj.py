"""Head training's native output projections and attention vector on the GPU (include/athd.h `athd_head_proj`,
`athd_head_proj_backward`, `athd_head_attn_vec`, `athd_head_attn_vec_backward`; athd/head.py `NativeProjOutput`,
`NativeAttnVector`, `TrainableHead(native_proj=True)`; athd/train.py `train(seed=)`).

Kernel level, on the shapes of `head_proj_refs.PROJ_CASES` / `ATTN_CASES` with guard bands round every buffer and NaN in
every output: both directions overwrite every element, are bit-equal run to run and under graph replay, bit-equal between
a float32 and a bf16 context, with the workspace prefilled with 0xFF and then 0x5A, and every tensor lies within ALLOW = 4
units of the float64 reference, the unit being max(a, floor): `a` the gap of torch's own float32 ops on the same GPU,
`floor` the rounding floor derived in tests/head_proj_refs.py (tests/test_head_proj_refs.py shows that a float32
evaluation reaches that and that planted defects do not).

End to end with all four native options at B = 2, T = 4096 and T = 5000, and with `native_decoders` off at T = 4096:
every one of the 50 tensors has a gradient, the live ones within 4 x the oracle's f32-against-f64 gap, the dead ones
exactly zero; the output against the torch head at F32_SDR_DB; three `train_epoch` steps with `HeadAdamW` within 1e-3 of
the float64 CPU loop; one autocast step under `GradScaler`; the refusals.

Reproducibility, with `torch.backends.cudnn.deterministic` explicitly off: three `train_epoch` steps twice from the same
start give equal metrics and 50 bit-equal tensors, and `train(cfg, model=..., seed=5)` twice into two directories writes
bit-equal model and optimizer tensors into `latest.pt`.
"""
import functools

import numpy as np
import pytest
import torch

import head_proj_refs as R
import head_refs as H
from test_gpu_head_cond import _get, _in, _lib, _new_model, _out, _rows, _stream, kt, models  # noqa: F401 (fixtures)
from test_gpu_head_dec import _oracle_grads, _target, _wav
from test_gpu_parity import F32_SDR_DB, _report

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
PROJ_IDS = ["-".join(str(int(v)) for v in c) for c in R.PROJ_CASES]
ALL4 = dict(native_output=True, native_cond=True, native_decoders=True, native_proj=True)
NO_DEC = dict(native_output=True, native_cond=True, native_proj=True)
E2E = [(ALL4, 4096), (ALL4, 5000), (NO_DEC, 4096)]
E2E_IDS = ["all4-4096", "all4-5000", "torchdec-4096"]
EINVAL, ESTATE, EWORKSPACE = -1, -3, -5
D, TEXT = R.D, R.TEXT
LR, WD = 1e-3, 1e-2


def _bits(o):
    return {k: v.view(np.uint32) for k, v in o.items()}


def _protocol(models, kt, sizes, launch, nws):
    """the house protocol: per context dtype two plain runs and one graph replay on fresh NaN outputs, the workspace
    filled with 0xFF, 0x5A, 0xFF; -> the float32 context's outputs"""
    runs = {}
    for dt in DTYPES:
        h = models[dt]._ensure_ctx().h
        res = []
        for i in range(3):
            ws = torch.full((max(nws, 16),), 0xFF if i != 1 else 0x5A, dtype=torch.uint8, device="cuda")
            outs = {k: _out(kt, n) for k, n in sizes.items()}
            if i < 2:
                launch(h, outs, ws)
            else:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    launch(h, outs, ws)
                graph.replay()
            kt.sync()
            res.append({k: _get(b) for k, b in outs.items()})
        for k, v in res[0].items():
            assert np.isfinite(v).all(), "%s: elements not written" % k
            assert np.array_equal(_bits(res[0])[k], _bits(res[1])[k]), "%s: repeat launch differs" % k
            assert np.array_equal(_bits(res[0])[k], _bits(res[2])[k]), "%s: graph replay differs" % k
        runs[dt] = res[0]
    for k in sizes:                                                   # one f32 variant serves both context dtypes
        assert np.array_equal(_bits(runs["f32"])[k], _bits(runs["bf16"])[k]), k
    return runs["f32"]


# ------------------------------------------------------------------------------------------------ the projection
@functools.lru_cache(maxsize=None)
def _proj_gpu_gap(shape):
    c, g64, _, _ = R.proj_refs(shape)
    g32 = R.proj_autograd(c, torch.float32, "cuda")
    return {k: R.gap(g32[k], g64[k]) for k in R.PROJ_NAMES}


@pytest.mark.parametrize("shape", R.PROJ_CASES, ids=PROJ_IDS)
def test_proj_kernels(models, kt, shape):
    B, Rr, S, cf, scale = shape
    c, g64, _, floor = R.proj_refs(shape)
    unit = R.units(_proj_gpu_gap(shape), floor)
    lib = _lib()
    ins = {k: _in(kt, c[k].numpy()) for k in ("x", "w", "b", "gy")}
    sc = _in(kt, c["scale"].numpy()) if scale else None
    nws = lib.athd_head_proj_workspace_bytes(B, Rr, S)
    assert nws > 0
    n = B * Rr * S
    sizes = dict(y=2 * n, x=4 * n, w=8, b=2)

    def launch(h, outs, ws):
        s = _stream()
        rc = lib.athd_head_proj(h, ins["x"].ptr, ins["w"].ptr, ins["b"].ptr, B, Rr, S, outs["y"].ptr, s)
        assert rc == 0, lib.athd_last_error(h)
        rc = lib.athd_head_proj_backward(h, ins["gy"].ptr, cf, sc.ptr if sc else None, ins["x"].ptr, ins["w"].ptr, B, Rr,
                                         S, outs["x"].ptr, outs["w"].ptr, outs["b"].ptr, ws.data_ptr(), nws, s)
        assert rc == 0, lib.athd_last_error(h)

    run = _protocol(models, kt, sizes, launch, nws)
    for b in list(ins.values()) + ([sc] if sc else []):
        _get(b)
    got = {k: run[k].astype(np.float64).reshape(g64[k].shape) for k in R.PROJ_NAMES}
    ratio = R.ratios({k: R.gap(got[k], g64[k]) for k in R.PROJ_NAMES}, unit)
    _report("head_proj/" + "-".join(str(int(v)) for v in shape), {"ratio_to_unit": ratio, "unit": unit})
    print(shape, "gap / unit:", ratio, "unit:", unit)
    assert max(ratio.values()) <= R.ALLOW, (ratio, unit)


def test_proj_argument_errors(models, kt):
    from athd import native
    lib = _lib()
    h, s = models["f32"]._ensure_ctx().h, _stream()
    B, Rr, S = 2, 3, 5
    buf = torch.zeros(4 * B * Rr * S + 64, dtype=torch.float32, device="cuda")
    nws = lib.athd_head_proj_workspace_bytes(B, Rr, S)
    assert nws == 2 * 80
    ws = torch.zeros(nws + 16, dtype=torch.uint8, device="cuda")
    p, w = buf.data_ptr(), ws.data_ptr()

    def fwd(h_=h, x=p, wt=p, bias=p, B_=B, R_=Rr, S_=S, y=p):
        return lib.athd_head_proj(h_, x, wt, bias, B_, R_, S_, y, s)

    def bwd(h_=h, gy=p, cf=0, scale=None, x=p, wt=p, B_=B, R_=Rr, S_=S, gx=p, gw=p, gb=p, w_=w, n_=nws):
        return lib.athd_head_proj_backward(h_, gy, cf, scale, x, wt, B_, R_, S_, gx, gw, gb, w_, n_, s)

    for kw in (dict(x=None), dict(wt=None), dict(bias=None), dict(y=None)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(gy=None), dict(x=None), dict(wt=None), dict(gx=None), dict(gw=None), dict(gb=None)):
        assert bwd(**kw) == EINVAL, kw
    assert b"null" in lib.athd_last_error(h)
    # the shape, refused on the arguments alone
    for kw in (dict(B_=0), dict(B_=65536), dict(R_=0), dict(R_=4097), dict(S_=0), dict(S_=(1 << 22) + 1),
               dict(R_=2, S_=1 << 22), dict(R_=4096, S_=1025)):
        a = dict(B_=B, R_=Rr, S_=S)
        a.update(kw)
        assert lib.athd_head_proj_workspace_bytes(a["B_"], a["R_"], a["S_"]) == 0, kw
        assert fwd(**kw) == EINVAL and bwd(**kw) == EINVAL, kw
    # a 2048 x 2048 grid and 47 s of samples with R = 1 are inside
    assert lib.athd_head_proj_workspace_bytes(1, 2048, 2048) > 0 and lib.athd_head_proj_workspace_bytes(1, 1, 2072700) > 0
    # misaligned: the big tensors to 16 bytes, the small ones to 4, the workspace to 16
    assert fwd(x=p + 4) == EINVAL and fwd(y=p + 8) == EINVAL and fwd(wt=p + 2) == EINVAL and fwd(bias=p + 1) == EINVAL
    assert bwd(gy=p + 4) == EINVAL and bwd(x=p + 4) == EINVAL and bwd(gx=p + 8) == EINVAL
    assert bwd(wt=p + 2) == EINVAL and bwd(gw=p + 2) == EINVAL and bwd(gb=p + 1) == EINVAL and bwd(scale=p + 2) == EINVAL
    assert bwd(w_=w + 4) == EINVAL
    # a short or missing workspace
    assert bwd(n_=nws - 1) == EWORKSPACE and bwd(w_=None) == EWORKSPACE and bwd(n_=0) == EWORKSPACE
    # the order: the state before the arguments, the arguments before the workspace
    assert bwd(gy=None, n_=0) == EINVAL and bwd(R_=0, n_=0) == EINVAL and bwd(gx=p + 4, n_=0) == EINVAL
    fresh = native.Context(0, native.F32)
    assert fwd(h_=fresh.h) == ESTATE and bwd(h_=fresh.h) == ESTATE
    assert fwd(h_=fresh.h, x=None) == ESTATE and bwd(h_=fresh.h, B_=0, n_=0) == ESTATE
    fresh.close()
    assert fwd(h_=None) == EINVAL and bwd(h_=None) == EINVAL
    kt.sync()
    assert not bool(buf.any()) and not bool(ws.any())                     # nothing was written by the refused calls


# ------------------------------------------------------------------------------------------ the attention vector
ATTN_SHAPES = dict(a=(-1, D), keep=(-1, 2 * D), wv=(D, TEXT), bv=(D,), w_in=(3 * D, D), b_in=(3 * D,), wo=(D, D),
                   bo=(D,))


@functools.lru_cache(maxsize=None)
def _attn_gpu_gap(B):
    c, g64, _, _ = R.attn_refs(B)
    return R.attn_gaps(R.attn_autograd(c, torch.float32, "cuda"), g64)


@pytest.mark.parametrize("B", R.ATTN_CASES)
def test_attn_vec_kernels(models, kt, B):
    c, g64, _, floor = R.attn_refs(B)
    unit = R.units(_attn_gpu_gap(B), floor)
    lib = _lib()
    w = R.attn_weights(c, np.float32)
    ins = {k: _in(kt, v) for k, v in w.items()}
    ins.update(text=_in(kt, c["text"].numpy()), ga=_in(kt, c["ga"].numpy()))
    sizes = {k: int(np.prod([B if v < 0 else v for v in sh])) for k, sh in ATTN_SHAPES.items()}

    def launch(h, outs, ws):
        s = _stream()
        rc = lib.athd_head_attn_vec(h, ins["text"].ptr, *[ins[k].ptr for k in ("wv", "bv", "w_in", "b_in", "wo", "bo")],
                                    B, outs["a"].ptr, outs["keep"].ptr, s)
        assert rc == 0, lib.athd_last_error(h)
        # (the backward reads the forward's keep where the forward wrote it: the same stream orders the two)
        rc = lib.athd_head_attn_vec_backward(h, ins["ga"].ptr, ins["text"].ptr, outs["keep"].ptr, ins["w_in"].ptr,
                                             ins["wo"].ptr, B, *[outs[k].ptr for k in ("wv", "bv", "w_in", "b_in", "wo",
                                                                                        "bo")], s)
        assert rc == 0, lib.athd_last_error(h)

    run = _protocol(models, kt, sizes, launch, 0)
    for b in ins.values():
        _get(b)
    got = R._split({k: run[k].astype(np.float64).reshape([B if v < 0 else v for v in ATTN_SHAPES[k]])
                    for k in ATTN_SHAPES if k != "keep"})
    assert not got["w_in_dead"].any() and not got["b_in_dead"].any()      # exact zeros, not small values
    ratio = R.ratios(R.attn_gaps(got, g64), unit)
    _report("head_attn_vec/%d" % B, {"ratio_to_unit": ratio, "unit": unit})
    print(B, "gap / unit:", ratio, "unit:", unit)
    assert max(ratio.values()) <= R.ALLOW, (ratio, unit)


def test_attn_vec_forward_beyond_the_backward_limit(models, kt):
    """the forward takes B up to 65535; only the backward, which parks its intermediates in grad_w_in, stops at 384"""
    B = 385
    c, g64, _, floor = R.attn_refs(B)
    a_gpu = _attn_gpu_gap(B)
    lib, h = _lib(), models["f32"]._ensure_ctx().h
    ins = {k: _in(kt, v) for k, v in R.attn_weights(c, np.float32).items()}
    ins["text"] = _in(kt, c["text"].numpy())
    outs = dict(a=_out(kt, B * D), keep=_out(kt, 2 * B * D))
    rc = lib.athd_head_attn_vec(h, ins["text"].ptr, *[ins[k].ptr for k in ("wv", "bv", "w_in", "b_in", "wo", "bo")], B,
                                outs["a"].ptr, outs["keep"].ptr, _stream())
    assert rc == 0, lib.athd_last_error(h)
    kt.sync()
    got, keep = _get(outs["a"]), _get(outs["keep"])
    assert np.isfinite(got).all() and np.isfinite(keep).all()
    assert R.gap(got.astype(np.float64).reshape(B, D), g64["a"]) <= R.ALLOW * max(a_gpu["a"], floor["a"])


def test_attn_vec_argument_errors(models, kt):
    from athd import native
    lib = _lib()
    h, s = models["f32"]._ensure_ctx().h, _stream()
    buf = torch.zeros(3 * D * TEXT, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    names_f = ["text", "wv", "bv", "w_in", "b_in", "wo", "bo", "a", "keep"]
    names_b = ["ga", "text", "keep", "w_in", "wo", "gwv", "gbv", "gw_in", "gb_in", "gwo", "gbo"]

    def fwd(h_=h, B_=2, **kw):
        v = [kw.get(k, p) for k in names_f]
        return lib.athd_head_attn_vec(h_, *v[:7], B_, *v[7:], s)

    def bwd(h_=h, B_=2, **kw):
        v = [kw.get(k, p) for k in names_b]
        return lib.athd_head_attn_vec_backward(h_, *v[:5], B_, *v[5:], s)

    for k in names_f:
        assert fwd(**{k: None}) == EINVAL and fwd(**{k: p + 2}) == EINVAL, k
    for k in names_b:
        assert bwd(**{k: None}) == EINVAL and bwd(**{k: p + 2}) == EINVAL, k
    for B_ in (0, -1, 65536):
        assert fwd(B_=B_) == EINVAL and bwd(B_=B_) == EINVAL, B_
    assert bwd(B_=385) == EINVAL                                          # the backward's own limit (include/athd.h)
    fresh = native.Context(0, native.F32)
    assert fwd(h_=fresh.h) == ESTATE and bwd(h_=fresh.h) == ESTATE
    assert fwd(h_=fresh.h, text=None) == ESTATE and bwd(h_=fresh.h, B_=0) == ESTATE
    fresh.close()
    assert fwd(h_=None) == EINVAL and bwd(h_=None) == EINVAL
    kt.sync()
    assert not bool(buf.any())                                            # nothing was written by the refused calls


# ---------------------------------------------------------------------------------------------------- end to end
def test_native_proj_refuses_what_it_does_not_cover(models):
    from athd.head import HeadTrainer, TrainableHead
    m = models["f32"]
    f = m.encode(torch.zeros(1, 2, 4096, device="cuda"))
    text = torch.zeros(1, 512)
    assert not TrainableHead().native_proj and not HeadTrainer(m).head.native_proj        # off by default
    with pytest.raises(RuntimeError, match="native_proj.*native_output=True and native_cond=True"):
        HeadTrainer(m, native_proj=True, native_cond=True).head(f, text.cuda())
    with pytest.raises(RuntimeError, match="native_proj.*native_output=True and native_cond=True"):
        HeadTrainer(m, native_proj=True, native_output=True).head(f, text.cuda())
    on = dict(native_proj=True, native_output=True, native_cond=True)
    with pytest.raises(RuntimeError, match="native_proj.*bind"):
        TrainableHead(**on).cuda()(f, text)                               # an unbound head
    with pytest.raises(RuntimeError, match="native_proj.*float32"):
        TrainableHead(**on).bind(m).double().cuda()(f, text)
    with pytest.raises(RuntimeError, match="native_proj.*float32"):
        TrainableHead(**on).bind(m)(f, text)                              # a CPU head
    # a decoder that emits another length than the segment's: the resize is not kept inside
    head = HeadTrainer(m, **on).head
    with pytest.raises(RuntimeError, match="native_proj.*length 4000"):
        head(f._replace(length=4000), text.cuda())
    for dec in (False, True):                                             # independent of native_decoders
        t = HeadTrainer(m, native_decoders=dec, **on)
        assert (t.head.native_proj, t.head.native_decoders) == (True, dec)
        with torch.no_grad():
            y = t.head(f, text.cuda())
        assert y.shape == (1, 2, 4096) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("opt,T", E2E, ids=E2E_IDS)
def test_gradients_against_float64(models, oracle_model, state_dict, text_table, opt, T):
    from athd.head import HeadTrainer
    from athd.loss import combined_loss
    prompts = ["bass", "vocals"]
    m = models["f32"]
    trainer = HeadTrainer(m, **opt)
    assert trainer.head.native_proj and trainer.head.native_decoders == bool(opt.get("native_decoders"))
    trainer.train()
    combined_loss(trainer(_wav(T).cuda(), prompts), _target(T).cuda())[0].backward()
    params = dict(trainer.head.named_parameters())
    assert len(params) == 50
    missing = [k for k, p in params.items() if p.grad is None]
    assert not missing, missing
    got = {k: p.grad.detach().cpu().double() for k, p in params.items()}
    g64, g32 = _oracle_grads(m, oracle_model, state_dict, text_table, prompts, T)
    worst = {}
    for k, w in g64.items():
        if k in H.DEAD:
            assert not bool(got[k].any()), k                              # exactly zero
            continue
        mx = float(w.abs().max())
        a = float((g32[k].double() - w).abs().max()) / mx
        worst[k] = float((got[k] - w).abs().max()) / mx / a
    for k in ("text_attn.attn.in_proj_weight", "text_attn.attn.in_proj_bias"):
        assert not bool(got[k][:768].any()) and bool(got[k][768:].any()), k
    top = max(worst, key=worst.get)
    _report("head_grad_native_proj_%s_T%d_f32_vs_f64" % ("_".join(sorted(opt)), T),
            {"worst_ratio_to_oracle_f32_gap": worst[top], "tensor": top})
    print(sorted(opt), T, "worst gap / oracle f32 gap:", top, worst[top])
    bad = {k: v for k, v in worst.items() if v > 4.0}
    assert not bad, bad


@pytest.mark.parametrize("opt,T", E2E, ids=E2E_IDS)
def test_output_against_torch_head(models, text_table, opt, T):
    from athd.head import TrainableHead
    m = models["f32"]
    wav = _wav(T).cuda()
    text = _rows(text_table, ["bass", "vocals"])
    head = TrainableHead.from_model(m).cuda().eval()
    feats = m.encode(wav)
    with torch.no_grad():
        want = head(feats, text)
        for k, v in opt.items():
            setattr(head, k, v)
        got = head.bind(m)(feats, text)
    assert got.shape == want.shape and got.dtype == torch.float32
    s = H.sdr_db(want.cpu().numpy(), got.cpu().numpy())
    _report("head_native_proj_%s_T%d_vs_torch_head" % ("_".join(sorted(opt)), T), {"out": s})
    print(sorted(opt), T, s)
    assert s >= F32_SDR_DB, s


def _batches3(T):
    from athd.synth import synthetic_batch
    prompts = [["bass", "vocals"], ["drums", "other"], ["vocals", "drums"]]
    return [{"mixture": torch.as_tensor(synthetic_batch(2, T, seed0=300 + i)),
             "target": 0.5 * torch.as_tensor(synthetic_batch(2, T, seed0=400 + i)), "prompt": prompts[i]}
            for i in range(3)]


_ref_epoch = {}


@pytest.mark.parametrize("opt,T", E2E, ids=E2E_IDS)
def test_train_epoch_with_head_adamw_matches_float64_loop(state_dict, text_table, oracle_model, opt, T):
    from athd.head import HeadTrainer, TrainableHead
    from athd.optim import HeadAdamW
    from athd.train import train_epoch
    from train_refs import train_epoch_ref
    batches = _batches3(T)
    trainer = HeadTrainer(_new_model(state_dict, text_table, "f32"), **opt)
    got = train_epoch(trainer, batches, HeadAdamW(trainer.parameters(), lr=LR, weight_decay=WD), None, "cuda", False,
                      False, None, None, 1.0, 0.9, 0.1, 0, 0)

    class Ref64(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.head = TrainableHead().double()
            self.head.load_state_dict(H.head_state(state_dict), strict=True)

        def forward(self, mixture, prompts):
            return self.head(H.oracle_features(oracle_model, mixture)[0], _rows(text_table, prompts).double())

    if T not in _ref_epoch:                                               # the float64 CPU loop, once per length
        ref = Ref64()
        _ref_epoch[T] = train_epoch_ref(ref, batches, torch.optim.AdamW(ref.parameters(), lr=LR, weight_decay=WD),
                                        "combined", 0.9, 0.1, 1.0)
    want = _ref_epoch[T]
    _report("head_train_epoch_native_proj_%s_T%d" % ("_".join(sorted(opt)), T), {"got": got, "want": want})
    print(sorted(opt), T, got, want)
    for k in ("loss", "sdr", "sisdr"):
        assert abs(got[k] - want[k]) <= 1e-3, (k, got[k], want[k])


def test_autocast_step_under_grad_scaler(models):
    from athd.head import HeadTrainer
    from athd.optim import HeadAdamW
    from athd.train import train_epoch
    trainer = HeadTrainer(models["f32"], **ALL4)
    scaler = torch.amp.GradScaler("cuda", init_scale=16.0)                # (tests/test_gpu_train.py: why 16)
    opt = HeadAdamW(trainer.parameters(), lr=LR, weight_decay=WD)         # (the trainer's own copy of the head moves)
    got = train_epoch(trainer, _batches3(4096)[:1], opt, scaler, "cuda", True, False, None, None, 1.0, 0.9, 0.1, 0, 0)
    assert all(np.isfinite(v) for v in got.values())
    for k, p in trainer.head.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
    assert bool(trainer.head.time_out.weight.grad.any()) and bool(trainer.head.text_attn.v_proj.weight.grad.any())
    assert scaler.get_scale() == 16.0 and opt.last_stats.cpu().tolist()[2] == 0.0      # the step was not skipped


# ------------------------------------------------------------------------------------------------ reproducibility
def test_train_epoch_repeats_bit_equal_without_torch_switches(models):
    """Three steps twice from the same start, `torch.backends.cudnn.deterministic` explicitly off: with `native_proj` no
    gradient is torch's, so the metrics are equal and all 50 tensors bit-equal.  (Without the option torch's gradient of
    `time_out.weight` differs from run to run: tests/test_gpu_head_step.py::test_train_epoch_repeats_bit_equal.)"""
    from athd.head import HeadTrainer
    from athd.optim import HeadAdamW
    from athd.train import train_epoch
    batches = _batches3(4096)
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = False
    try:
        runs = []
        for _ in range(2):
            trainer = HeadTrainer(models["f32"], **ALL4)
            opt = HeadAdamW(trainer.parameters(), lr=LR, weight_decay=WD)
            got = train_epoch(trainer, batches, opt, None, "cuda", False, False, None, None, 1.0, 0.9, 0.1, 0, 0)
            runs.append((got, {k: v.detach().clone() for k, v in trainer.head.state_dict().items()}))
    finally:
        torch.backends.cudnn.deterministic = saved
    print("repeat:", runs[0][0], runs[1][0])
    assert runs[0][0] == runs[1][0]
    assert len(runs[0][1]) == 50
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k


def test_train_job_repeats_bit_equal_from_a_seed(state_dict, text_table, tmp_path):
    """`train(cfg, model=..., seed=5)` twice into two directories, on the tiny splits of
    tests/test_gpu_head_step.py::test_train_job: every model tensor and every optimizer state tensor of the two
    `latest.pt` files is bit-equal."""
    from athd.model import AudioTextHTDemucs
    from athd.musdb import STEM_PROMPTS
    from athd.train import train
    from athd.weights import STEMS, synthetic_text_table
    from test_gpu_head_step import _write_split
    _write_split(tmp_path / "train", 2, 5000, 1)
    _write_split(tmp_path / "test", 1, 5000, 2)
    prompts = sorted({p for ps in STEM_PROMPTS.values() for p in ps} - set(STEMS))
    extra = synthetic_text_table(len(prompts), seed=11)
    table = {s: text_table[i] for i, s in enumerate(STEMS)}
    table.update({p: extra[i] for i, p in enumerate(prompts)})
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = False
    try:
        cks = []
        for run in ("a", "b"):
            cfg = {"data": {"train_dir": str(tmp_path / "train"), "test_dir": str(tmp_path / "test"),
                            "sample_rate": 44100, "segment_seconds": 0.0929, "pct_train": 0.25, "pct_test": 0.5},
                   "model": {},
                   "training": {"batch_size": 2, "num_epochs": 2,
                                "optimizer": {"lr": 1e-3, "weight_decay": 1e-2, "grad_clip": 1.0}, "L1_comb_loss": {},
                                "loss_weights": {}},
                   "wandb": {"use_wandb": False, "checkpoint_dir": str(tmp_path / ("ck_" + run)), "log_every": 1}}
            m = AudioTextHTDemucs(dtype="f32", text_table=table)          # its own model: train() syncs the head into it
            m.load_state_dict(state_dict)
            m.to("cuda").eval()
            out = train(cfg, model=m, seed=5)
            cks.append((out, torch.load(tmp_path / ("ck_" + run) / "latest.pt", map_location="cpu", weights_only=True)))
    finally:
        torch.backends.cudnn.deterministic = saved
    (out_a, a), (out_b, b) = cks
    assert out_a == out_b and a["epoch"] == b["epoch"] == 2 and a["metrics"] == b["metrics"]
    assert set(a["model_state_dict"]) == set(b["model_state_dict"])
    for k, v in a["model_state_dict"].items():
        assert torch.equal(v, b["model_state_dict"][k]), k
    sa, sb = a["optimizer_state_dict"]["state"], b["optimizer_state_dict"]["state"]
    assert set(sa) == set(sb) and len(sa) == 50
    for i in sa:
        for k, v in sa[i].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(sb[i][k])), (i, k)
    # and it did train: the head moved away from the start
    assert not torch.equal(a["model_state_dict"]["time_out.weight"], torch.as_tensor(state_dict["time_out.weight"]))
