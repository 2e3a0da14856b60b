"""Head training's native decoder levels on the GPU (include/athd.h `athd_head_dec_level`, `athd_head_dec_level_backward`;
athd/head.py `NativeDecoderLevel`, `TrainableHead(native_decoders=True)`).

Kernel level, on the shapes of `head_dec_refs.CASES` with guard bands round every buffer and NaN in every output: both
directions overwrite every element, are bit-equal run to run and under graph replay, bit-equal between a float32 and a
bf16 context, and the output and every gradient (input, weight, bias, GroupNorm weight and bias) lie within ALLOW = 4
times `a` of the float64 reference, `a` being the gap of torch's own float32 `_Decoder` level on the same GPU to that
reference (tests/test_head_dec_refs.py shows that a float32 evaluation reaches that and that planted defects do not).

End to end with `HeadTrainer(model, native_decoders=True)` and with all three native options, at CASE_SHORT (B = 2,
T = 4096) and at B = 2, T = 5000, the smallest length at which the time decoder resizes (L = 5000, 1250, 313, 79, 20:
80 -> 79, 316 -> 313, 1252 -> 1250) and where Ts = 5, so the frequency decoder both up- and downsamples: every one of
the 50 tensors has a gradient, the live ones within 4 x the oracle's f32-against-f64 gap, the dead ones exactly zero
with `native_cond`; the output against the torch head at F32_SDR_DB = 110 dB; three `train_epoch` steps within 1e-3 dB
of the float64 CPU loop; one autocast step with finite float32 gradients.
"""
import functools

import numpy as np
import pytest
import torch

import head_dec_refs as R
import head_refs as H
from test_gpu_head_cond import _get, _in, _lib, _new_model, _out, _rows, _stream, kt, models  # noqa: F401 (fixtures)
from test_gpu_parity import F32_SDR_DB, _report

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
IDS = ["-".join(str(v) for v in c) for c in R.CASES]
OPTIONS = [dict(native_decoders=True), dict(native_decoders=True, native_cond=True, native_output=True)]
OPT_IDS = ["dec", "dec+cond+output"]
LENGTHS = [4096, 5000]
GRADS = ["x", "w", "b", "gamma", "beta"]                        # athd_head_dec_level_backward's outputs, in its order
EINVAL, ESTATE, EWORKSPACE = -1, -3, -5


@functools.lru_cache(maxsize=None)
def _gpu_gap(shape):
    """torch's float32 `torch_level` on this GPU against the float64 reference, per tensor"""
    c, g64, _ = R.refs(shape)
    return R.gaps(R.autograd(c, torch.float32, "cuda"), g64)


def _sizes(shape):
    level, B, M, inner, Lt, S = shape
    Ci, Co = R.LEVELS[level]
    s = dict(y=B * Co * Lt * inner, x=B * Ci * M * inner, w=Ci * Co * 8, b=Co)
    if level < 3:
        s.update(stats=2 * B, gamma=Co, beta=Co)
    return s


def _launch(lib, h, shape, ins, outs, ws, nws):
    level, B, M, inner, Lt, S = shape
    s = _stream()
    ptr = lambda d, k: d[k].ptr if k in d else None
    par = [ptr(ins, k) for k in ("w", "b", "gamma", "beta")]
    rc = lib.athd_head_dec_level(h, level, ins["x"].ptr, *par, ins["skip"].ptr, B, M, inner, S, Lt, outs["y"].ptr,
                                 ptr(outs, "stats"), ws.data_ptr(), nws, s)
    assert rc == 0, lib.athd_last_error(h)
    # (the backward reads the forward's stats where the forward wrote them: the same stream orders the two)
    rc = lib.athd_head_dec_level_backward(h, level, ins["gy"].ptr, ins["x"].ptr, *par, ptr(outs, "stats"), B, M, inner,
                                          Lt, *[ptr(outs, k) for k in GRADS], ws.data_ptr(), nws, s)
    assert rc == 0, lib.athd_last_error(h)


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_kernels(models, kt, shape):
    level, B, M, inner, Lt, S = shape
    c, g64, _ = R.refs(shape)
    a_gpu = _gpu_gap(shape)
    lib = _lib()
    keys = ["x", "w", "b", "skip", "gy"] + (["gamma", "beta"] if level < 3 else [])
    ins = {k: _in(kt, c[k].numpy()) for k in keys}
    nws = lib.athd_head_dec_workspace_bytes(level, B, M, inner, Lt)
    assert nws > 0
    sizes = _sizes(shape)
    bits = lambda o: {k: v.view(np.uint32) for k, v in o.items()}
    runs = {}
    for dt in DTYPES:
        h = models[dt]._ensure_ctx().h
        res = []
        for i in range(3):
            # the workspace is not initialised by the caller: NaN bytes in one run, another pattern in the next
            ws = torch.full((nws,), 0xFF if i != 1 else 0x5A, dtype=torch.uint8, device="cuda")
            outs = {k: _out(kt, n) for k, n in sizes.items()}
            if i < 2:
                _launch(lib, h, shape, ins, outs, ws, nws)
            else:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    _launch(lib, h, shape, ins, outs, ws, nws)
                graph.replay()
            kt.sync()
            res.append({k: _get(b) for k, b in outs.items()})
        for k, v in res[0].items():
            assert np.isfinite(v).all(), "%s: elements not written" % k
            assert np.array_equal(bits(res[0])[k], bits(res[1])[k]), "%s: repeat launch differs" % k
            assert np.array_equal(bits(res[0])[k], bits(res[2])[k]), "%s: graph replay differs" % k
        runs[dt] = res[0]
    for b in ins.values():
        _get(b)
    for k in sizes:                                                   # one f32 variant serves both context dtypes
        assert np.array_equal(bits(runs["f32"])[k], bits(runs["bf16"])[k]), k
    got = {k: runs["f32"][k].astype(np.float64).reshape(g64[k].shape) for k in g64}
    ratio = R.ratios(R.gaps(got, g64), a_gpu)
    _report("head_dec/" + "-".join(str(v) for v in shape), {"ratio_to_torch_f32_gap": ratio, "a": a_gpu})
    print(shape, "gap / a:", ratio, "a:", a_gpu)
    assert max(ratio.values()) <= R.ALLOW, (ratio, a_gpu)


def test_no_skip(models, kt):
    """skip == NULL with S == 0: the level without its skip term"""
    shape = (2, 2, 37, 37, 37, 128)
    level, B, M, inner, Lt, S = shape
    c, _, _ = R.refs(shape)
    lib, h = _lib(), models["f32"]._ensure_ctx().h
    ins = {k: _in(kt, c[k].numpy()) for k in ("x", "w", "b", "gamma", "beta")}
    nws = lib.athd_head_dec_workspace_bytes(level, B, M, inner, Lt)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")
    outs = {k: _out(kt, n) for k, n in _sizes(shape).items() if k in ("y", "stats")}
    par = [ins[k].ptr for k in ("w", "b", "gamma", "beta")]
    rc = lib.athd_head_dec_level(h, level, ins["x"].ptr, *par, None, B, M, inner, 0, Lt, outs["y"].ptr,
                                 outs["stats"].ptr, ws.data_ptr(), nws, _stream())
    assert rc == 0, lib.athd_last_error(h)
    kt.sync()
    dec = R._decoder(torch.float64, "cpu")
    R.autograd(c, torch.float64)                                      # loads the case's parameters into the level
    with torch.no_grad():
        want = R.torch_level(dec, level, c["x"], torch.zeros_like(c["skip"]), Lt).numpy()
    got = _get(outs["y"]).astype(np.float64).reshape(want.shape)
    assert R.gap(got, want) <= R.ALLOW * _gpu_gap(shape)["y"]


# ---------------------------------------------------------------------------------------------------- error paths
def test_argument_errors(models, kt):
    from athd import native
    lib, m = _lib(), models["f32"]
    h, s = m._ensure_ctx().h, _stream()
    L, B, M, I, Lt = 0, 1, 2, 3, 9
    buf = torch.zeros(384 * 192 * 8 + 16, dtype=torch.float32, device="cuda")
    nws = lib.athd_head_dec_workspace_bytes(L, B, M, I, Lt)
    assert nws > 0
    ws = torch.zeros(nws + 16, dtype=torch.uint8, device="cuda")
    p, w = buf.data_ptr(), ws.data_ptr()

    def fwd(h_=h, level=L, B_=B, M_=M, I_=I, Lt_=Lt, x=p, wt=p, gamma=p, skip=p, S=2, y=p, stats=p, w_=w, n_=nws):
        return lib.athd_head_dec_level(h_, level, x, wt, p, gamma, p, skip, B_, M_, I_, S, Lt_, y, stats, w_, n_, s)

    def bwd(h_=h, level=L, B_=B, M_=M, I_=I, Lt_=Lt, gy=p, wt=p, gamma=p, gx=p, gw=p, ggamma=p, w_=w, n_=nws):
        return lib.athd_head_dec_level_backward(h_, level, gy, p, wt, p, gamma, p, p, B_, M_, I_, Lt_, gx, gw, p, ggamma,
                                                p, w_, n_, s)

    # null pointers; the GroupNorm tensors are required on levels 0..2 only (test_kernels runs level 3 without them)
    for kw in (dict(x=None), dict(wt=None), dict(y=None), dict(gamma=None), dict(stats=None)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(gy=None), dict(wt=None), dict(gx=None), dict(gw=None), dict(gamma=None), dict(ggamma=None)):
        assert bwd(**kw) == EINVAL, kw
    assert b"null" in lib.athd_last_error(h)
    # the level and the shape (refused on the arguments alone: no tensor of that size exists here)
    for kw in (dict(level=-1), dict(level=4), dict(B_=0), dict(B_=65536), dict(M_=0), dict(M_=(1 << 20) + 1),
               dict(I_=0), dict(I_=4097), dict(Lt_=0), dict(Lt_=(1 << 22) + 1), dict(M_=1 << 20, I_=128),
               dict(I_=4096, Lt_=1 << 20)):
        a = dict(level=L, B_=B, M_=M, I_=I, Lt_=Lt)
        a.update(kw)
        assert lib.athd_head_dec_workspace_bytes(a["level"], a["B_"], a["M_"], a["I_"], a["Lt_"]) == 0, kw
        assert fwd(**kw) == EINVAL and bwd(**kw) == EINVAL, kw
    # 2048 frames: the time decoder's last level and the frequency decoder's widest
    assert lib.athd_head_dec_workspace_bytes(3, 1, 524288, 1, 2097152) > 0
    assert lib.athd_head_dec_workspace_bytes(1, 1, 2048, 2048, 2048) > 0
    # a skip without its length and a length without a skip
    assert fwd(skip=None, S=2) == EINVAL and fwd(S=0) == EINVAL and fwd(S=-1) == EINVAL
    # a misaligned weight, weight gradient or workspace
    assert fwd(wt=p + 4) == EINVAL and bwd(wt=p + 4) == EINVAL and bwd(gw=p + 4) == EINVAL
    assert fwd(w_=w + 4) == EINVAL and bwd(w_=w + 4) == EINVAL
    # a short or missing workspace, in both directions
    assert fwd(n_=nws - 1) == EWORKSPACE and fwd(w_=None) == EWORKSPACE
    assert bwd(n_=nws - 1) == EWORKSPACE and bwd(w_=None) == EWORKSPACE
    # the order: the state before the arguments, the arguments before the workspace
    assert fwd(x=None, n_=0) == EINVAL and bwd(level=7, n_=0) == EINVAL and fwd(wt=p + 4, n_=0) == EINVAL
    fresh = native.Context(0, native.F32)
    assert fwd(h_=fresh.h) == ESTATE and bwd(h_=fresh.h) == ESTATE
    assert fwd(h_=fresh.h, x=None, n_=0) == ESTATE and bwd(h_=fresh.h, level=9) == ESTATE
    fresh.close()
    kt.sync()
    assert not bool(buf.any()) and not bool(ws.any())                     # nothing was written by the refused calls


def test_native_decoders_refuses_what_it_does_not_cover(models):
    from athd.head import HeadTrainer, TrainableHead
    m = models["f32"]
    f = m.encode(torch.zeros(1, 2, 4096, device="cuda"))
    text = torch.zeros(1, 512)
    with pytest.raises(RuntimeError, match="native_decoders.*bind"):
        TrainableHead(native_decoders=True).cuda()(f, text)               # an unbound head
    with pytest.raises(RuntimeError, match="native_decoders.*float32"):
        TrainableHead(native_decoders=True).bind(m).double().cuda()(f, text)
    with pytest.raises(RuntimeError, match="native_decoders.*float32"):
        TrainableHead(native_decoders=True).bind(m)(f, text)              # a CPU head
    with pytest.raises(RuntimeError, match="native_decoders.*skips_t\\[1\\]"):
        skips_t = [t.double() if i == 1 else t for i, t in enumerate(f.skips_t)]
        TrainableHead(native_decoders=True).bind(m).cuda()(f._replace(skips_t=skips_t), text)
    # the option is off by default and composes with the other two, in any combination
    assert not TrainableHead().native_decoders and not HeadTrainer(m).head.native_decoders
    for cond in (False, True):
        for out in (False, True):
            t = HeadTrainer(m, native_decoders=True, native_cond=cond, native_output=out)
            assert (t.head.native_decoders, t.head.native_cond, t.head.native_output) == (True, cond, out)
            with torch.no_grad():
                y = t.head(f, text.cuda())
            assert y.shape == (1, 2, 4096) and bool(torch.isfinite(y).all())


# ---------------------------------------------------------------------------------------------------- end to end
def _wav(T):
    from athd.synth import synthetic_batch
    return torch.as_tensor(synthetic_batch(2, T, seed0=107))              # T = 4096: CASE_SHORT's mixture


@functools.lru_cache(maxsize=None)
def _target(T):
    from athd.synth import synthetic_batch
    return 0.5 * torch.as_tensor(synthetic_batch(2, T, seed0=211))


_oracle = {}


def _oracle_grads(m, oracle_model, state_dict, text_table, prompts, T):
    """the oracle's float64 and float32 gradients on the features of the length-T mixture, once for both options"""
    if T not in _oracle:
        from train_refs import LOSSES, total64
        feats = m.encode(_wav(T).cuda())
        text = _rows(text_table, prompts)
        w1, w2 = LOSSES["combined"]
        loss_fn = lambda out: total64(out, _target(T), "combined", w1, w2)
        g64, _ = H.oracle_grads(oracle_model, state_dict, H.decode_inputs(oracle_model, feats), text, T, loss_fn)
        g32, _ = H.oracle_grads(oracle_model, state_dict, H.decode_inputs(oracle_model, feats, torch.float32), text, T,
                                loss_fn, torch.float32)
        _oracle[T] = (g64, g32)
    return _oracle[T]


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("opt", OPTIONS, ids=OPT_IDS)
def test_gradients_against_float64(models, oracle_model, state_dict, text_table, opt, T):
    from athd.head import HeadTrainer
    from athd.loss import combined_loss
    prompts = ["bass", "vocals"]
    m = models["f32"]
    trainer = HeadTrainer(m, **opt)
    assert trainer.head.native_decoders and trainer.head.native_cond == bool(opt.get("native_cond"))
    trainer.train()
    combined_loss(trainer(_wav(T).cuda(), prompts), _target(T).cuda())[0].backward()
    params = dict(trainer.head.named_parameters())
    assert len(params) == 50
    missing = [k for k, p in params.items() if p.grad is None]
    assert not missing, missing
    got = {k: p.grad.detach().cpu().double() for k, p in params.items()}
    g64, g32 = _oracle_grads(m, oracle_model, state_dict, text_table, prompts, T)
    largest = max(float(g.abs().max()) for g in g64.values())
    dead_bound = 0.0 if opt.get("native_cond") else 1e-9 * largest      # (torch's query side leaves rounding noise)
    worst = {}
    for k, w in g64.items():
        if k in H.DEAD:
            assert float(got[k].abs().max()) <= dead_bound, k
            continue
        mx = float(w.abs().max())
        a = float((g32[k].double() - w).abs().max()) / mx
        worst[k] = float((got[k] - w).abs().max()) / mx / a
    for k in ("text_attn.attn.in_proj_weight", "text_attn.attn.in_proj_bias"):
        assert float(got[k][:768].abs().max()) <= dead_bound, k
    top = max(worst, key=worst.get)
    _report("head_grad_native_%s_T%d_f32_vs_f64" % ("_".join(sorted(opt)), T),
            {"worst_ratio_to_oracle_f32_gap": worst[top], "tensor": top})
    print(opt, T, "worst gap / oracle f32 gap:", top, worst[top])
    bad = {k: v for k, v in worst.items() if v > 4.0}
    assert not bad, bad


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("opt", OPTIONS, ids=OPT_IDS)
def test_output_against_torch_head(models, text_table, opt, T):
    from athd.head import TrainableHead
    m = models["f32"]
    wav = _wav(T).cuda()
    text = _rows(text_table, ["bass", "vocals"])
    head = TrainableHead.from_model(m).cuda().eval()
    feats = m.encode(wav)
    with torch.no_grad():
        want = head(feats, text)
        _, _, xdw, xtdw = head.branches(feats, text)
        head.native_decoders = True
        head.native_cond, head.native_output = bool(opt.get("native_cond")), bool(opt.get("native_output"))
        got = head.bind(m)(feats, text)
        _, _, xdg, xtdg = head.branches(feats, text)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert xdg.shape == xdw.shape and xtdg.shape == xtdw.shape
    n = lambda t: t.cpu().numpy()
    s = {"out": H.sdr_db(n(want), n(got)), "xd": H.sdr_db(n(xdw), n(xdg)), "xtd": H.sdr_db(n(xtdw), n(xtdg))}
    _report("head_native_%s_T%d_vs_torch_head" % ("_".join(sorted(opt)), T), s)
    print(opt, T, s)
    assert min(s.values()) >= F32_SDR_DB, s


_ref_epoch = {}


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("opt", OPTIONS, ids=OPT_IDS)
def test_train_epoch_matches_float64_loop(state_dict, text_table, oracle_model, opt, T):
    from athd.head import HeadTrainer, TrainableHead
    from athd.synth import synthetic_batch
    from athd.train import train_epoch
    from train_refs import train_epoch_ref
    B = 2
    prompts = [["bass", "vocals"], ["drums", "other"], ["vocals", "drums"]]
    batches = [{"mixture": torch.as_tensor(synthetic_batch(B, T, seed0=300 + i)),
                "target": 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=400 + i)), "prompt": prompts[i]}
               for i in range(3)]
    trainer = HeadTrainer(_new_model(state_dict, text_table, "f32"), **opt)
    got = train_epoch(trainer, batches, torch.optim.SGD(trainer.parameters(), lr=1e-2), None, "cuda", False, False,
                      None, None, 1.0, 0.9, 0.1, 0, 0)

    class Ref64(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.head = TrainableHead().double()
            self.head.load_state_dict(H.head_state(state_dict), strict=True)

        def forward(self, mixture, prompts):
            return self.head(H.oracle_features(oracle_model, mixture)[0], _rows(text_table, prompts).double())

    if T not in _ref_epoch:                                               # the float64 CPU loop, once for both options
        ref = Ref64()
        _ref_epoch[T] = train_epoch_ref(ref, batches, torch.optim.SGD(ref.parameters(), lr=1e-2), "combined", 0.9, 0.1,
                                        1.0)
    want = _ref_epoch[T]
    _report("head_train_epoch_native_%s_T%d" % ("_".join(sorted(opt)), T), {"got": got, "want": want})
    for k in ("loss", "sdr", "sisdr"):
        assert abs(got[k] - want[k]) <= 1e-3, (k, got[k], want[k])


def test_autocast_step(models):
    from athd.head import HeadTrainer
    from athd.loss import combined_loss
    T = 5000
    trainer = HeadTrainer(models["f32"], native_decoders=True)
    trainer.train()
    with torch.autocast("cuda"):
        feats = trainer.model.encode(_wav(T).cuda())
        _, _, xd, xtd = trainer.head.branches(feats, trainer.model.embedder.rows(["bass", "vocals"], 2))
        assert xd.shape[1:] == (2, 5, 5) and xtd.shape[1:] == (2, T)
        xdec, _ = trainer.head._native_decoder_stage(feats, feats.x_enc, feats.xt_enc)
        assert xdec.dtype == torch.float32                                # the stage computes and returns float32
        loss = combined_loss(trainer(_wav(T).cuda(), ["bass", "vocals"]), _target(T).cuda())[0]
    loss.backward()
    for k, p in trainer.head.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
    assert bool(trainer.head.freq_decoder.layers[1][0].weight.grad.any())
    assert bool(trainer.head.time_decoder.layers[3][0].weight.grad.any())
