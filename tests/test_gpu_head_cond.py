"""Head training's native text-conditioning stage on the GPU (include/athd.h `athd_head_cond`, `athd_head_cond_backward`;
athd/head.py `NativeCondStage`, `TrainableHead(native_cond=True)`).

Kernel level, on the shapes of `head_cond_refs.CASES` with guard bands round every buffer and NaN in every output: both
directions overwrite every element, are bit-equal run to run and under graph replay, bit-equal between a float32 and a
bf16 context, and the output, the six parameter gradients and the gradient of the attention vector each lie within
ALLOW = 4 times `a` of the float64 reference, `a` being the gap of torch's own float32 `_TextAttention.rows` on the same
GPU to that reference (tests/test_head_cond_refs.py shows that a float32 evaluation reaches that and that planted
defects do not).

End to end at the smallest shapes of tests/test_gpu_head_output.py, with `HeadTrainer(model, native_cond=True)` and with
`native_cond=True, native_output=True`: every one of the 50 tensors has a gradient, the live ones within 4 x the oracle's
f32-against-f64 gap, the dead ones exactly zero; the output against the torch head at F32_SDR_DB = 110 dB; three
`train_epoch` steps within 1e-3 dB of the float64 CPU loop; one autocast step with finite float32 gradients.
"""
import functools

import numpy as np
import pytest
import torch

import head_cond_refs as R
import head_refs as H
from test_gpu_head_output import _new_model, _rows, _wav, CASE_SHORT
from test_gpu_parity import F32_SDR_DB, _report

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
IDS = ["%d-%d" % c for c in R.CASES]
OPTIONS = [dict(native_cond=True), dict(native_cond=True, native_output=True)]
OPT_IDS = ["cond", "cond+output"]
C = R.C
GRADS = ["w0", "b0", "w2", "b2", "gamma", "beta", "a"]          # athd_head_cond_backward's outputs, in its order


@pytest.fixture(scope="module")
def models(state_dict, text_table):
    return {dt: _new_model(state_dict, text_table, dt) for dt in DTYPES}


@pytest.fixture(scope="module")
def kt():
    import ktest
    return ktest


def _lib():
    from athd import native
    return native.lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _in(kt, a):
    return kt.Buf(np.asarray(a, dtype=np.float32), "f32", 4096)


def _out(kt, n):
    return kt.Buf(np.full(n, np.nan, dtype=np.float32), "f32", 4096, output=True)


def _get(buf):
    raw, bands = buf.host()
    assert bands, "guard band overwritten"
    return raw


@functools.lru_cache(maxsize=None)
def _gpu_gap(shape):
    """torch's float32 `torch_stage` on this GPU against the float64 reference, per tensor"""
    c, g64, _ = R.refs(shape)
    return R.gaps(R.autograd(c, torch.float32, "cuda"), g64)


def _sizes(B, N):
    return dict(y=B * C * N, w0=C * C, b0=C, w2=C * C, b2=C, gamma=C, beta=C, a=B * C)


def _launch(lib, h, ins, outs, B, N, ws, nws):
    s = _stream()
    w = [ins[k].ptr for k in ("w0", "b0", "w2", "b2", "gamma")]
    rc = lib.athd_head_cond(h, ins["x"].ptr, ins["a"].ptr, *w, ins["beta"].ptr, B, N, outs["y"].ptr, None, 0, s)
    assert rc == 0, lib.athd_last_error(h)
    rc = lib.athd_head_cond_backward(h, ins["gy"].ptr, ins["x"].ptr, ins["a"].ptr, *w, B, N,
                                     *[outs[k].ptr for k in GRADS], ws.data_ptr(), nws, s)
    assert rc == 0, lib.athd_last_error(h)


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_kernels(models, kt, shape):
    B, N = shape
    c, g64, _ = R.refs(shape)
    a_gpu = _gpu_gap(shape)
    lib = _lib()
    w = R.weights(c, np.float32)
    ins = {k: _in(kt, v) for k, v in w.items()}
    ins.update(x=_in(kt, c["x"].numpy()), gy=_in(kt, c["gy"].numpy()), a=_in(kt, R.attn_vector(c, np.float32)))
    nws = lib.athd_head_cond_workspace_bytes(B, N)
    assert nws > 0
    sizes = _sizes(B, N)
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
                _launch(lib, h, ins, outs, B, N, ws, nws)
            else:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    _launch(lib, h, ins, outs, B, N, ws, nws)
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
    got = {k: runs["f32"][k].astype(np.float64).reshape(g64[k].shape) for k in sizes}
    g = R.gaps(got, g64)
    ratio = {k: (g[k] / a_gpu[k] if a_gpu[k] > 0 else (0.0 if g[k] == 0 else float("inf"))) for k in R.NAMES}
    _report("head_cond/%d-%d" % shape, {"ratio_to_torch_f32_gap": ratio, "a": a_gpu})
    print(shape, "gap / a:", ratio, "a:", a_gpu)
    assert max(ratio.values()) <= R.ALLOW, (ratio, a_gpu)


# ---------------------------------------------------------------------------------------------------- error paths
def test_argument_errors(models, kt):
    from athd import native
    lib, m = _lib(), models["f32"]
    h, s = m._ensure_ctx().h, _stream()
    B, N = 1, 8
    buf = torch.zeros(C * C, dtype=torch.float32, device="cuda")
    nws = lib.athd_head_cond_workspace_bytes(B, N)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    p, w = buf.data_ptr(), ws.data_ptr()
    fwd = lambda h_, B_, N_, x=p, y=p: lib.athd_head_cond(h_, x, p, p, p, p, p, p, p, B_, N_, y, None, 0, s)
    bwd = lambda h_, B_, N_, gy=p, ga=p, w_=w, n_=nws: lib.athd_head_cond_backward(h_, gy, p, p, p, p, p, p, p, B_, N_,
                                                                                  p, p, p, p, p, p, ga, w_, n_, s)
    # null pointers
    assert fwd(h, B, N, x=None) == -1 and fwd(h, B, N, y=None) == -1
    assert bwd(h, B, N, gy=None) == -1 and bwd(h, B, N, ga=None) == -1
    assert b"null" in lib.athd_last_error(h)
    # B = 0, N = 0, N over the limit (refused on the arguments alone: no tensor of that size exists here)
    limit = 1 << 20
    for B_, N_ in [(0, N), (65536, N), (B, 0), (B, limit + 1)]:
        assert lib.athd_head_cond_workspace_bytes(B_, N_) == 0
        assert fwd(h, B_, N_) == -1 and bwd(h, B_, N_) == -1, (B_, N_)
    assert lib.athd_head_cond_workspace_bytes(8, 8 * 2048) > 0           # 2048 frames of the frequency branch
    # a short workspace (the forward needs none)
    assert bwd(h, B, N, n_=nws - 1) == -5 and bwd(h, B, N, w_=None) == -5
    # an unfinalised context
    fresh = native.Context(0, native.F32)
    assert fwd(fresh.h, B, N) == -3 and bwd(fresh.h, B, N) == -3
    fresh.close()
    kt.sync()
    assert not bool(buf.any()) and not bool(ws.any())                     # nothing was written by the refused calls


def test_native_cond_refuses_what_it_does_not_cover(models):
    from athd.head import TrainableHead
    m = models["f32"]
    f = m.encode(torch.zeros(1, 2, 4096, device="cuda"))
    text = torch.zeros(1, 512)
    with pytest.raises(RuntimeError, match="bind"):
        TrainableHead(native_cond=True).cuda()(f, text)                   # an unbound head
    with pytest.raises(RuntimeError, match="float32"):
        TrainableHead(native_cond=True).bind(m).double().cuda()(f, text)
    with pytest.raises(RuntimeError, match="float32"):
        TrainableHead(native_cond=True).bind(m)(f, text)                  # a CPU head
    with pytest.raises(RuntimeError, match="x_enc"):
        TrainableHead(native_cond=True).bind(m).cuda()(f._replace(x_enc=f.x_enc.double()), text)


# ---------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _target():
    from athd.synth import synthetic_batch
    B, T, _ = CASE_SHORT
    return 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=211))


_oracle = {}


def _oracle_grads(m, oracle_model, state_dict, text_table, prompts):
    """the oracle's float64 and float32 gradients on the features of CASE_SHORT, computed once for both options"""
    if "g" not in _oracle:
        from train_refs import LOSSES, total64
        _, T, _ = CASE_SHORT
        feats = m.encode(_wav().cuda())
        text = _rows(text_table, prompts)
        w1, w2 = LOSSES["combined"]
        loss_fn = lambda out: total64(out, _target(), "combined", w1, w2)
        g64, _ = H.oracle_grads(oracle_model, state_dict, H.decode_inputs(oracle_model, feats), text, T, loss_fn)
        g32, _ = H.oracle_grads(oracle_model, state_dict, H.decode_inputs(oracle_model, feats, torch.float32), text, T,
                                loss_fn, torch.float32)
        _oracle["g"] = (g64, g32)
    return _oracle["g"]


@pytest.mark.parametrize("opt", OPTIONS, ids=OPT_IDS)
def test_gradients_against_float64(models, oracle_model, state_dict, text_table, opt):
    from athd.head import HeadTrainer
    from athd.loss import combined_loss
    prompts = ["bass", "vocals"]
    m = models["f32"]
    trainer = HeadTrainer(m, **opt)
    assert trainer.head.native_cond and trainer.head.native_output == bool(opt.get("native_output"))
    trainer.train()
    combined_loss(trainer(_wav().cuda(), prompts), _target().cuda())[0].backward()
    params = dict(trainer.head.named_parameters())
    assert len(params) == 50
    missing = [k for k, p in params.items() if p.grad is None]
    assert not missing, missing
    got = {k: p.grad.detach().cpu().double() for k, p in params.items()}
    g64, g32 = _oracle_grads(m, oracle_model, state_dict, text_table, prompts)
    worst = {}
    for k, w in g64.items():
        if k in H.DEAD:
            assert not bool(got[k].any()), k                              # exactly zero
            continue
        mx = float(w.abs().max())
        a = float((g32[k].double() - w).abs().max()) / mx
        worst[k] = float((got[k] - w).abs().max()) / mx / a
    for k in ("text_attn.attn.in_proj_weight", "text_attn.attn.in_proj_bias"):
        assert not bool(got[k][:768].any()), k
    top = max(worst, key=worst.get)
    _report("head_grad_native_%s_f32_vs_f64" % "_".join(sorted(opt)), {"worst_ratio_to_oracle_f32_gap": worst[top],
                                                                       "tensor": top})
    print(opt, "worst gap / oracle f32 gap:", top, worst[top])
    bad = {k: v for k, v in worst.items() if v > 4.0}
    assert not bad, bad


@pytest.mark.parametrize("opt", OPTIONS, ids=OPT_IDS)
def test_output_against_torch_head(models, text_table, opt):
    from athd.head import TrainableHead
    m = models["f32"]
    wav = _wav().cuda()
    text = _rows(text_table, ["bass", "vocals"])
    head = TrainableHead.from_model(m).cuda().eval()
    feats = m.encode(wav)
    with torch.no_grad():
        want = head(feats, text)
        xw, xtw, _, _ = head.branches(feats, text)
        head.native_cond, head.native_output = True, bool(opt.get("native_output"))
        got = head.bind(m)(feats, text)
        xg, xtg, _, _ = head.branches(feats, text)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert xg.shape == xw.shape and xtg.shape == xtw.shape and xg.is_contiguous() and xtg.is_contiguous()
    s = {"out": H.sdr_db(want.cpu().numpy(), got.cpu().numpy()), "x_cond": H.sdr_db(xw.cpu().numpy(), xg.cpu().numpy()),
         "xt_cond": H.sdr_db(xtw.cpu().numpy(), xtg.cpu().numpy())}
    _report("head_native_%s_vs_torch_head" % "_".join(sorted(opt)), s)
    print(opt, s)
    assert min(s.values()) >= F32_SDR_DB, s


_ref_epoch = {}


@pytest.mark.parametrize("opt", OPTIONS, ids=OPT_IDS)
def test_train_epoch_matches_float64_loop(state_dict, text_table, oracle_model, opt):
    from athd.head import HeadTrainer, TrainableHead
    from athd.synth import synthetic_batch
    from athd.train import train_epoch
    from train_refs import train_epoch_ref
    B, T = 2, 4096
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

    if "want" not in _ref_epoch:                                          # the float64 CPU loop, once for both options
        ref = Ref64()
        _ref_epoch["want"] = train_epoch_ref(ref, batches, torch.optim.SGD(ref.parameters(), lr=1e-2), "combined", 0.9,
                                             0.1, 1.0)
    want = _ref_epoch["want"]
    _report("head_train_epoch_native_%s" % "_".join(sorted(opt)), {"got": got, "want": want})
    for k in ("loss", "sdr", "sisdr"):
        assert abs(got[k] - want[k]) <= 1e-3, (k, got[k], want[k])


def test_autocast_step(models):
    from athd.head import HeadTrainer
    from athd.loss import combined_loss
    trainer = HeadTrainer(models["f32"], native_cond=True)
    trainer.train()
    with torch.autocast("cuda"):
        feats = trainer.model.encode(_wav().cuda())
        x_cond, xt_cond, _, _ = trainer.head.branches(feats, trainer.model.embedder.rows(["bass", "vocals"], 2))
        assert x_cond.dtype == torch.float32 and xt_cond.dtype == torch.float32
        loss = combined_loss(trainer(_wav().cuda(), ["bass", "vocals"]), _target().cuda())[0]
    loss.backward()
    for k, p in trainer.head.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
    assert bool(trainer.head.text_attn.out_mlp[0].weight.grad.any())
