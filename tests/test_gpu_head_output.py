"""Head training's native output stage on the GPU (include/athd.h `athd_pack_spectrum`, `athd_head_output`,
`athd_head_output_backward`; athd/head.py `NativeOutputStage`, `TrainableHead(native_output=True)`).

Kernel level, on the shapes of `head_output_refs.CASES` with guard bands round every buffer and sentinels in every output:
the pack is a bit-exact permute; the forward is bit-equal to the inference path's launch (`kt_istft_ola`, P = 1) on the
same buffers and the context's own tables, in both dtype modes; the backward overwrites every element, is bit-equal run
to run and under graph replay in both modes, and each item lies within ALLOW = 4 times `a` of the float64 closed form,
`a` being torch's own float32-against-float64 autograd gap on the case (tests/test_head_output_refs.py shows that a
float32 evaluation reaches that and that planted defects do not).

End to end, with `HeadTrainer(model, native_output=True)`: the protocol of tests/test_gpu_head.py's
`test_gradients_against_float64` (every live head tensor within 4 x the oracle's f32-against-f64 gap, the dead ones
zero), the output against the torch stage (float32 context: F32_SDR_DB = 110 dB; bf16 context: BF16_STAGE_DB, 10 dB under
the measured value), and three `train_epoch` steps within 1e-3 dB of the float64 CPU loop.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import head_output_refs as R
import head_refs as H
import spectral_cases as sc
from test_gpu_parity import F32_SDR_DB, _report

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
IDS = ["%d-%d-%d" % c for c in R.CASES]
# The bf16 context's forward (float FFT with running-product twiddles, v_exp / v_rcp in the mask) against the float64
# torch stage on the same float32 inputs, whole-output SDR.  Measured on MI355X on the features of CASE_SHORT:
# 131.5 dB (the float32 context: 136.8 dB; against the float32 torch stage 131.0 / 135.7 dB); the gate sits 10 dB under
# the measured value.
BF16_STAGE_MEASURED_DB = 131.5
BF16_STAGE_DB = BF16_STAGE_MEASURED_DB - 10.0


def _new_model(state_dict, text_table, dt):
    from athd.model import AudioTextHTDemucs
    from athd.weights import STEMS
    m = AudioTextHTDemucs(dtype=dt, text_table={s: text_table[i] for i, s in enumerate(STEMS)})
    m.load_state_dict(state_dict)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def models(state_dict, text_table):
    return {dt: _new_model(state_dict, text_table, dt) for dt in DTYPES}


@pytest.fixture(scope="module")
def kt():
    import ktest
    ktest.lib.kt_ctx_tables.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return ktest


def _lib():
    from athd import native
    return native.lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _in(kt, a):
    return kt.Buf(np.asarray(a, dtype=np.float32), "f32", 4096)


def _out(kt, n):
    return kt.Buf(np.full(n, kt.F32_SENTINEL, dtype=np.float32), "f32", 4096, output=True)


def _get(buf):
    raw, bands = buf.host()
    assert bands, "guard band overwritten"
    return raw


@functools.lru_cache(maxsize=None)
def _kernel_case(shape):
    """the kernel-layout arrays of a shape: fo (B, Ts, Ts, 2), spec (B, Ts, 2048, 4), xt2 (B, T, 2), tnorm (B, 2), g"""
    Ts, T, B = shape
    c = sc.istft_case(Ts, T, B, 1)
    return c, R.refs(shape)[0]["g"].numpy().astype(np.float32)


@functools.lru_cache(maxsize=None)
def _closed64(shape):
    return R.closed_form(R.refs(shape)[0])[0]


# ---------------------------------------------------------------------------------------------------- the pack
@pytest.mark.parametrize("B,Ts", [(2, 1), (2, 4), (1, 33)])
def test_pack_spectrum_exact(models, kt, B, Ts):
    z = np.random.default_rng(B * 100 + Ts).standard_normal((B, 2, 2048, Ts, 2)).astype(np.float32)
    src, dst = _in(kt, z), _out(kt, z.size)
    assert _lib().athd_pack_spectrum(models["f32"]._ensure_ctx().h, src.ptr, B, Ts, dst.ptr, _stream()) == 0
    kt.sync()
    got = _get(dst).reshape(B, Ts, 2048, 4)
    _get(src)
    want = np.ascontiguousarray(z.transpose(0, 3, 2, 1, 4)).reshape(B, Ts, 2048, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_forward_bit_equal_to_inference_kernel(models, kt, shape, dt):
    Ts, T, B = shape
    c, _ = _kernel_case(shape)
    lib, h = _lib(), models[dt]._ensure_ctx().h
    tabs = (ctypes.c_void_p * 4)()
    assert kt.lib.kt_ctx_tables(h, tabs) == 0
    nws = lib.athd_head_output_workspace_bytes(B, T)
    assert nws == kt.lib.kt_istft_part_floats(B, Ts) * 4
    bfo, bsp, bx, bt = (_in(kt, c[k]) for k in ("fo", "spec", "xt2", "tnorm"))
    o1, o2, p1, p2 = _out(kt, B * 2 * T), _out(kt, B * 2 * T), _out(kt, nws // 4), _out(kt, nws // 4)
    assert lib.athd_head_output(h, bfo.ptr, bsp.ptr, bx.ptr, bt.ptr, B, T, o1.ptr, p1.ptr, nws, _stream()) == 0
    kt.sync()
    d = kt.fill(kt.KtIstft, fo=bfo.ptr, NI=B, Tspec=Ts, P=1, T=T, spec=bsp.ptr, tw=tabs[0],
                tw64=tabs[1] if dt == "f32" else None, win=tabs[2], win2=tabs[3], xt2=bx.ptr, tnorm=bt.ptr, out=o2.ptr,
                part=p2.ptr)
    assert kt.lib.kt_istft_ola(ctypes.byref(d), None) == 0
    kt.sync()
    a, b = _get(o1), _get(o2)
    assert np.isfinite(a).all() and (a != np.float32(kt.F32_SENTINEL)).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(_get(p1).view(np.uint32), _get(p2).view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the backward
@pytest.mark.parametrize("shape", R.CASES, ids=IDS)
def test_backward_kernel(models, kt, shape):
    Ts, T, B = shape
    c, g = _kernel_case(shape)
    _, _, a = R.refs(shape)
    want = _closed64(shape)                                             # (B, 2, row, frame)
    lib = _lib()
    bg, bfo, bsp = _in(kt, g), _in(kt, c["fo"]), _in(kt, c["spec"])
    runs = {}
    for dt in DTYPES:
        h = models[dt]._ensure_ctx().h
        outs = []
        for _ in range(2):
            bo = _out(kt, B * Ts * Ts * 2)
            assert lib.athd_head_output_backward(h, bg.ptr, bfo.ptr, bsp.ptr, B, T, bo.ptr, _stream()) == 0
            kt.sync()
            outs.append(_get(bo))
        # graph replay on a sentinel-filled buffer
        bo = _out(kt, B * Ts * Ts * 2)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            rc = lib.athd_head_output_backward(h, bg.ptr, bfo.ptr, bsp.ptr, B, T, bo.ptr, _stream())
        assert rc == 0
        graph.replay()
        kt.sync()
        outs.append(_get(bo))
        assert np.isfinite(outs[0]).all() and (outs[0] != np.float32(kt.F32_SENTINEL)).all(), "elements not written"
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "repeat launch differs"
        assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32)), "graph replay differs"
        runs[dt] = outs[0]
    for b in (bg, bfo, bsp):
        _get(b)
    # one f32 variant serves both context dtypes
    assert np.array_equal(runs["f32"].view(np.uint32), runs["bf16"].view(np.uint32))
    got = runs["f32"].astype(np.float64).reshape(B, Ts, Ts, 2).transpose(0, 3, 2, 1)
    ratio = [gp / ai for gp, ai in zip(R.item_gap(got, want), a)]
    _report("head_output_backward/%d-%d-%d" % shape, {"worst_ratio_to_f32_autograd_gap": max(ratio), "a": a})
    print(shape, "gap / a:", ratio, "a:", a)
    assert max(ratio) <= R.ALLOW, (ratio, a)


# ---------------------------------------------------------------------------------------------------- the Function
def _stage_inputs(model, shape):
    """(head bound to the model, xd, xtd leaves, spec, meant, stdt, g) on the GPU in float32"""
    from athd.head import TrainableHead
    c = R.refs(shape)[0]
    head = TrainableHead(native_output=True).bind(model)
    cu = lambda t: t.float().cuda()
    z = c["z"].to(torch.complex64).cuda().contiguous()
    return (head, cu(c["xd"]).requires_grad_(True), cu(c["xtd"]).requires_grad_(True), head.packed_spectrum(z),
            cu(c["meant"]), cu(c["stdt"]), cu(c["g"]))


def test_time_branch_gradient(models):
    from athd.head import NativeOutputStage
    shape = (3, 3072, 2)
    m = models["f32"]
    head, xd, xtd, spec, meant, stdt, g = _stage_inputs(m, shape)
    NativeOutputStage.apply(xd, xtd, spec, meant, stdt, m._ensure_ctx()).backward(g)
    assert torch.equal(xtd.grad, g * stdt)
    assert xd.grad.shape == xd.shape
    # a head that emits another length: the torch resize in front of the Function
    c, g64, _ = R.refs(shape)
    short = c["xtd"][..., :3000].contiguous()
    want = R.autograd(c, torch.float64, xtd=short)[1]
    a = R.item_gap(R.autograd(c, torch.float32, xtd=short)[1], want)
    xs = short.float().cuda().requires_grad_(True)
    xr = torch.nn.functional.interpolate(xs, size=3072, mode="linear", align_corners=False)
    NativeOutputStage.apply(xd.detach(), xr, spec, meant, stdt, m._ensure_ctx()).backward(g)
    ratio = [gp / ai for gp, ai in zip(R.item_gap(xs.grad.cpu().double().numpy(), want), a)]
    print("resized time branch, gap / a:", ratio)
    assert max(ratio) <= R.ALLOW, ratio


def test_native_output_refuses_what_it_does_not_cover(models):
    from athd.head import TrainableHead
    m = models["f32"]
    f = m.encode(torch.zeros(1, 2, 4096, device="cuda"))
    text = torch.zeros(1, 512)
    with pytest.raises(RuntimeError, match="bind"):
        TrainableHead(native_output=True).cuda()(f, text)
    with pytest.raises(RuntimeError, match="float32"):
        TrainableHead(native_output=True).bind(m).double().cuda()(f, text)
    with pytest.raises(RuntimeError, match="float32"):
        TrainableHead(native_output=True).bind(m)(f, text)               # a CPU head


# ---------------------------------------------------------------------------------------------------- error paths
def test_argument_errors(models, kt):
    from athd import native
    lib, m = _lib(), models["f32"]
    h, s = m._ensure_ctx().h, _stream()
    B, T, Ts = 1, 1000, 1
    buf = torch.zeros(max(B * Ts * 2048 * 4, B * 2 * T), dtype=torch.float32, device="cuda")
    nws = lib.athd_head_output_workspace_bytes(B, T)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    p, w = buf.data_ptr(), ws.data_ptr()
    # more than 2048 frames: refused on the arguments alone (no tensor of that size exists here)
    long_T = 2049 * 1024
    assert lib.athd_head_output_workspace_bytes(1, long_T) == 0
    assert lib.athd_head_output_backward(h, p, p, p, 1, long_T, p, s) == -1
    assert b"2048" in lib.athd_last_error(h)
    assert lib.athd_head_output(h, p, p, p, p, 1, long_T, p, w, nws, s) == -1
    assert lib.athd_pack_spectrum(h, p, 1, 2049, p, s) == -1
    # null pointers
    assert lib.athd_head_output_backward(h, p, None, p, B, T, p, s) == -1
    assert lib.athd_head_output_backward(h, p, p, p, B, T, None, s) == -1
    assert lib.athd_head_output(h, p, p, None, p, B, T, p, w, nws, s) == -1
    assert lib.athd_pack_spectrum(h, None, B, Ts, p, s) == -1
    assert lib.athd_head_output_backward(h, p, p, p, 0, T, p, s) == -1
    # a short workspace
    assert lib.athd_head_output(h, p, p, p, p, B, T, p, w, nws - 1, s) == -5
    assert lib.athd_head_output(h, p, p, p, p, B, T, p, None, nws, s) == -5
    # an unfinalised context
    fresh = native.Context(0, native.F32)
    assert lib.athd_pack_spectrum(fresh.h, p, B, Ts, p, s) == -3
    assert lib.athd_head_output(fresh.h, p, p, p, p, B, T, p, w, nws, s) == -3
    assert lib.athd_head_output_backward(fresh.h, p, p, p, B, T, p, s) == -3
    fresh.close()
    kt.sync()
    assert not bool(buf.any())                                            # nothing was written by the refused calls


# ---------------------------------------------------------------------------------------------------- end to end
CASE_SHORT = (2, 4096, 107)          # (B, T, seed0): tests/test_gpu_head.py CASES["short"]


def _wav():
    from athd.synth import synthetic_batch
    B, T, seed0 = CASE_SHORT
    return torch.as_tensor(synthetic_batch(B, T, seed0=seed0))


def _rows(text_table, prompts):
    from athd.weights import STEMS
    return torch.as_tensor(np.stack([text_table[STEMS.index(p)] for p in prompts]))


def test_gradients_against_float64_native_output(models, oracle_model, state_dict, text_table):
    from athd.head import HeadTrainer
    from athd.loss import combined_loss
    from athd.synth import synthetic_batch
    from train_refs import LOSSES, total64
    B, T, _ = CASE_SHORT
    mix = _wav().cuda()
    target = 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=211))
    prompts = ["bass", "vocals"]
    m = models["f32"]
    trainer = HeadTrainer(m, native_output=True)
    assert trainer.head.native_output
    trainer.train()
    combined_loss(trainer(mix, prompts), target.cuda())[0].backward()
    got = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().double()
           for k, p in trainer.head.named_parameters()}
    feats = m.encode(mix)
    text = _rows(text_table, prompts)
    w1, w2 = LOSSES["combined"]
    loss_fn = lambda out: total64(out, target, "combined", w1, w2)
    g64, _ = H.oracle_grads(oracle_model, state_dict, H.decode_inputs(oracle_model, feats), text, T, loss_fn)
    g32, _ = H.oracle_grads(oracle_model, state_dict, H.decode_inputs(oracle_model, feats, torch.float32), text, T,
                            loss_fn, torch.float32)
    largest = max(float(g.abs().max()) for g in g64.values())
    worst = {}
    for k, w in g64.items():
        if k in H.DEAD:
            assert float(got[k].abs().max()) <= 1e-9 * largest, k
            continue
        mx = float(w.abs().max())
        a = float((g32[k].double() - w).abs().max()) / mx
        worst[k] = float((got[k] - w).abs().max()) / mx / a
    for k in ("text_attn.attn.in_proj_weight", "text_attn.attn.in_proj_bias"):
        assert float(got[k][:768].abs().max()) <= 1e-9 * largest, k
    top = max(worst, key=worst.get)
    _report("head_grad_native_output_f32_vs_f64", {"worst_ratio_to_oracle_f32_gap": worst[top], "tensor": top})
    print("worst gap / oracle f32 gap:", top, worst[top])
    bad = {k: v for k, v in worst.items() if v > 4.0}
    assert not bad, bad


def test_output_against_torch_stage(models, text_table):
    from athd.head import TrainableHead
    B, T, _ = CASE_SHORT
    wav = _wav().cuda()
    text = _rows(text_table, ["bass", "vocals"])
    measured = {}
    for dt in DTYPES:
        m = models[dt]
        head = TrainableHead.from_model(m).cuda().eval()
        feats = m.encode(wav)
        with torch.no_grad():
            want = head(feats, text)
            head.native_output = True
            got = head.bind(m)(feats, text)
            _, _, xd, xtd = head.branches(feats, text)
        assert got.shape == want.shape and got.dtype == torch.float32
        s = H.sdr_db(want.cpu().numpy(), got.cpu().numpy())
        # the float64 torch stage on the same float32 inputs
        d = lambda t: t.detach().cpu().double()
        ref = R.torch_stage(d(xd), d(xtd), feats.z.cpu().to(torch.complex128), d(feats.meant), d(feats.stdt), T)
        s64 = H.sdr_db(ref.numpy(), got.cpu().numpy())
        measured[dt] = {"vs_torch_f32_stage_db": s, "vs_float64_stage_db": s64}
        print(dt, measured[dt])
        if dt == "f32":
            assert s >= F32_SDR_DB, s
        else:
            assert s64 >= BF16_STAGE_DB, s64
    _report("head_native_output_vs_torch_stage", measured)


def test_train_epoch_native_output_matches_float64_loop(state_dict, text_table, oracle_model):
    from athd.head import HeadTrainer, TrainableHead
    from athd.synth import synthetic_batch
    from athd.train import train_epoch
    from train_refs import train_epoch_ref
    B, T = 2, 4096
    prompts = [["bass", "vocals"], ["drums", "other"], ["vocals", "drums"]]
    batches = [{"mixture": torch.as_tensor(synthetic_batch(B, T, seed0=300 + i)),
                "target": 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=400 + i)), "prompt": prompts[i]}
               for i in range(3)]
    trainer = HeadTrainer(_new_model(state_dict, text_table, "f32"), native_output=True)
    got = train_epoch(trainer, batches, torch.optim.SGD(trainer.parameters(), lr=1e-2), None, "cuda", False, False,
                      None, None, 1.0, 0.9, 0.1, 0, 0)

    class Ref64(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.head = TrainableHead().double()
            self.head.load_state_dict(H.head_state(state_dict), strict=True)

        def forward(self, mixture, prompts):
            return self.head(H.oracle_features(oracle_model, mixture)[0], _rows(text_table, prompts).double())

    ref = Ref64()
    want = train_epoch_ref(ref, batches, torch.optim.SGD(ref.parameters(), lr=1e-2), "combined", 0.9, 0.1, 1.0)
    _report("head_train_epoch_native_output", {"got": got, "want": want})
    for k in ("loss", "sdr", "sisdr"):
        assert abs(got[k] - want[k]) <= 1e-3, (k, got[k], want[k])
