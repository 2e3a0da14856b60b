"""Head training on the native encoder, on the GPU: the export kernels alone, `AudioTextHTDemucs.encode` against the
oracle, `TrainableHead` against the native decoder, its gradients, the round trip into the inference path, the step
loop, determinism / graph capture, and the untouched forward.

Gates: exact equality for the export kernels (they copy); F32_STAGE_DB = 90 dB per exported tensor in f32 mode;
BF16_FEATURE_DB per exported tensor in bf16 mode (10 dB under the lowest measured, see below); F32_SDR_DB = 110 dB /
BF16_SDR_DB = 40 dB between the torch head and the native decoder on the same features; gradients within 4 x the
oracle's own f32-against-f64 gap per tensor; the step loop within 1e-3 (dB) of a float64 CPU loop.
"""
import functools

import numpy as np
import pytest
import torch

import head_refs as H
from test_gpu_parity import BF16_SDR_DB, F32_SDR_DB, F32_STAGE_DB, PHASE_COND_MIN, _phase_cond, _report

pytestmark = pytest.mark.gpu

# bf16 mode, per exported tensor against the f32 oracle.  Measured on MI355X (the parity report's "encode_bf16/*"):
# x_enc 47.9 / 48.2, xt_enc 47.8 / 47.7, skips 52.0-52.4 / 47.6 / 46.2 / 46.6-46.9, skips_t 48.5-49.1 / 47.1-47.3 /
# 45.8-46.0 / 44.8-45.0, z 129 dB (T = 4096 / 33297).  The lowest is skips_t[3] at T = 33297; the gate sits 10 dB under.
BF16_FEATURE_MEASURED_MIN_DB = 44.8
BF16_FEATURE_DB = BF16_FEATURE_MEASURED_MIN_DB - 10.0

CASES = {"short": (2, 4096, 107), "ragged": (1, 33297, 6), "mid": (1, 9999, 6)}     # (B, T, seed0)
NAMES = (["x_enc", "xt_enc"] + [f"skips[{i}]" for i in range(4)] + [f"skips_t[{i}]" for i in range(4)]
         + ["z", "meant", "stdt"])


def _flat(f):
    return [f.x_enc, f.xt_enc, *f.skips, *f.skips_t, f.z, f.meant, f.stdt]


def _wav(case):
    from athd.synth import synthetic_batch
    B, T, seed0 = CASES[case]
    return torch.as_tensor(synthetic_batch(B, T, seed0=seed0))


def _new_model(state_dict, text_table, dt):
    from athd.model import AudioTextHTDemucs
    from athd.weights import STEMS
    m = AudioTextHTDemucs(dtype=dt, text_table={s: text_table[i] for i, s in enumerate(STEMS)})
    m.load_state_dict(state_dict)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def models(state_dict, text_table):
    return {dt: _new_model(state_dict, text_table, dt) for dt in ("f32", "bf16")}


@pytest.fixture(scope="module")
def oracle_feats(oracle_model):
    @functools.lru_cache(maxsize=None)
    def get(case):
        return H.oracle_features(oracle_model, _wav(case), torch.float32)[0]
    return get


def _rows(text_table, prompts):
    from athd.weights import STEMS
    return torch.as_tensor(np.stack([text_table[STEMS.index(p)] for p in prompts]))


# ------------------------------------------------------------------------------------------ 5. the kernels alone
def test_ktest_struct_sizes():
    import ktest_head as KH
    for name, (c, py) in KH.sizes_match().items():
        assert c == py, name


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("C,Cs", [(4, 4), (48, 4), (96, 48), (384, 192), (384, 384)])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 8325])
def test_export_cf_exact(rows, C, Cs, bf16):
    import ktest_head as KH
    rng = np.random.default_rng(rows * 1000 + C + Cs)
    if bf16:
        x = rng.integers(0, 0x7F80, size=(2, rows, C)).astype(np.uint16)        # finite, non-negative bf16 patterns
        x |= (rng.integers(0, 2, size=x.shape).astype(np.uint16) << 15)
    else:
        x = rng.standard_normal((2, rows, C)).astype(np.float32)
    got, bands = KH.export_cf(x, Cs, bf16)
    assert bands
    assert np.array_equal(got.view(np.uint32), KH.export_cf_ref(x, Cs, bf16).view(np.uint32))


@pytest.mark.parametrize("B,Ts", [(2, 1), (2, 4), (1, 33)])
def test_export_spec_exact(B, Ts):
    import ktest_head as KH
    x = np.random.default_rng(B * 100 + Ts).standard_normal((B, Ts, 2048, 4)).astype(np.float32)
    got, bands = KH.export_spec(x)
    assert bands
    assert np.array_equal(got, KH.export_spec_ref(x))


# ------------------------------------------------------------------------------------------ 6. encode vs the oracle
def _encode_sdrs(model, case, oracle_feats):
    want = oracle_feats(case)
    got = model.encode(_wav(case).cuda())
    torch.cuda.synchronize()
    assert got.lengths == list(want.lengths) and got.lengths_t == list(want.lengths_t) and got.length == want.length
    out = {}
    for name, g, w in zip(NAMES, _flat(got), _flat(want)):
        assert g.is_contiguous() and g.shape == w.shape, name
        assert g.dtype == (torch.complex64 if name == "z" else torch.float32), name
        gc, wc = g.cpu(), w
        if name == "z":
            gc, wc = torch.view_as_real(gc), torch.view_as_real(wc.contiguous())
        assert bool(torch.isfinite(gc).all()), name
        out[name] = H.sdr_db(wc.numpy(), gc.numpy())
    return out


@pytest.mark.parametrize("case", ["short", "ragged"])
def test_encode_f32_against_oracle(models, oracle_feats, case):
    sdrs = _encode_sdrs(models["f32"], case, oracle_feats)
    _report(f"encode_f32/{case}", sdrs)
    print(case, {k: round(v, 1) for k, v in sdrs.items()})
    bad = {k: v for k, v in sdrs.items() if v < F32_STAGE_DB}
    assert not bad, bad


@pytest.mark.parametrize("case", ["short", "ragged"])
def test_encode_bf16_against_oracle(models, oracle_feats, case):
    sdrs = _encode_sdrs(models["bf16"], case, oracle_feats)
    _report(f"encode_bf16/{case}", sdrs)
    print(case, {k: round(v, 1) for k, v in sdrs.items()})
    bad = {k: v for k, v in sdrs.items() if v < BF16_FEATURE_DB}
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 7. the two decoders
@pytest.mark.parametrize("case,prompt", [("short", "bass"), ("mid", "vocals")])
def test_head_matches_native_decoder(models, oracle_model, text_table, case, prompt):
    from athd.head import TrainableHead
    wav = _wav(case)
    assert _phase_cond(oracle_model.prepare(wav)[0]) >= PHASE_COND_MIN
    B = wav.shape[0]
    for dt, gate in (("f32", F32_SDR_DB), ("bf16", BF16_SDR_DB)):
        m = models[dt]
        head = TrainableHead.from_model(m).cuda().eval()
        with torch.no_grad():
            got = head(m.encode(wav.cuda()), _rows(text_table, [prompt] * B))
        want = m(wav.cuda(), prompt)
        assert got.shape == want.shape and got.dtype == torch.float32
        s = H.sdr_db(want.cpu().numpy(), got.cpu().numpy())
        _report(f"head_vs_native/{case}/{dt}", s)
        print(case, dt, round(s, 1))
        assert s >= gate, (dt, s)


# ------------------------------------------------------------------------------------------ 8. gradients
def test_gradients_against_float64(models, oracle_model, state_dict, text_table):
    from athd.head import HeadTrainer
    from athd.loss import combined_loss
    from athd.synth import synthetic_batch
    from train_refs import LOSSES, total64
    B, T, _ = CASES["short"]
    mix = _wav("short").cuda()
    target = 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=211))
    prompts = ["bass", "vocals"]
    m = models["f32"]
    trainer = HeadTrainer(m)
    trainer.train()
    combined_loss(trainer(mix, prompts), target.cuda())[0].backward()
    got = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().double()
           for k, p in trainer.head.named_parameters()}
    # the float64 reference on the CPU, fed the exported features; its own f32 evaluation gives the allowance
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
        a = float((g32[k].double() - w).abs().max()) / mx          # the reference's own noise on this case
        gap = float((got[k] - w).abs().max()) / mx
        worst[k] = gap / a
    for k in ("text_attn.attn.in_proj_weight", "text_attn.attn.in_proj_bias"):
        assert float(got[k][:768].abs().max()) <= 1e-9 * largest, k
    top = max(worst, key=worst.get)
    _report("head_grad_f32_vs_f64", {"worst_ratio_to_oracle_f32_gap": worst[top], "tensor": top})
    print("worst gap / oracle f32 gap:", top, worst[top])
    bad = {k: v for k, v in worst.items() if v > 4.0}
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 9. round trip
def test_round_trip_into_inference(state_dict, text_table):
    from athd.head import HeadTrainer
    from athd.loss import combined_loss
    from athd.synth import synthetic_batch
    B, T, _ = CASES["short"]
    m = _new_model(state_dict, text_table, "f32")
    wav = _wav("short").cuda()
    target = 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=211)).cuda()
    before = m(wav, "bass").clone()
    trainer = HeadTrainer(m)
    trainer.train()
    opt = torch.optim.SGD(trainer.parameters(), lr=1e-2)
    combined_loss(trainer(wav, ["bass"] * B), target)[0].backward()
    opt.step()
    trainer.sync()
    trainer.eval()
    after = m(wav, "bass")
    with torch.no_grad():
        via_head = trainer(wav, ["bass"] * B)
    s = H.sdr_db(after.cpu().numpy(), via_head.cpu().numpy())
    _report("head_round_trip_f32", s)
    assert s >= F32_SDR_DB, s
    assert not torch.allclose(after, before)
    assert sorted(trainer.state_dict()) == sorted(k for k, _ in __import__("athd.head").head.head_keys())


# ------------------------------------------------------------------------------------------ 10. train_epoch
def test_train_epoch_matches_float64_loop(state_dict, text_table, oracle_model):
    from athd.head import HeadTrainer, TrainableHead
    from athd.synth import synthetic_batch
    from athd.train import train_epoch
    from train_refs import train_epoch_ref
    B, T = 2, 4096
    prompts = [["bass", "vocals"], ["drums", "other"], ["vocals", "drums"]]
    batches = [{"mixture": torch.as_tensor(synthetic_batch(B, T, seed0=300 + i)),
                "target": 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=400 + i)), "prompt": prompts[i]}
               for i in range(3)]
    trainer = HeadTrainer(_new_model(state_dict, text_table, "f32"))
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
    _report("head_train_epoch", {"got": got, "want": want})
    for k in ("loss", "sdr", "sisdr"):
        assert abs(got[k] - want[k]) <= 1e-3, (k, got[k], want[k])


# ------------------------------------------------------------------------------------------ 11. determinism, capture
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_encode_deterministic_and_capturable(models, dt):
    m = models[dt]
    wav = _wav("short").cuda()
    a, b = m.encode(wav), m.encode(wav)
    for name, x, y in zip(NAMES, _flat(a), _flat(b)):
        assert torch.equal(torch.view_as_real(x) if name == "z" else x, torch.view_as_real(y) if name == "z" else y), name
    from athd.synth import synthetic_batch
    buf = torch.as_tensor(synthetic_batch(2, 4096, seed0=55)).cuda().contiguous()
    g, feats = m.capture_encode(buf)
    buf.copy_(wav)
    g.replay()
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, _flat(feats), _flat(a)):
        assert torch.equal(torch.view_as_real(x) if name == "z" else x, torch.view_as_real(y) if name == "z" else y), name


# ------------------------------------------------------------------------------------------ 12. the forward is untouched
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_unchanged_by_encode(models, dt):
    m = models[dt]
    wav = _wav("short").cuda()
    ctx = m._ensure_ctx()
    sizes = [ctx.workspace_bytes(2, 4096, 1), ctx.workspace_bytes(3, 9999, 4)]
    before = m(wav, "drums").clone()
    m.encode(_wav("mid").cuda())
    after = m(wav, "drums")
    assert torch.equal(before, after)
    assert [ctx.workspace_bytes(2, 4096, 1), ctx.workspace_bytes(3, 9999, 4)] == sizes
    assert ctx.encode_workspace_bytes(2, 4096) == sizes[0]


def test_encode_argument_errors(models):
    """a null member, a small workspace (as the forward: ATHD_EINVAL / ATHD_EWORKSPACE) and a call before finalize"""
    from athd import native
    m = models["f32"]
    ctx = m._ensure_ctx()
    f, feats = m._feature_buffers(1, 4096)
    wav = _wav("short")[:1].cuda().contiguous()
    ws = torch.empty(ctx.encode_workspace_bytes(1, 4096), dtype=torch.uint8, device="cuda")
    h, stream = ctx.h, torch.cuda.current_stream().cuda_stream
    import ctypes
    assert native.lib.athd_encode(h, wav.data_ptr(), 1, 4096, ctypes.byref(f), ws.data_ptr(), ws.numel() - 1, stream) == -5
    f.skip_t[2] = None
    assert native.lib.athd_encode(h, wav.data_ptr(), 1, 4096, ctypes.byref(f), ws.data_ptr(), ws.numel(), stream) == -1
    fresh = native.Context(0, native.F32)
    g, _ = m._feature_buffers(1, 4096)
    assert native.lib.athd_encode(fresh.h, wav.data_ptr(), 1, 4096, ctypes.byref(g), ws.data_ptr(), ws.numel(), stream) == -3
    fresh.close()
    torch.cuda.synchronize()
