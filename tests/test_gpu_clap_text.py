"""The native CLAP text tower on the GPU: `athd_text_*` (csrc/text_tower.{hip,cpp}), `athd.text.NativeClapText`,
`PromptEmbedder(native=)` and `AudioTextHTDemucs(native_text=True)`, against the float64 restatement of
tests/clap_text_refs.py on the synthetic tower weights.

Tolerances (err = max over prompts of max|a - b| / max|b|, constants measured in tests/test_clap_text_refs.py):
  f32  err(native, restatement) <= 4 x R32   (the factor the spectrogram tests give torch's own fp32 noise)
  bf16 err(native, restatement) <= 2 x RBF   (the emulation leaves q k^T, P V and the LayerNorms unrounded, as the
                                              kernels do: their rounding points are the emulation's)
Independence of batch, padding, run and graph replay is checked bit for bit.  Kernel level (tests/ktest_text.py):
the skinny GEMM against numpy float64 within K 2^-24 sum|x||w| per element (bf16: on the bf16-rounded operands), an
activation's Lipschitz constant (1.13 for GELU, 1 otherwise) and 4 ulp of its fp32 evaluation on top where there is
one; the attention kernel within the bound derived at `_attn_bound`.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import clap_text_refs as R
import ktest as kt
import ktest_text as ktt

pytestmark = pytest.mark.gpu

EINVAL, EKEY, ESTATE, EWORKSPACE = -1, -2, -3, -5
SENTINEL = -12345.5
U = 2.0 ** -24
DTYPES = ["f32", "bf16"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Tower:
    def __init__(self):
        from athd.text import NativeClapText
        from athd.weights import synthetic_clap_text_state_dict
        self.sd = synthetic_clap_text_state_dict(R.SEED)
        self.nat = {}
        for d in DTYPES:
            n = NativeClapText("cuda", dtype=d)
            n.load_state_dict(self.sd)
            n._ensure_ctx()
            self.nat[d] = n
        self._ref = {}

    def ref(self, case, normalize=False):
        key = (case, bool(normalize))
        if key not in self._ref:
            ids, mask = R.CASES[case]
            self._ref[key] = R.restatement(self.sd, ids, mask, normalize=normalize)
        return self._ref[key]

    def fresh_ctx(self, dtype):
        """a new finalized context (its first encode has not happened yet)"""
        from athd import native
        ctx = native.TextContext(0, native.BF16 if dtype == "bf16" else native.F32)
        for k, v in self.sd.items():
            ctx.set_weight("clap." + k, v)            # the checkpoint's prefix is stripped
        ctx.finalize()
        return ctx


@pytest.fixture(scope="module")
def tower():
    return Tower()


def _dev(ids, mask):
    return (torch.as_tensor(np.asarray(ids)).to(torch.int32).cuda().contiguous(),
            torch.as_tensor(np.asarray(mask)).to(torch.int32).cuda().contiguous())


def _raw(ctx, ids, mask, normalize=0):
    """athd_text_encode with a sentinel row after `out` and sentinel bytes after the workspace -> (rc, out (P, 512))"""
    from athd import native
    ids, mask = _dev(ids, mask)
    P, L = ids.shape
    need = native.lib.athd_text_workspace_bytes(ctx.h, P, L)
    assert need > 0
    out = torch.full((P + 1, 512), SENTINEL, dtype=torch.float32, device="cuda")
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = native.lib.athd_text_encode(ctx.h, ids.data_ptr(), mask.data_ptr(), P, L, normalize, out.data_ptr(),
                                     ws.data_ptr(), need, _stream())
    kt.sync()
    assert torch.all(out[P] == SENTINEL), "a row past out was written"
    assert torch.all(ws[need:] == 0x5A), "bytes past the workspace were written"
    return rc, out[:P].clone()


def _enc(tower, dtype, ids, mask, normalize=0):
    rc, out = _raw(tower.nat[dtype]._ctx, ids, mask, normalize)
    assert rc == 0
    return out


# ------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("case", list(R.CASES))
def test_f32_matches_restatement(tower, case, normalize):
    got = _enc(tower, "f32", *R.CASES[case], normalize=normalize).cpu()
    e = R.err(got, tower.ref(case, normalize))
    print(f"f32 {case} normalize={normalize}: err {e:.3e} (bound {4 * R.R32:.1e})")
    assert torch.isfinite(got).all() and e <= 4 * R.R32, e
    if normalize:
        assert torch.allclose(got.double().norm(dim=1), torch.ones(got.shape[0], dtype=torch.float64), atol=1e-6)


@pytest.mark.parametrize("case", list(R.CASES))
def test_bf16_matches_restatement(tower, case):
    got = _enc(tower, "bf16", *R.CASES[case]).cpu()
    e = R.err(got, tower.ref(case))
    cos = float(torch.nn.functional.cosine_similarity(got.double(), tower.ref(case), dim=1).min())
    print(f"bf16 {case}: err {e:.3e} (bound {2 * R.RBF:.1e}) cosine {cos:.6f}")
    assert torch.isfinite(got).all() and e <= 2 * R.RBF, e


def test_python_wrapper_equals_the_raw_call(tower):
    ids, mask = R.CASES["ragged9"]
    for d in DTYPES:
        for nrm in (False, True):
            a = tower.nat[d].encode(torch.as_tensor(ids), torch.as_tensor(mask), nrm)      # int64 CPU tensors
            assert a.dtype == torch.float32 and a.is_cuda and tuple(a.shape) == (4, 512)
            assert torch.equal(a, _enc(tower, d, ids, mask, int(nrm)))
    with pytest.raises(ValueError):
        tower.nat["f32"].encode(torch.zeros(1, 129, dtype=torch.long), torch.ones(1, 129, dtype=torch.long), False)


# ------------------------------------------------------------------------------------------------- bit-exactness
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_depend_on_batch_padding_or_run(tower, dtype):
    ids9, mask9 = R.CASES["ragged9"]
    base = _enc(tower, dtype, ids9, mask9)
    assert torch.equal(base, _enc(tower, dtype, ids9, mask9))                        # two runs
    for n in ("ragged17", "ragged33"):                                               # padded further
        assert torch.equal(base, _enc(tower, dtype, *R.CASES[n])), n
    for i, n in enumerate(R.RAGGED):                                                 # alone, at L = 9 and unpadded
        assert torch.equal(base[i:i + 1], _enc(tower, dtype, ids9[i:i + 1], mask9[i:i + 1])), i
        assert torch.equal(base[i:i + 1], _enc(tower, dtype, ids9[i:i + 1, :n], mask9[i:i + 1, :n])), i
    five = _enc(tower, dtype, *R.CASES["five17"])                                    # rows in the second 64-row block
    ids, mask = R.CASES["five17"]
    assert torch.equal(five[4:5], _enc(tower, dtype, ids[4:5], mask[4:5]))
    assert torch.equal(five.flip(0),
                       _enc(tower, dtype, ids[::-1].copy(), mask[::-1].copy()))      # the batch in reverse order


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_captured_at_the_first_call(tower, dtype):
    """Everything one-time happens in athd_text_finalize: the context's very first encode is captured, replayed on
    other ids, and equals the eager call bit for bit."""
    from athd import native
    ctx = tower.fresh_ctx(dtype)
    ids, mask = _dev(*R.CASES["ragged9"])
    P, L = ids.shape
    out = torch.full((P, 512), SENTINEL, dtype=torch.float32, device="cuda")
    need = ctx.workspace_bytes(P, L)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def run():
        assert native.lib.athd_text_encode(ctx.h, ids.data_ptr(), mask.data_ptr(), P, L, 1, out.data_ptr(),
                                           ws.data_ptr(), need, _stream()) == 0

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    perm = [2, 0, 3, 1]
    ids.copy_(ids[perm].clone())
    mask.copy_(mask[perm].clone())
    ws.fill_(0xFF)
    graph.replay()
    kt.sync()
    replayed = out.clone()
    out.fill_(SENTINEL)
    run()
    kt.sync()
    assert torch.equal(replayed, out) and not torch.any(out == SENTINEL)
    assert torch.equal(out, _enc(tower, dtype, *R.CASES["ragged9"], normalize=1)[perm])
    ctx.close()


# -------------------------------------------------------------------------------------------------- clean failure
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_ids_and_empty_masks_stay_in_their_row(tower, dtype):
    """An id outside the table is clamped into it (tt_embed_kernel: min(max(id, 0), 50264); the position index is at
    most L + 1), a prompt with an all-zero mask gets zero probabilities: rc 0, the other rows bit-identical."""
    ids9, mask9 = R.CASES["ragged9"]
    base = _enc(tower, dtype, ids9, mask9)
    for bad in (-1, R.VOCAB, 2 ** 31 - 1, -2 ** 31):
        ids = ids9.copy()
        ids[1, 3] = bad
        rc, got = _raw(tower.nat[dtype]._ctx, ids, mask9)
        assert rc == 0 and torch.isfinite(got).all()
        assert torch.equal(got[[0, 2, 3]], base[[0, 2, 3]]), bad
    mask = mask9.copy()
    mask[1, :] = 0
    rc, got = _raw(tower.nat[dtype]._ctx, ids9, mask)
    assert rc == 0 and torch.isfinite(got).all()
    assert torch.equal(got[[0, 2, 3]], base[[0, 2, 3]])


# --------------------------------------------------------------------------------------------------- status codes
def test_refusals_write_nothing(tower):
    from athd import native
    ctx = tower.nat["f32"]._ctx
    ids, mask = _dev(*R.CASES["ragged9"])
    P, L = ids.shape
    need = ctx.workspace_bytes(P, L)
    out = torch.full((P, 512), SENTINEL, dtype=torch.float32, device="cuda")
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    ok = dict(ids=ids.data_ptr(), mask=mask.data_ptr(), P=P, L=L, out=out.data_ptr(), ws=ws.data_ptr(), n=need)

    def call(h=ctx.h, **kw):
        a = {**ok, **kw}
        return native.lib.athd_text_encode(h, a["ids"], a["mask"], a["P"], a["L"], 0, a["out"], a["ws"], a["n"],
                                           _stream())

    for kw in (dict(P=0), dict(P=257), dict(L=0), dict(L=129), dict(P=-1), dict(ids=None), dict(mask=None),
               dict(out=None), dict(ws=None)):
        assert call(**kw) == EINVAL, kw
    assert call(h=None) == EINVAL
    assert call(n=need - 1) == EWORKSPACE and call(n=0) == EWORKSPACE
    assert b"workspace" in native.lib.athd_text_last_error(ctx.h)
    for P_, L_ in ((0, 9), (257, 9), (4, 0), (4, 129)):
        assert native.lib.athd_text_workspace_bytes(ctx.h, P_, L_) == 0
    assert ctx.workspace_bytes(256, 128) > ctx.workspace_bytes(4, 9) > 0

    fresh = native.TextContext(0, native.F32)
    assert call(h=fresh.h) == ESTATE
    assert native.lib.athd_text_finalize(fresh.h) == EKEY                  # nothing staged: a missing key
    assert b"missing" in native.lib.athd_text_last_error(fresh.h)
    e = "text_model.embeddings."
    for k in list(tower.sd)[:5]:
        assert k.startswith(e)
        fresh.set_weight(k, tower.sd[k])
    fresh.set_weight("text_model.embeddings.position_ids", np.zeros((1, 514), np.float32))      # ignored
    fresh.set_weight("clap.audio_model.some.weight", np.zeros((3,), np.float32))                # ignored
    q = "text_model.encoder.layer.0.attention.self.query.weight"
    fresh.set_weight(q, np.zeros((768, 767), np.float32))
    assert native.lib.athd_text_finalize(fresh.h) == EKEY
    assert q.encode() in native.lib.athd_text_last_error(fresh.h)
    assert call(h=fresh.h) == ESTATE
    fresh.close()
    assert native.lib.athd_text_create(None, 0, 0) == EINVAL
    h = ctypes.c_void_p()
    assert native.lib.athd_text_create(ctypes.byref(h), 0, 7) == EINVAL

    kt.sync()
    assert torch.all(out == SENTINEL) and torch.all(ws == 0x5A)
    assert call() == 0
    kt.sync()
    assert not torch.any(out == SENTINEL)


# ---------------------------------------------------------------------------------------------------- kernel level
def test_descriptor_sizes_and_plans():
    for n, (a, b) in ktt.sizes_match().items():
        assert a == b, n
    for N, K in ktt.SHAPES:
        p = ktt.gemm_plan(N, K)
        assert p["S"] * p["W"] * p["KW"] == K and (N // 16) * p["S"] >= 256, (N, K, p)
    assert ktt.gemm_plan(768, 512) is None


EPILOGUE = {(2304, 768): ("bias", ktt.ACT_NONE), (768, 768): ("res", ktt.ACT_NONE), (3072, 768): ("bias", ktt.ACT_GELU),
            (768, 3072): ("res", ktt.ACT_NONE), (512, 768): ("bias", ktt.ACT_RELU), (512, 512): ("bias", ktt.ACT_NONE)}


def _gemm_case(N, K, M, bf16, epi, act, ldx_extra=0, seed=0):
    rng = np.random.default_rng(zlib.crc32(f"{N},{K},{M},{bf16},{seed}".encode()))
    ldx = K + ldx_extra
    X = rng.standard_normal((M, ldx)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    res = rng.standard_normal((M, N)).astype(np.float32) if epi == "res" else None
    S = ktt.gemm_plan(N, K)["S"]
    bX = kt.Buf(X, "f32", 64)
    bW = kt.Buf(ktt.bf16_bits(W), "bf16", 64) if bf16 else kt.Buf(W, "f32", 64)
    bB = kt.Buf(bias, "f32", 64)
    bR = kt.Buf(res, "f32", 64) if res is not None else None
    bP = kt.Buf(np.zeros(S * M * N, np.float32), "f32", 4096, output=True)
    bO = kt.Buf(np.full(M * N, kt.F32_SENTINEL, np.float32), "f32", 4096, output=True)
    d = kt.fill(ktt.KtTtGemm, W=bW.ptr, bf16=int(bf16), X=bX.ptr, ldx=ldx, M=M, N=N, K=K, bias=bB.ptr,
                res=bR.ptr if bR else None, ldr=N, act=act, part=bP.ptr, out=bO.ptr, ldo=N)
    rc = ktt.lib.kt_tt_gemm(ctypes.byref(d), _stream())
    kt.sync()
    assert rc == 0
    got, intact = bO.host()
    _, part_intact = bP.host()
    assert intact and part_intact, "a guard band was written"
    Xe = (ktt.bf16_value(X[:, :K]) if bf16 else X[:, :K]).astype(np.float64)
    We = (ktt.bf16_value(W) if bf16 else W).astype(np.float64)
    z = Xe @ We.T + bias + (res if res is not None else 0.0)
    ref = ktt.act64(z, act)
    bound = K * U * (np.abs(Xe) @ np.abs(We).T)
    if act != ktt.ACT_NONE:
        bound = bound * (1.13 if act == ktt.ACT_GELU else 1.0) + 4 * U * np.abs(ref)
    diff = np.abs(got.reshape(M, N).astype(np.float64) - ref)
    assert not np.any(got == np.float32(kt.F32_SENTINEL))
    worst = float((diff / bound).max())
    assert worst <= 1.0, (N, K, M, bf16, worst)
    return worst


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N,K", ktt.SHAPES)
def test_skinny_gemm(N, K, bf16):
    epi, act = EPILOGUE[(N, K)]
    worst = [(_gemm_case(N, K, M, bf16, epi, act, ldx_extra=64 if M == 15 else 0)) for M in (1, 2, 15, 16, 17, 64, 65)]
    print(f"tt_gemm N={N} K={K} bf16={bf16} {epi}/{act}: worst diff/bound per M {[f'{w:.3f}' for w in worst]}")


@pytest.mark.parametrize("bf16", [False, True])
def test_skinny_gemm_pooler_rows(bf16):
    """tanh on first-token rows: row stride L * 768 as the pooler reads them"""
    w = _gemm_case(768, 768, 5, bf16, "bias", ktt.ACT_TANH, ldx_extra=8 * 768)
    print(f"tt_gemm pooler bf16={bf16}: worst diff/bound {w:.3f}")


def _attn_bound(q, k, v, p):
    """fp32 evaluation of softmax(q k^T / 8) v with exact inputs: a score carries at most 66 roundings of sum|q_d k_d| / 8
    (64 fmas, the scale is exact, the subtraction of the maximum), so every exponent is off by at most ds = 66 u max_j
    sum_d|q_d k_d| / 8 and every probability by the relative 2 ds + 8 u (expf and the division, the denominator's L
    additions of positive terms another L u); the L fmas of P V add L u.  Per element: (2 ds + (2 L + 16) u) sum_j p_j |v_jd|."""
    L = q.shape[0]
    ds = 66 * U * (np.abs(q) @ np.abs(k).T).max(axis=1, keepdims=True) / 8.0            # (L, 1)
    return (2 * ds + (2 * L + 16) * U) * (p @ np.abs(v)) + 1e-30


@pytest.mark.parametrize("L", [1, 2, 9, 17, 33, 128])
def test_attention_kernel(L):
    """P = 3 prompts: every key kept, a ragged mask, only key 0 kept.  q, k, v arrive as two split-K slices and a
    bias on a 2^-6 grid, so that their sums are exact in fp32 and the bound is about the attention alone."""
    rng = np.random.default_rng(100 + L)
    P, S, N = 3, 2, 2304
    M = P * L
    grid = lambda *s: rng.integers(-64, 65, size=s).astype(np.float32) / 64.0
    part, bias = grid(S, M, N), grid(N)
    mask = np.ones((P, L), np.int32)
    mask[1] = rng.integers(0, 2, size=L)
    mask[1, 0] = 1
    mask[2, 1:] = 0
    bP, bB = kt.Buf(part, "f32", 64), kt.Buf(bias, "f32", 64)
    bM = torch.from_numpy(mask).cuda()
    bO = kt.Buf(np.full(M * 768, kt.F32_SENTINEL, np.float32), "f32", 4096, output=True)
    d = kt.fill(ktt.KtTtAttn, part=bP.ptr, S=S, bias=bB.ptr, mask=bM.data_ptr(), P=P, L=L, out=bO.ptr)
    rc = ktt.lib.kt_tt_attn(ctypes.byref(d), _stream())
    kt.sync()
    assert rc == 0
    got, intact = bO.host()
    assert intact and not np.any(got == np.float32(kt.F32_SENTINEL))
    got = got.reshape(P, L, 12, 64).astype(np.float64)
    qkv = (part.astype(np.float64).sum(0) + bias).reshape(P, L, 3, 12, 64)
    worst = 0.0
    for p_ in range(P):
        for h in range(12):
            q, k, v = (qkv[p_, :, i, h] for i in range(3))
            s = q @ k.T / 8.0
            s[:, mask[p_] == 0] = -np.inf
            e = np.exp(s - s.max(axis=1, keepdims=True))
            pr = e / e.sum(axis=1, keepdims=True)
            ref = pr @ v
            worst = max(worst, float((np.abs(got[p_, :, h] - ref) / _attn_bound(q, k, v, pr)).max()))
            if p_ == 2:
                assert np.array_equal(got[p_, :, h], np.broadcast_to(v[0], (L, 64)))      # only key 0: its v, exactly
    print(f"tt_attn L={L}: worst diff/bound {worst:.3f}")
    assert worst <= 1.0, worst


# ----------------------------------------------------------------------------------------------------- integration
class WordTokenizer:
    """RoBERTa-shaped stand-in: <s> = 0, </s> = 2, pad = 1, one id in [3, 50265) per word, padded to the longest"""
    calls = 0

    def __call__(self, prompts, padding=True, return_tensors="pt"):
        assert padding is True and return_tensors == "pt"
        type(self).calls += 1
        seqs = [[0] + [3 + zlib.crc32(w.encode()) % (R.VOCAB - 3) for w in p.split()] + [2] for p in prompts]
        n = max(map(len, seqs))
        ids = torch.tensor([s + [1] * (n - len(s)) for s in seqs])
        return {"input_ids": ids, "attention_mask": (ids != 1).long()}


def test_prompt_embedder_uses_and_caches_the_native_tower(tower):
    from athd.text import PromptEmbedder
    nat, tok = tower.nat["f32"], WordTokenizer()
    prompts = ["drums", "the bass guitar", "vocals"]
    inp = tok(sorted(prompts))
    for source, nrm in ((None, True), ("ClapModel", True), ("ClapTextModelWithProjection", False)):
        e = PromptEmbedder(tokenizer=tok, native=nat, native_source=source)
        before = nat.calls
        rows = e.rows(prompts, 3)
        assert nat.calls == before + 1
        want = dict(zip(sorted(prompts), nat.encode(inp["input_ids"], inp["attention_mask"], nrm).cpu()))
        assert rows.shape == (3, 512) and all(torch.equal(rows[i], want[p]) for i, p in enumerate(prompts))
        n = nat.calls
        again = e.rows(["vocals", "drums"], 2)
        assert nat.calls == n and torch.equal(again[0], rows[2]) and torch.equal(again[1], rows[0])   # cached
    assert torch.equal(nat.embed(prompts, tok, True), nat.encode(tok(prompts)["input_ids"],
                                                                 tok(prompts)["attention_mask"], True))


def test_load_clap_state_feeds_the_tower_and_drops_cached_rows(tower):
    from athd.text import NativeClapText, PromptEmbedder
    nat = NativeClapText("cuda", dtype="bf16")
    e = PromptEmbedder(tokenizer=WordTokenizer(), native=nat, table={"given": np.ones(512, np.float32)})
    with pytest.raises(RuntimeError, match="load_state_dict"):
        e.rows("vocals", 1)
    with pytest.raises(KeyError, match="missing.*text_projection.linear2.bias"):
        e.load_clap_state({k: v for k, v in tower.sd.items() if k != "text_projection.linear2.bias"})
    e.load_clap_state(dict(tower.sd))
    first = e.rows("vocals", 1).clone()
    assert torch.equal(first, tower.nat["bf16"].embed(["vocals"], WordTokenizer(), True).cpu())
    changed = dict(tower.sd)
    changed["text_projection.linear2.weight"] = -tower.sd["text_projection.linear2.weight"]
    e.load_clap_state(changed)
    assert "vocals" not in e.table and "given" in e.table
    second = e.rows("vocals", 1)
    assert not torch.equal(first, second)


@pytest.fixture(scope="module")
def native_model(tower, state_dict):
    from athd.model import AudioTextHTDemucs
    sd = dict(state_dict)
    sd.update({"clap." + k: v for k, v in tower.sd.items()})
    sd["clap.text_model.embeddings.position_ids"] = np.arange(514, dtype=np.int64)[None]
    m = AudioTextHTDemucs(None, None, WordTokenizer(), dtype="bf16", native_text=True)
    missing, unexpected = m.load_state_dict(sd)
    assert not missing and not any(k.startswith("clap.text_projection") for k in unexpected)
    return m.to("cuda").eval()


def test_model_with_native_text_equals_a_text_table_forward(tower, native_model, state_dict):
    from athd.model import AudioTextHTDemucs
    from athd.synth import synthetic_batch
    wav = torch.as_tensor(synthetic_batch(1, 1500)).cuda()
    prompt = "some prompt"
    out = native_model(wav, prompt)
    row = tower.nat["f32"].embed([prompt], WordTokenizer(), True)            # the f32 tower, get_text_features rows
    assert torch.equal(native_model.embedder.table[prompt], row[0].cpu())
    plain = AudioTextHTDemucs(dtype="bf16", text_table={prompt: row[0].cpu().numpy()})
    plain.load_state_dict(state_dict)
    want = plain.to("cuda").eval()(wav, prompt)
    assert tuple(out.shape) == (1, 2, 1500) and torch.isfinite(out).all() and torch.equal(out, want)


def test_encode_feeds_forward_prompts_on_one_stream(tower, native_model):
    """athd_text_encode -> athd_forward_prompts with the device rows as text_table, no host step in between"""
    from athd import native
    from athd.synth import synthetic_batch
    wav = torch.as_tensor(synthetic_batch(1, 1500)).cuda().contiguous()
    prompts = ["some prompt", "another longer prompt here"]
    want = native_model.forward_prompts(wav, prompts)
    inp = WordTokenizer()(prompts)
    ids, mask = _dev(inp["input_ids"], inp["attention_mask"])
    P, L = ids.shape
    tctx, ctx = tower.nat["f32"]._ctx, native_model._ensure_ctx()
    table = torch.full((P, 512), SENTINEL, dtype=torch.float32, device="cuda")
    tws = torch.empty(tctx.workspace_bytes(P, L), dtype=torch.uint8, device="cuda")
    out = torch.empty((1, P, 2, 1500), dtype=torch.float32, device="cuda")
    ws = torch.empty(ctx.workspace_bytes(1, 1500, P), dtype=torch.uint8, device="cuda")
    st = _stream()
    tctx.encode(ids.data_ptr(), mask.data_ptr(), P, L, True, table.data_ptr(), tws.data_ptr(), tws.numel(), st)
    ctx.forward_prompts(wav.data_ptr(), 1, 1500, table.data_ptr(), P, out.data_ptr(), ws.data_ptr(), ws.numel(), st)
    kt.sync()
    assert torch.equal(out, want)


def test_load_model_native_text(tower, state_dict, tmp_path, monkeypatch):
    import athd.inference as inf
    from athd.inference import load_model
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()}
    bare = tmp_path / "bare.pt"
    torch.save({"model_state_dict": sd}, bare)
    with pytest.raises(RuntimeError, match="clap.text_model"):
        load_model(str(bare), "cuda", native_text=True, tokenizer=WordTokenizer())
    with pytest.raises(ValueError, match="tokenizer"):
        load_model(str(bare), "cuda", native_text=True)
    sd.update({"clap." + k: torch.from_numpy(v) for k, v in tower.sd.items()})
    # (the 0.5 GB tower is handed over in memory instead of through a checkpoint file)
    monkeypatch.setattr(inf.torch, "load", lambda path, **kw: {"model_state_dict": sd})
    m = load_model("full.pt", "cuda", native_text=True, tokenizer=WordTokenizer())
    rows = m.embedder.rows(["vocals"], 1)
    assert torch.equal(rows, tower.nat["f32"].embed(["vocals"], WordTokenizer(), True).cpu())
