"""References of the CLAP text tower tests (tests/test_clap_text_refs.py on the CPU, tests/test_gpu_clap_text.py on the
GPU): the float64 restatement of the semantics stated in include/athd.h (`athd_text_*`), a bf16 emulation of it, the
token-id cases and the error measure.  A plain helper module; torch on the CPU only.

Restatement, per prompt of ids / mask (P, L):
  pos = cumsum(ids != 1) * (ids != 1) + 1;  x = LN(word[id] + type[0] + position[pos])
  per layer: q, k, v = linear(x); softmax(q k^T / 8) over the keys with mask != 0 (probability exactly 0 elsewhere);
             x = LN(out(attn) + x);  x = LN(W2 gelu_erf(W1 x + b1) + b2 + x)            (LayerNorm eps 1e-12)
  pooled = tanh(dense(x[:, 0]));  emb = linear2(relu(linear1(pooled)));  normalize: emb / max(||emb||, 1e-12)

bf16 emulation: the 2-D weights outside the embedding tables and every GEMM input (the fp32 value, as the kernel holds
it) rounded to bf16; everything else float64 - q k^T, P V, the softmax and the LayerNorms are not rounded.
"""
import math

import numpy as np
import torch

VOCAB, PAD, BOS, EOS = 50265, 1, 0, 2
H, HEADS, DH, LAYERS, PROJ = 768, 12, 64, 12, 512
EPS = 1e-12
SEED = 3                                     # synthetic_clap_text_state_dict(SEED) everywhere in these tests

# ---- measured on the CPU over CASES (tests/test_clap_text_refs.py asserts both) ----
# r32: err(transformers ClapTextModelWithProjection fp32 forward = tests/golden/clap_text_ref.npz, float64 restatement)
# measured per case 5.0e-7 .. 1.59e-6 (transformers 5.15.0), rounded up to one digit: the fp32 side moves with the BLAS's
# summation order
R32 = 2.0e-6
# rbf: err(bf16 emulation, float64 restatement)
# measured per case 8.7e-3 .. 1.373e-2, cosine >= 0.99989
RBF = 1.4e-2


def _prompt(rng, n, L):
    """n tokens `<s> ... </s>` with n - 2 ids from [3, VOCAB), padded with 1 to L"""
    assert 2 <= n <= L
    body = rng.integers(3, VOCAB, size=n - 2).tolist()
    return [BOS] + body + [EOS] + [PAD] * (L - n)


def _batch(seed, lengths, L):
    rng = np.random.default_rng(seed)
    ids = np.array([_prompt(rng, n, max(lengths)) for n in lengths], dtype=np.int64)   # the same ids at every padding
    ids = np.concatenate([ids, np.full((len(lengths), L - ids.shape[1]), PAD, dtype=np.int64)], axis=1)
    return ids, (ids != PAD).astype(np.int64)


RAGGED = (4, 9, 2, 6)
CASES = {
    "bos_eos": _batch(10, (2,), 2),                      # <s></s> alone
    "ragged9": _batch(11, RAGGED, 9),
    "ragged17": _batch(11, RAGGED, 17),                  # the same batch padded further
    "ragged33": _batch(11, RAGGED, 33),
    "one16": _batch(12, (16,), 16),
    "five17": _batch(13, (17, 5, 11, 3, 14), 17),        # 85 rows: past a 16-row tile and a 64-row M block
    "long128": _batch(14, (128,), 128),
}


def err(a, b):
    """max over prompts of max|a - b| / max|b|"""
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return float(((a - b).abs().amax(dim=1) / b.abs().amax(dim=1)).max())


def bf16_round(x):
    """the fp32 value rounded to bf16 (round to nearest even), as float64"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


_cache = {}


def weights64(sd, bf16=False):
    """sd (numpy float32) -> {key: float64 tensor}; bf16: the 2-D weights outside the embedding tables rounded"""
    key = (id(sd), bool(bf16))
    if key not in _cache:
        w = {}
        for k, v in sd.items():
            t = torch.from_numpy(np.asarray(v))
            if bf16 and t.dim() == 2 and "embeddings" not in k:
                t = t.to(torch.bfloat16)
            w[k] = t.to(torch.float64)
        _cache[key] = (sd, w)                # (keeps sd alive so that its id stays its own)
    return _cache[key][1]


def _ln(x, w, b):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + EPS) * w + b


def restatement(sd, ids, mask, normalize=False, bf16=False, use_mask=True):
    """(P, 512) float64"""
    w = weights64(sd, bf16)
    rnd = bf16_round if bf16 else (lambda t: t)
    ids = torch.as_tensor(np.asarray(ids)).long()
    mask = torch.as_tensor(np.asarray(mask)).long()
    P, L = ids.shape
    keep = (ids != PAD).long()
    pos = torch.cumsum(keep, 1) * keep + PAD
    e = "text_model.embeddings."
    x = w[e + "word_embeddings.weight"][ids] + w[e + "token_type_embeddings.weight"][0] + \
        w[e + "position_embeddings.weight"][pos]
    x = _ln(x, w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"])

    def lin(t, p):
        return rnd(t) @ w[p + ".weight"].T + w[p + ".bias"]

    kept = (mask != 0) if use_mask else torch.ones_like(mask, dtype=torch.bool)
    for i in range(LAYERS):
        p = f"text_model.encoder.layer.{i}."
        q, k, v = (lin(x, p + "attention.self." + n).view(P, L, HEADS, DH).transpose(1, 2)
                   for n in ("query", "key", "value"))
        s = q @ k.transpose(-1, -2) / 8.0
        s = s.masked_fill(~kept[:, None, None, :], -math.inf)
        a = torch.softmax(s, dim=-1)                                     # exp(-inf) = 0 exactly
        ctx = (a @ v).transpose(1, 2).reshape(P, L, H)
        x = _ln(lin(ctx, p + "attention.output.dense") + x, w[p + "attention.output.LayerNorm.weight"],
                w[p + "attention.output.LayerNorm.bias"])
        hmid = lin(x, p + "intermediate.dense")
        hmid = 0.5 * hmid * (1.0 + torch.erf(hmid / math.sqrt(2.0)))
        x = _ln(lin(hmid, p + "output.dense") + x, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"])
    pooled = torch.tanh(lin(x[:, 0], "text_model.pooler.dense"))
    emb = lin(torch.relu(lin(pooled, "text_projection.linear1")), "text_projection.linear2")
    if normalize:
        emb = emb / emb.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return emb


def hf_model(sd):
    """transformers' ClapTextModelWithProjection (fp32, CPU, eval) holding sd"""
    from transformers import ClapTextConfig, ClapTextModelWithProjection
    cfg = ClapTextConfig(vocab_size=VOCAB, hidden_size=H, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                         intermediate_size=3072, max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=EPS,
                         projection_dim=PROJ, hidden_act="gelu", projection_hidden_act="relu", pad_token_id=PAD,
                         hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = ClapTextModelWithProjection(cfg).eval()
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith(("position_ids", "token_type_ids")) for k in missing), (missing, unexpected)
    return m


def hf_forward(model, ids, mask):
    with torch.no_grad():
        return model(input_ids=torch.as_tensor(np.asarray(ids)).long(),
                     attention_mask=torch.as_tensor(np.asarray(mask)).long()).text_embeds
