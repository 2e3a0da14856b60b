"""Shared inputs and float64 references for the head-training tests (tests/test_head_refs.py, tests/test_gpu_head.py)
and tests/golden/gen_head_fixture.py; a helper module, not a test file.

  * `seeded_features` / `seeded_text`: the random features of the T = 4096, B = 2 shapes the fixture was made on,
    regenerated from seeds (never stored);
  * `oracle_features`: the oracle's `prepare` + `encode` as an `EncodedFeatures`;
  * `oracle64`: the oracle with the 50 head tensors as float64 leaves, for autograd through its `decode`;
  * `branch_loss`, `strided`, `DEAD`.
"""
import numpy as np
import torch

from athd.head import head_keys
from athd.model import FREQ_ROWS, SKIP_CH, EncodedFeatures, time_lengths

STRIDE = 97                      # the fixture keeps elements 0::97 of every gradient (and its largest |g|)
FIX_B, FIX_T = 2, 4096
OUTPUTS = ("x_cond", "xt_cond", "xd", "xtd")
# mathematically zero gradient: one key, softmax == 1 (athd/head.py)
DEAD = tuple(f"text_attn.{m}.{p}" for m in ("q_proj", "k_proj", "norm_q") for p in ("weight", "bias"))


def seeded_features(dtype=torch.float64, B=FIX_B, T=FIX_T, seed=4242) -> EncodedFeatures:
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Ts, L = -(-T // 1024), time_lengths(T)
    x_enc, xt_enc = rnd(B, 384, 8, Ts), rnd(B, 384, L[4])
    skips = [rnd(B, SKIP_CH[i], FREQ_ROWS[i], Ts) for i in range(4)]
    skips_t = [rnd(B, SKIP_CH[i], L[i + 1]) for i in range(4)]
    z = torch.complex(rnd(B, 2, 2048, Ts), rnd(B, 2, 2048, Ts))
    meant, stdt = 0.01 * rnd(B, 1, 1), 0.2 + 0.05 * rnd(B, 1, 1).abs()
    c = lambda t: t.to(dtype)
    return EncodedFeatures(c(x_enc), c(xt_enc), [c(s) for s in skips], [c(s) for s in skips_t],
                           z.to(torch.complex128 if dtype == torch.float64 else torch.complex64), c(meant), c(stdt),
                           [Ts] * 4, L[:4], T)


def seeded_text(dtype=torch.float64, B=FIX_B, seed=4243) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, 512, generator=g, dtype=torch.float64)
    return (t / t.norm(dim=1, keepdim=True)).to(dtype)


def head_state(state_dict, dtype=torch.float64):
    return {k: torch.as_tensor(state_dict[k]).to(dtype) for k, _ in head_keys()}


def branch_loss(xd: torch.Tensor, xtd: torch.Tensor) -> torch.Tensor:
    return (xd ** 2).mean() + (xtd ** 2).mean()


def strided(t) -> np.ndarray:
    return np.asarray(t.detach().cpu().double().reshape(-1)[::STRIDE].numpy())


def oracle_features(oracle_model, wav: torch.Tensor, dtype=torch.float64):
    """(EncodedFeatures, (z, mag, enc, meant, stdt) for `oracle.decode`), both in `dtype`, from the f32 oracle"""
    with torch.no_grad():
        z, mag, x, xt, meant, stdt = oracle_model.prepare(wav)
        x_enc, xt_enc, saved, saved_t, lengths, lengths_t = oracle_model.encode(x, xt)
    c = lambda t: t.to(dtype)
    zc = z.to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    enc = (c(x_enc), c(xt_enc), [c(s) for s in saved], [c(s) for s in saved_t], lengths, lengths_t)
    feats = EncodedFeatures(enc[0], enc[1], [s[:, :SKIP_CH[i]].contiguous() for i, s in enumerate(enc[2])],
                            [s[:, :SKIP_CH[i]].contiguous() for i, s in enumerate(enc[3])], zc[:, :2].contiguous(),
                            c(meant), c(stdt), list(lengths), list(lengths_t), wav.shape[-1])
    mag_c = oracle_model.htdemucs._magnitude(zc)
    return feats, (zc, mag_c, enc, c(meant), c(stdt))


def decode_inputs(oracle_model, feats: EncodedFeatures, dtype=torch.float64):
    """the arguments of `oracle.decode` rebuilt from an EncodedFeatures (e.g. exported by the library), in `dtype`"""
    c = lambda t: t.detach().cpu().to(dtype)
    zc = feats.z.detach().cpu().to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    enc = (c(feats.x_enc), c(feats.xt_enc), [c(s) for s in feats.skips], [c(s) for s in feats.skips_t],
           list(feats.lengths), list(feats.lengths_t))
    return zc, oracle_model.htdemucs._magnitude(zc), enc, c(feats.meant), c(feats.stdt)


def oracle_leaves(oracle_model, state_dict, dtype=torch.float64):
    """(AudioTextHTDemucsRef whose 50 head tensors are leaves of `dtype` requiring grad, {key: leaf})"""
    from oracle.athtdemucs_ref import AudioTextHTDemucsRef
    leaves = {k: v.clone().requires_grad_(True) for k, v in head_state(state_dict, dtype).items()}
    sd = dict(state_dict)
    sd.update(leaves)
    return AudioTextHTDemucsRef(sd, htdemucs=oracle_model.htdemucs), leaves


def oracle_grads(oracle_model, state_dict, dec_in, text, length, loss_fn, dtype=torch.float64):
    """({key: gradient}, output) of loss_fn(oracle.decode(...)) with respect to the 50 head tensors, in `dtype`"""
    ref, leaves = oracle_leaves(oracle_model, state_dict, dtype)
    z, mag, enc, meant, stdt = dec_in
    out = ref.decode(z, mag, enc, text.to(dtype), meant, stdt, length)
    loss_fn(out).backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in leaves.items()}, out.detach()


def sdr_db(ref, out) -> float:
    ref = np.asarray(ref, np.float64)
    out = np.asarray(out, np.float64)
    return float(10 * np.log10(np.sum(ref ** 2) / max(np.sum((ref - out) ** 2), 1e-300)))
