"""`athd.head.TrainableHead` on the CPU in float64: its key contract, its arithmetic against the reference's own classes
(tests/golden/head_ref.npz, made by tests/golden/gen_head_fixture.py) and, end to end with its gradients, against the
oracle's `decode`.  Tolerances:
  * against the fixture 1e-10 of each tensor's largest magnitude: two float64 evaluations of one formula differ by
    rounding order only;
  * against the oracle SDR >= 150 dB (float64 buys about 170 dB over the project's 110 dB float32 gate; a formula error
    shows at 90 dB or less) and gradients within 1e-9 of each tensor's largest;
  * the six dead tensors (athd/head.py) at most 1e-12 of the largest gradient of all.
"""
import os

import numpy as np
import pytest
import torch

import head_refs as H
from conftest import GOLDEN


@pytest.fixture(scope="module")
def head64(state_dict):
    from athd.head import TrainableHead
    head = TrainableHead().double()
    head.load_state_dict(H.head_state(state_dict), strict=True)
    return head


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "head_ref.npz")))


def _grads(head):
    return {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone()
            for k, p in head.named_parameters()}


def _dead_ok(grads, bound):
    largest = max(float(g.abs().max()) for g in grads.values())
    assert largest > 0
    for k in H.DEAD:
        assert float(grads[k].abs().max()) <= bound * largest, (k, float(grads[k].abs().max()), largest)
    for k in ("text_attn.attn.in_proj_weight", "text_attn.attn.in_proj_bias"):      # the query and key thirds
        assert float(grads[k][:768].abs().max()) <= bound * largest, k
    return largest


def test_keys_and_shapes():
    from athd.head import TrainableHead, head_keys
    from athd.weights import hot_path_spec
    want = {k: tuple(s) for k, s, _ in hot_path_spec() if not k.startswith("htdemucs.")}
    got = {k: tuple(v.shape) for k, v in TrainableHead().state_dict().items()}
    assert len(want) == 50 and got == want
    assert [k for k, _ in head_keys()] == [k for k in want]
    assert all(p.requires_grad for p in TrainableHead().parameters())


def test_against_reference_classes(head64, fixture):
    assert list(fixture["keys"]) == [k for k, _ in __import__("athd.head").head.head_keys()]
    f, text = H.seeded_features(), H.seeded_text()
    head64.zero_grad()
    outs = dict(zip(H.OUTPUTS, head64.branches(f, text)))
    for n in H.OUTPUTS:
        ref = fixture[n + "_f64"]
        got = outs[n].detach().numpy()
        assert got.shape == ref.shape, n
        gap = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"{n}: {gap:.3g} of the tensor max")
        assert gap <= 1e-10, (n, gap)
    H.branch_loss(outs["xd"], outs["xtd"]).backward()
    grads = _grads(head64)
    for i, k in enumerate(fixture["keys"]):
        gmax = float(fixture["gmax"][i])
        ref = fixture["g/" + k]
        got = H.strided(grads[k])
        assert got.shape == ref.shape, k
        if gmax == 0.0:
            continue                # a dead tensor: bounded below against the largest gradient of all
        assert abs(float(grads[k].abs().max()) - gmax) <= 1e-10 * gmax, k
        assert float(np.abs(got - ref).max()) <= 1e-10 * gmax, (k, float(np.abs(got - ref).max()) / gmax)
    _dead_ok(grads, 1e-12)


@pytest.mark.parametrize("B,T,seed0,prompt", [(2, 4096, 107, 1), (1, 9999, 6, 3)])
def test_whole_head_against_oracle(head64, oracle_model, state_dict, text_table, B, T, seed0, prompt):
    from athd.synth import synthetic_batch
    wav = torch.as_tensor(synthetic_batch(B, T, seed0=seed0))
    feats, dec_in = H.oracle_features(oracle_model, wav)
    text = torch.as_tensor(text_table[prompt:prompt + 1]).double().expand(B, -1)
    ref, _ = H.oracle_leaves(oracle_model, state_dict)
    with torch.no_grad():
        want = ref.decode(dec_in[0], dec_in[1], dec_in[2], text, dec_in[3], dec_in[4], T)
        got = head64(feats, text)
    assert got.shape == want.shape == (B, 2, T) and got.dtype == torch.float64
    s = H.sdr_db(want.numpy(), got.numpy())
    print(f"T={T}: head vs oracle decode {s:.1f} dB")
    assert s >= 150.0, s


def test_shapes_ragged_33297(head64):
    f, text = H.seeded_features(B=1, T=33297, seed=5), H.seeded_text(B=1)
    assert f.lengths == [33] * 4 and f.lengths_t == [33297, 8325, 2082, 521]
    with torch.no_grad():
        out = head64(f, text)
    assert out.shape == (1, 2, 33297) and bool(torch.isfinite(out).all())


def test_whole_head_gradients_against_oracle(head64, oracle_model, state_dict, text_table):
    from athd.synth import synthetic_batch
    B, T = 2, 4096
    wav = torch.as_tensor(synthetic_batch(B, T, seed0=107))
    target = 0.5 * torch.as_tensor(synthetic_batch(B, T, seed0=211)).double()
    feats, dec_in = H.oracle_features(oracle_model, wav)
    text = torch.as_tensor(text_table[:2]).double()
    loss_fn = lambda out: ((out - target) ** 2).mean()
    want, _ = H.oracle_grads(oracle_model, state_dict, dec_in, text, T, loss_fn)
    head64.zero_grad()
    loss_fn(head64(feats, text)).backward()
    got = _grads(head64)
    worst = 0.0
    for k, w in want.items():
        m = float(w.abs().max())
        if k in H.DEAD:
            continue
        assert m > 0, k
        gap = float((got[k] - w).abs().max()) / m
        worst = max(worst, gap)
        assert gap <= 1e-9, (k, gap)
    print(f"worst gradient gap {worst:.3g} of its tensor's max")
    _dead_ok(got, 1e-12)
    _dead_ok(want, 1e-12)
