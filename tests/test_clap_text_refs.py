"""The CLAP text tower's references on the CPU (tests/clap_text_refs.py): the float64 restatement against the recorded
transformers outputs (tests/golden/clap_text_ref.npz, written by tests/golden/gen_clap_text_fixture.py) and against
live transformers where it imports, its padding invariance, its sensitivity to the mask, and the two constants the GPU
test (tests/test_gpu_clap_text.py) builds its tolerances from:

  R32 = 2.0e-6: err(transformers fp32 forward, float64 restatement), measured per case 5.0e-7 .. 1.59e-6
  RBF = 1.4e-2: err(bf16 emulation, float64 restatement), measured per case 8.7e-3 .. 1.373e-2 (cosine >= 0.99989)

Both are asserted here over the cases, from above and (so that a constant cannot be left far too wide) from below.
"""
import os

import numpy as np
import pytest
import torch

import clap_text_refs as R
from conftest import GOLDEN


@pytest.fixture(scope="module")
def sd():
    from athd.weights import synthetic_clap_text_state_dict
    return synthetic_clap_text_state_dict(R.SEED)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "clap_text_ref.npz"))


@pytest.fixture(scope="module")
def ref64(sd):
    return {n: R.restatement(sd, ids, mask) for n, (ids, mask) in R.CASES.items()}


def test_synthetic_weights_are_the_contract(sd):
    from athd import native
    from athd.weights import clap_text_spec, synthetic_clap_text_state_dict
    assert len(sd) == 203 and list(sd) == native.text_required_keys() == [k for k, _, _ in clap_text_spec()]
    assert all(v.dtype == np.float32 and v.shape == tuple(s) for v, (_, s, _) in zip(sd.values(), clap_text_spec()))
    q = sd["text_model.encoder.layer.0.attention.self.query.weight"]
    v = sd["text_model.encoder.layer.0.attention.self.value.weight"]
    assert abs(q.std() * np.sqrt(768) - 2.0) < 0.02 and abs(v.std() * np.sqrt(768) - 1.0) < 0.01
    again = synthetic_clap_text_state_dict(R.SEED)
    assert all(np.array_equal(sd[k], again[k]) for k in ("text_projection.linear2.weight",
                                                         "text_model.embeddings.position_embeddings.weight"))


def test_fixture_holds_the_cases(golden):
    for n, (ids, mask) in R.CASES.items():
        assert np.array_equal(golden[n + "_ids"], ids) and np.array_equal(golden[n + "_mask"], mask), n
        assert golden[n + "_text_embeds"].shape == (ids.shape[0], 512)
    assert int(golden["seed"]) == R.SEED
    assert {k: v[0].shape for k, v in R.CASES.items()} == {"bos_eos": (1, 2), "ragged9": (4, 9), "ragged17": (4, 17),
                                                           "ragged33": (4, 33), "one16": (1, 16), "five17": (5, 17),
                                                           "long128": (1, 128)}


def test_restatement_matches_the_fixture_within_r32(golden, ref64):
    worst = 0.0
    for n in R.CASES:
        e = R.err(golden[n + "_text_embeds"], ref64[n])
        print(f"r32 {n}: {e:.3e}")
        worst = max(worst, e)
    assert R.R32 / 2 <= worst <= R.R32, worst


def test_restatement_matches_live_transformers(sd, ref64):
    pytest.importorskip("transformers")          # the fixture is the pin; this repeats it on the installed version
    model = R.hf_model(sd)
    for n in ("ragged9", "five17"):
        e = R.err(R.hf_forward(model, *R.CASES[n]), ref64[n])
        print(f"live {n}: {e:.3e}")
        assert e <= R.R32, (n, e)


def test_bf16_emulation_constant(sd, ref64):
    worst, cos = 0.0, 1.0
    for n, (ids, mask) in R.CASES.items():
        bf = R.restatement(sd, ids, mask, bf16=True)
        e = R.err(bf, ref64[n])
        c = float(torch.nn.functional.cosine_similarity(bf, ref64[n], dim=1).min())
        print(f"rbf {n}: {e:.3e} cosine {c:.6f}")
        worst, cos = max(worst, e), min(cos, c)
    assert R.RBF / 2 <= worst <= R.RBF, worst
    assert cos >= 0.9998, cos


def test_padding_changes_nothing_and_the_mask_matters(sd, ref64):
    assert torch.equal(ref64["ragged9"], ref64["ragged17"]) and torch.equal(ref64["ragged9"], ref64["ragged33"])
    for n in ("ragged9", "ragged17", "ragged33"):
        ids, mask = R.CASES[n]
        nomask = R.restatement(sd, ids, mask, use_mask=False)
        per_prompt = ((nomask - ref64[n]).abs().amax(dim=1) / ref64[n].abs().amax(dim=1)).tolist()
        print(f"no mask {n}: {per_prompt}")
        padded = [i for i in range(ids.shape[0]) if (ids[i] == R.PAD).any()]
        assert padded and all(per_prompt[i] > 0.1 for i in padded), per_prompt
        assert all(per_prompt[i] == 0.0 for i in range(ids.shape[0]) if i not in padded)


def test_normalize_branch(sd, ref64):
    ids, mask = R.CASES["ragged9"]
    n = R.restatement(sd, ids, mask, normalize=True)
    assert torch.allclose(n.norm(dim=1), torch.ones(4, dtype=torch.float64), atol=1e-14)
    assert torch.allclose(n * ref64["ragged9"].norm(dim=1, keepdim=True), ref64["ragged9"], atol=1e-14)
