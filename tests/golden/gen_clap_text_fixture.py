"""Writes tests/golden/clap_text_ref.npz: transformers' ClapTextModelWithProjection (fp32, CPU) on the synthetic tower
weights (athd.weights.synthetic_clap_text_state_dict(SEED), regenerated from the seed, never stored) for the cases of
tests/clap_text_refs.py - per case `<name>_ids`, `<name>_mask`, `<name>_text_embeds` - and the transformers / torch
versions it ran with.

    python tests/golden/gen_clap_text_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "audio-to-sheet-music_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import transformers

    import clap_text_refs as R
    from athd.weights import synthetic_clap_text_state_dict
    sd = synthetic_clap_text_state_dict(R.SEED)
    model = R.hf_model(sd)
    out = {"transformers_version": np.array(transformers.__version__), "torch_version": np.array(torch.__version__),
           "seed": np.array(R.SEED)}
    for name, (ids, mask) in R.CASES.items():
        emb = R.hf_forward(model, ids, mask).numpy()
        assert emb.dtype == np.float32 and emb.shape == (ids.shape[0], R.PROJ)
        out[name + "_ids"] = ids.astype(np.int32)
        out[name + "_mask"] = mask.astype(np.int32)
        out[name + "_text_embeds"] = emb
    path = os.path.join(HERE, "clap_text_ref.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
