"""Generator of tests/golden/head_ref.npz: the reference's own trainable classes (`TextCrossAttention`, `FreqDecoder`,
`TimeDecoder` of `ATHTDemucs_v2.py`, plus the two 1x1 output convolutions it builds in its constructor) with the head
tensors of `synthetic_state_dict(0)`, on the seeded random features of tests/head_refs.py (T = 4096, B = 2).  Run once
by hand on the CPU where the reference checkout is available; never run by a test:

    python tests/golden/gen_head_fixture.py --reference /path/to/reference/checkout

The reference module imports `demucs.htdemucs.HTDemucs` at its top; where demucs is not installed an empty stand-in
satisfies that import (transformers and einops must be installed).

The file holds data only.  For dtype d in (f64, f32):
  x_cond_d, xt_cond_d     text_attn(x_enc, xt_enc, text)
  xd_d, xtd_d             freq_out(freq_decoder(x_cond, skips, lengths)), time_out(time_decoder(xt_cond, ...))
For the loss mean(xd^2) + mean(xtd^2) in float64, per head tensor k (keys: the list of names):
  gmax (50,)              max |grad_k|
  g/<k>                   grad_k.ravel()[0::97]
and the reference's own float32-against-float64 gaps, each as a fraction of the float64 tensor's largest magnitude:
  gap_out (4,)            x_cond, xt_cond, xd, xtd
  gap_grad (50,)          per head tensor (0 where the float64 gradient is zero)
"""
import argparse
import importlib
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for p in (TESTS, REPO, os.path.join(REPO, "audio-to-sheet-music_amd")):
    sys.path.insert(0, p)


def import_reference(root: str):
    sys.path.insert(0, os.path.abspath(root))
    from transformers import ClapModel, ClapTextModelWithProjection, RobertaTokenizerFast  # noqa: F401
    try:
        importlib.import_module("demucs.htdemucs")
    except ImportError:
        for name in ("demucs", "demucs.htdemucs"):
            mod = types.ModuleType(name)
            mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = mod
        sys.modules["demucs.htdemucs"].HTDemucs = object
        sys.modules["demucs"].htdemucs = sys.modules["demucs.htdemucs"]
    return importlib.import_module("src.models.stem_separation.ATHTDemucs_v2")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="directory of the reference checkout (holds src/)")
    ap.add_argument("--out", default=os.path.join(HERE, "head_ref.npz"))
    args = ap.parse_args()
    ref = import_reference(args.reference)

    import head_refs as H
    from athd.head import head_keys
    from athd.weights import DEC_CH, synthetic_state_dict

    sd = synthetic_state_dict(0)
    keys = [k for k, _ in head_keys()]
    runs = {}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        mods = torch.nn.ModuleDict({
            "text_attn": ref.TextCrossAttention(384, 512, 8), "freq_decoder": ref.FreqDecoder(list(DEC_CH)),
            "time_decoder": ref.TimeDecoder(list(DEC_CH)), "freq_out": torch.nn.Conv2d(4, 2, 1),
            "time_out": torch.nn.Conv1d(4, 2, 1)}).to(dtype)
        assert sorted(mods.state_dict()) == sorted(keys), set(mods.state_dict()) ^ set(keys)
        mods.load_state_dict(H.head_state(sd, dtype), strict=True)
        f, text = H.seeded_features(dtype), H.seeded_text(dtype)
        x_cond, xt_cond = mods["text_attn"](f.x_enc, f.xt_enc, text)
        xd = mods["freq_out"](mods["freq_decoder"](x_cond, f.skips[::-1], f.lengths[::-1]))
        xtd = mods["time_out"](mods["time_decoder"](xt_cond, f.skips_t[::-1], f.lengths_t[::-1]))
        H.branch_loss(xd, xtd).backward()
        params = dict(mods.named_parameters())
        runs[tag] = ({"x_cond": x_cond, "xt_cond": xt_cond, "xd": xd, "xtd": xtd},
                     {k: (params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])) for k in keys})

    arrays = {"keys": np.array(keys)}
    o64, g64 = runs["f64"]
    o32, g32 = runs["f32"]
    for n in H.OUTPUTS:
        arrays[f"{n}_f64"] = o64[n].detach().numpy()
        arrays[f"{n}_f32"] = o32[n].detach().numpy()
    gap = lambda a, b: float((a.double() - b.double()).abs().max() / b.abs().max()) if float(b.abs().max()) > 0 else 0.0
    arrays["gap_out"] = np.array([gap(o32[n].detach(), o64[n].detach()) for n in H.OUTPUTS])
    arrays["gmax"] = np.array([float(g64[k].abs().max()) for k in keys])
    arrays["gap_grad"] = np.array([gap(g32[k], g64[k]) for k in keys])
    for k in keys:
        arrays["g/" + k] = H.strided(g64[k])
    np.savez(args.out, **arrays)
    live = [i for i, k in enumerate(keys) if k not in H.DEAD]
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes; forward gaps {arrays['gap_out']}, "
          f"worst live gradient gap {arrays['gap_grad'][live].max():.3g}, largest |g| {arrays['gmax'].max():.3g}, "
          f"largest dead |g| {max(arrays['gmax'][keys.index(k)] for k in H.DEAD):.3g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
