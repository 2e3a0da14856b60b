"""Generator of tests/golden/loss_ref.npz: the reference's own `src/loss.py` functions and its own `validate`
(`src/train.py:132-202`) on the seeded inputs of tests/validate_refs.py.  Run once by hand where the reference checkout
is available; never run by a test:

    python tests/golden/gen_loss_fixture.py --reference /path/to/reference/checkout

`validate` needs only torch at run time; modules that `src/train.py` imports at its top and that are not installed
(demucs, stempeg, soundfile, ...) are satisfied by empty stand-ins, as oracle/gen_golden.py does for the model.

The file holds data only:
  loss_est, loss_target (5, 2, 750) float32          one row per SNR 25, 10, 0, -10, -25 dB
  sdr_loss_rows, sisdr_loss_rows (5,), *_batch ()     each function on est[i:i+1] and on the whole batch
  new_sdr_rows (5,), new_sdr_batch (5,)
  combined_rows (5, 7), combined_batch (7,)           [total, then the metric dict in the order of combined_keys]
  combined_l1_rows (5, 6), combined_l1_batch (6,)     likewise with combined_l1_keys
  val_mixture, val_target, val_noise (16, 2, 256) float32, val_stems (16,)
  validate_{cmb,l1}_keys, validate_{cmb,l1}_vals      the dict `validate` returned for either loss choice
                                                      (batch_size 3; l1: l1_sdr_weight 1.0, l1_weight 0.05)
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
sys.path.insert(0, os.path.dirname(HERE))


def _stand_in(name: str, **attrs):
    try:
        importlib.import_module(name)
    except ImportError:
        mod = types.ModuleType(name)
        mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
        if "." in name:
            setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], mod)


def import_reference(root: str):
    """(src.loss, src.train) of the reference checkout at `root`."""
    sys.path.insert(0, os.path.abspath(root))
    from transformers import ClapModel, ClapTextModelWithProjection  # noqa: F401  (resolved before the stand-ins exist)
    _stand_in("demucs")
    _stand_in("demucs.pretrained")
    _stand_in("demucs.htdemucs", HTDemucs=type("HTDemucs", (torch.nn.Module,), {}))
    _stand_in("stempeg")
    _stand_in("soundfile")
    return importlib.import_module("src.loss"), importlib.import_module("src.train")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="directory of the reference checkout (holds src/)")
    ap.add_argument("--out", default=os.path.join(HERE, "loss_ref.npz"))
    args = ap.parse_args()
    ref_loss, ref_train = import_reference(args.reference)

    import validate_refs as V
    est, tgt = V.loss_fixture_inputs()
    arrays = {"loss_est": est.numpy(), "loss_target": tgt.numpy()}
    n = est.shape[0]

    def both(fn):
        return [fn(est[i:i + 1], tgt[i:i + 1]) for i in range(n)], fn(est, tgt)

    for name in ("sdr_loss", "sisdr_loss"):
        rows, batch = both(getattr(ref_loss, name))
        arrays[f"{name}_rows"] = np.array([float(v) for v in rows])
        arrays[f"{name}_batch"] = np.array(float(batch))
    rows, batch = both(ref_loss.new_sdr_metric)
    arrays["new_sdr_rows"] = np.array([float(v[0]) for v in rows])
    arrays["new_sdr_batch"] = batch.double().numpy()
    for name, fn, keys in (("combined", ref_loss.combined_loss, V.COMBINED_KEYS),
                           ("combined_l1", ref_loss.combined_L1_sdr_loss, V.COMBINED_L1_KEYS)):
        rows, batch = both(fn)
        for _, metrics in rows + [batch]:
            assert tuple(metrics) == tuple(keys), tuple(metrics)
        flat = lambda r: [float(r[0])] + [float(r[1][k]) for k in keys]
        arrays[f"{name}_keys"] = np.array(keys)
        arrays[f"{name}_rows"] = np.array([flat(r) for r in rows])
        arrays[f"{name}_batch"] = np.array(flat(batch))

    mixture, target, noise, stems = V.validate_fixture_inputs()
    arrays.update(val_mixture=mixture.numpy(), val_target=target.numpy(), val_noise=noise.numpy(),
                  val_stems=np.array(stems))
    batches = V.make_batches(mixture, target, stems, V.VAL_BATCH)
    assert len(batches) == 6 and len(batches[-1]["prompt"]) == 1
    for tag, kw in (("cmb", dict(use_L1_cmb_loss=False, l1_sdr_weight=None, l1_weight=None)),
                    ("l1", dict(use_L1_cmb_loss=True, l1_sdr_weight=1.0, l1_weight=0.05))):
        got = ref_train.validate(V.StubModel(noise), batches, "cpu", False, **kw)
        arrays[f"validate_{tag}_keys"] = np.array(list(got))
        arrays[f"validate_{tag}_vals"] = np.array([float(v) for v in got.values()])
    np.savez(args.out, **arrays)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
