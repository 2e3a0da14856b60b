"""Generator of tests/golden/evalspec_ref.npz: the reference's own `utils.compute_spectrogram` (its defaults: power 2,
dB, top_db 80) on two seeded inputs of tests/evalspec_refs.py, T = 5000, stereo.  Run once by hand where the reference
checkout, matplotlib and yaml are available; never run by a test:

    python tests/golden/gen_evalspec_fixture.py --reference /path/to/reference/checkout

The file holds data only: `{kind}_input` (2, 5000) float32 and `{kind}_spec` (1025, 10) float32 for kind in
randn, tone.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

KINDS = ("randn", "tone")
T, C = 5000, 2


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="directory of the reference checkout (holds utils.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "evalspec_ref.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    import utils as reference_utils        # the reference's module, not athd.utils

    import evalspec_refs as E
    arrays = {}
    for kind in KINDS:
        x = E.make_input(kind, T, C)
        spec = reference_utils.compute_spectrogram(x)
        assert tuple(spec.shape) == (1025, E.frames(T))
        arrays[f"{kind}_input"] = x.numpy()
        arrays[f"{kind}_spec"] = spec.numpy().astype(np.float32)
    np.savez(args.out, **arrays)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
