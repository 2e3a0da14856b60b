"""The float64 restatement of the evaluation spectrogram (tests/evalspec_refs.py) against recorded outputs of the
reference's own `utils.compute_spectrogram` (tests/golden/evalspec_ref.npz, made by tests/golden/
gen_evalspec_fixture.py): the restatement the GPU tests compare against is the reference's function.  CPU only.

TOL = 4 x r, r = 1.84e-7: the largest |X32 - X64| / den of torch's own fp32 Hann stft against its float64 stft,
measured on the CPU over the inputs of these tests and of tests/test_gpu_evalspec.py (four kinds, T in {1025, 2048,
5000, 20000}, mono and stereo, seeds 0..2: randn 0.98e-7 .. 1.46e-7, tone 0.77e-7 .. 1.72e-7, quiet 0.91e-7 ..
1.84e-7, late 1.05e-7 .. 1.57e-7; `evalspec_refs.stft_error_ratio`).  The factor 4 is what tests/test_gpu_audio.py
allows a different FFT factorisation.
"""
import os

import numpy as np
import pytest
import torch

import evalspec_refs as E
from conftest import GOLDEN

TOL = E.TOL


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "evalspec_ref.npz"))


@pytest.mark.parametrize("kind,wide_db", [("randn", 0.1), ("tone", 1.0)])
def test_restatement_reproduces_the_reference(fixture, kind, wide_db):
    x = torch.from_numpy(fixture[f"{kind}_input"])
    assert torch.equal(x, E.make_input(kind, 5000, 2)), "the fixture's input is the seeded input of evalspec_refs"
    got = torch.from_numpy(fixture[f"{kind}_spec"])
    X, norm, final = E.spectrogram_ref(x, 2.0, True, 80.0)
    E.check_db(got, X, norm, TOL, 2.0, 80.0, wide_db, f"reference {kind}")
    # the restatement itself lies in its own interval
    E.check_db(final, X, norm, TOL, 2.0, 80.0, wide_db, f"restatement {kind}")
    if kind == "tone":
        assert (got == got.min()).double().mean().item() > 0.5       # most bins sit on the top_db floor

