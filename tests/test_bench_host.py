"""Host-side pieces of bench.py (CPU): the bench batch generated on several cores equals the serial
`athd.synth.synthetic_batch`, `--dump-outputs` writes a reproducible float32 sample within its size limit, and the
`--full`-only options are refused in a plain run."""
import numpy as np
import pytest
import torch

import bench


def test_bench_batch_equals_synthetic_batch():
    from athd.synth import synthetic_batch
    got = bench.bench_batch(3, 1000)
    assert got.dtype == np.float32 and got.shape == (3, 2, bench.SEG)
    assert np.array_equal(got, synthetic_batch(3, bench.SEG, seed0=1000))


def test_dump_outputs_rows_and_seeded_sample(tmp_path):
    out = torch.randn((5, 4, 2, 1000), generator=torch.Generator().manual_seed(3))
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out.clone())
    rows = np.load(tmp_path / "a" / "stems_rows.npy")
    sample = np.load(tmp_path / "a" / "stems_sample.npy")
    assert rows.dtype == sample.dtype == np.float32
    assert np.array_equal(rows, out[[0, 2, 4]].numpy())
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, out.numel(), size=out.numel()))
    assert np.array_equal(sample, out.reshape(-1).numpy()[idx])
    for n in ("stems_rows.npy", "stems_sample.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    # the bench shape: 3 whole segments x 4 stems + the sample stay far below the 64 MB limit
    assert 4 * (3 * 4 * 2 * bench.SEG + bench.DUMP_SAMPLE) < 64e6


def test_full_only_options_are_refused_in_a_plain_run(capsys):
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", "d"])
    assert (plain.steps, plain.warmup, plain.full, plain.dump_outputs) == (7, 3, False, "d")
    for extra in (["--dump-kernels", "k.json"], ["--segments", "8"], ["--kernel", "attn32_kernel@transformer"]):
        with pytest.raises(SystemExit):
            bench.parse_args(["--gpus", "1", *extra])
        assert "--full" in capsys.readouterr().err
        assert bench.parse_args(["--full", *extra]).full
