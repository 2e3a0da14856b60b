"""CPU side of the embedding-comparison twin: the float64 restatement of tests/embedding_refs.py against what the
reference's own functions returned (tests/golden/embedding_ref.npz), and the host pieces of athd/embedding_comparison.py.

  1. `a_sim`, `a_dist`: the largest |reference - restatement| over the recorded cases.  The reference's similarity is a
     float32 BLAS product of unit rows, d <= 512 terms of magnitude <= 1 each rounded at 2^-24: a few 1e-7 (bound asserted:
     2e-6, the worst case sqrt(d) 2^-24 with a factor 1.5); its distance is computed in float64 and rounded once to
     float32 at values <= 2: <= 2^-23 = 1.2e-7 (asserted).  Measured: a_sim 7.2e-07, a_dist 9.8e-08 (scikit-learn 1.7.2);
     DESIGN.md §0 carries the same two figures and this file checks that it does.
  2. the normalised rows: numpy's float32 norm (pairwise float32 sum of squares, <= log2(512) + 2 roundings) against the
     float64-accumulated one moves the float32 quotient by at most 4 ulp (measured: 2).
  3. `analyze_clustering`: the reference averages float32 values in float32 (np.mean / np.std of a float32 array,
     pairwise: <= log2(8515) 2^-24 ~ 8e-7 relative to values <= 1), so its five numbers are within 2e-6 of the float64
     statistics of its own matrix; NaN exactly where a class is empty.
  4. the prompt collection, the Word2Vec averaging, `convert_to_native_types`, the JSON layout, `category_ids`.
"""
import json
import os
import re

import numpy as np
import pytest

import embedding_refs as E
from conftest import PKG, REPO

F32_MEAN_TOL = 2e-6


def _names():
    return [str(s) for s in E.fixture()["case_names"]]


def test_fixture_holds_the_seeded_cases():
    from athd.embedding_comparison import TILE
    f = E.fixture()
    assert int(f["tile"]) == TILE
    cases = dict(E.recorded_cases(TILE))
    cases["prompts18"] = E.prompt_case(list(f["prompts"]), list(f["categories"]))
    assert _names() == list(cases)
    for name, (table, cats) in cases.items():
        assert np.array_equal(f[f"{name}_input"], table), name
        assert [str(c) for c in f[f"{name}_categories"]] == [str(c) for c in cats], name
        n = len(table)
        assert f[f"{name}_similarity"].shape == (n, n) and f[f"{name}_distance"].shape == (n, n)
    ns = {len(c[0]) for c in cases.values()}
    ds = {c[0].shape[1] for c in cases.values()}
    assert {1, 2, TILE, TILE + 1, 2 * TILE + 3} <= ns and {1, 7, 300, 512} <= ds


def test_tile_constant_matches_the_kernel():
    from athd.embedding_comparison import TILE
    src = open(os.path.join(PKG, "csrc", "embed_compare.hip")).read()
    assert int(re.search(r"constexpr int EC_TILE = (\d+);", src).group(1)) == TILE


def test_reference_gap_to_the_restatement():
    a_sim, a_dist, per = E.reference_gaps()
    for name, (s, d) in per.items():
        print(f"{name}: a_sim {s:.3e} a_dist {d:.3e}")
    print(f"a_sim {a_sim:.1e} a_dist {a_dist:.1e}")
    assert 0.0 < a_sim <= 2e-6 and 0.0 < a_dist <= 2.0 ** -23
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert f"a_sim = {a_sim:.1e}" in design and f"a_dist = {a_dist:.1e}" in design


def test_restatement_structure():
    f = E.fixture()
    for name in _names():
        r = E.restatement(f[f"{name}_input"], list(f[f"{name}_categories"]))
        sim, dist = r["similarity"], r["distance"]
        assert np.array_equal(sim, sim.T) and np.array_equal(dist, dist.T) and not dist.diagonal().any()
        zero = ~f[f"{name}_input"].any(axis=1)
        assert not r["normed"][zero].any() and not sim[zero].any() and not sim[:, zero].any()
        assert np.all(np.abs(sim.diagonal()[~zero] - 1.0) <= 2.0 ** -52 * 4)


def test_normalisation_against_the_reference():
    f = E.fixture()
    worst = 0.0
    for name in _names():
        got, want = E.normalize_rows(f[f"{name}_input"]), f[f"{name}_normed"]
        worst = max(worst, float((np.abs(got.astype(np.float64) - want) / E.ulp32(want)).max()))
    print(f"normalised rows: worst {worst:.2f} ulp")
    assert worst <= 4.0


def test_analysis_against_the_reference():
    f = E.fixture()
    a_sim = E.reference_gaps()[0]
    for name in _names():
        cats = list(f[f"{name}_categories"])
        want = f[f"{name}_analysis"]
        own = E.stats_of(f[f"{name}_similarity"], cats)                       # float64 statistics of ITS matrix
        full = E.restatement(f[f"{name}_input"], cats)["stats"]               # the whole chain restated
        assert np.array_equal(np.isnan(want), np.isnan(own[:5])) and np.array_equal(np.isnan(want), np.isnan(full[:5]))
        ok = ~np.isnan(want)
        assert np.all(np.abs(own[:5] - want)[ok] <= F32_MEAN_TOL * np.array([1, 1, 1, 1, 2])[ok]), name
        assert np.all(np.abs(full[:5] - want)[ok] <=
                      (F32_MEAN_TOL + E.allowance(a_sim)) * np.array([1, 1, 1, 1, 2])[ok]), name
        n = len(cats)
        assert own[5] + own[6] == n * (n - 1) // 2 and own[7] == 0.0
    one, distinct, single = (E.stats_of(f[f"{k}_similarity"], list(f[f"{k}_categories"]))
                             for k in ("one_category", "all_distinct", "n1_d512"))
    assert one[6] == 0 and np.isnan(one[[2, 3, 4]]).all() and not np.isnan(one[[0, 1]]).any()
    assert distinct[5] == 0 and np.isnan(distinct[[0, 1, 4]]).all() and not np.isnan(distinct[[2, 3]]).any()
    assert np.isnan(single[:5]).all() and single[5] == single[6] == 0
    equal = E.restatement(f["all_equal_input"], list(f["all_equal_categories"]))["stats"]
    assert equal[1] <= 1e-12 and equal[3] <= 1e-12


def test_collect_all_prompts():
    from athd.embedding_comparison import category_ids, collect_all_prompts
    f = E.fixture()
    prompts, categories = collect_all_prompts()
    assert prompts == [str(p) for p in f["prompts"]] and categories == [str(c) for c in f["categories"]]
    assert len(prompts) == E.N_PROMPTS and len(set(categories)) == E.N_CATEGORIES
    ids = category_ids(categories)
    assert ids.dtype == np.int32 and ids.tolist() == [0] * 4 + [1] * 4 + [2] * 3 + [3] * 4 + [4] * 3
    assert category_ids(["b", "a", "b", 7, "a"]).tolist() == [0, 1, 0, 2, 1]


def test_word2vec_rows(capsys):
    from athd.embedding_comparison import EmbeddingExtractor
    f = E.fixture()
    model = E.word2vec_model()
    assert list(model) == [str(w) for w in f["w2v_words"]] and np.array_equal(np.stack(list(model.values())),
                                                                              f["w2v_vectors"])
    ex = EmbeddingExtractor(word2vec_model=model)
    rows, valid = ex.word2vec_rows([str(p) for p in f["prompts"]])
    assert "Warning: Could not embed 'viola'" in capsys.readouterr().out
    assert valid == [str(p) for p in f["w2v_valid"]] and "viola" not in valid and rows.dtype == np.float32
    got, want = E.normalize_rows(rows), f["w2v_embeddings"]
    assert got.shape == want.shape == (E.N_PROMPTS - 1, E.W2V_DIM)
    assert (np.abs(got.astype(np.float64) - want) / E.ulp32(want)).max() <= 4.0
    with pytest.raises(ValueError, match="No valid embeddings"):
        ex.word2vec_rows(["viola", "zither"])
    with pytest.raises(RuntimeError, match="word2vec_model="):
        EmbeddingExtractor().word2vec_rows(["drums"])


def test_word2vec_npz_round_trip(tmp_path):
    from athd.embedding_comparison import load_word2vec_npz
    model = E.word2vec_model()
    np.savez(tmp_path / "w2v.npz", words=np.array(list(model)), vectors=np.stack(list(model.values())))
    back = load_word2vec_npz(tmp_path / "w2v.npz")
    assert list(back) == list(model) and all(np.array_equal(back[w], model[w]) for w in model)
    assert "drums" in back and "viola" not in back


def test_convert_to_native_types_and_json_layout():
    from athd.embedding_comparison import STATS, build_results, convert_to_native_types
    got = convert_to_native_types({"a": np.float32(1.5), "b": [np.int64(3), (np.float64(2.0), "s")],
                                   "c": np.arange(3, dtype=np.int32), "d": None, "e": {"f": np.bool_(True)}})
    assert got == {"a": 1.5, "b": [3, (2.0, "s")], "c": [0, 1, 2], "d": None, "e": {"f": np.bool_(True)}}
    assert type(got["a"]) is float and type(got["b"][0]) is int and type(got["b"][1]) is tuple
    assert type(got["c"]) is list and type(got["c"][0]) is int
    assert STATS == E.STAT_KEYS
    analysis = {k: np.float64(i) for i, k in enumerate(STATS)}
    res = build_results((18, 512), analysis, ["p"], ["c"], (17, 300), dict(analysis), ["p"])
    back = json.loads(json.dumps(res, indent=2))
    assert list(back) == ["clap", "word2vec", "prompts", "categories"]
    assert list(back["clap"]) == ["embeddings_shape", "analysis"] and back["clap"]["embeddings_shape"] == [18, 512]
    assert list(back["word2vec"]) == ["embeddings_shape", "analysis", "valid_prompts"]
    assert list(back["clap"]["analysis"]) == list(STATS)
    none = build_results((18, 512), analysis, ["p"], ["c"])
    assert none["word2vec"] == {"embeddings_shape": None, "analysis": None, "valid_prompts": None}


def test_reduce_dimensions_host_route():
    from athd.embedding_comparison import reduce_dimensions
    with pytest.raises(ValueError, match="Unknown method"):
        reduce_dimensions(np.zeros((4, 8), np.float32), method="mds")
    x = np.random.default_rng(0).standard_normal((12, 16)).astype(np.float32)
    try:
        import sklearn  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="scikit-learn"):
            reduce_dimensions(x, method="pca")
        return
    assert reduce_dimensions(x, method="pca").shape == (12, 2)


def test_compare_has_no_cpu_path():
    import torch

    from athd.embedding_comparison import compare
    with pytest.raises(ValueError, match="HIP device"):
        compare(torch.zeros(2, 4))
