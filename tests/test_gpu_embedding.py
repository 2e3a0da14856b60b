"""The embedding-comparison twin on the GPU: `athd_embed_compare` and athd/embedding_comparison.py against the float64
restatement of tests/embedding_refs.py.

Allowances (none of them taken from the code under test):
  normed      2 float32 ulp per element of the restatement's value (the norm's fp64 sum has another order on the device:
              its float32 rounding can flip, which moves the quotient by one ulp, plus the quotient's own rounding)
  sim, dist   max(4 a, 2^-23) with a = the reference's own gap to the restatement on the recorded cases
              (tests/golden/embedding_ref.npz; a_sim 7.2e-07, a_dist 9.8e-08), embedding_refs.allowance
  stats       means and stds within the sim allowance, the separation within twice it (a mean and a population std move
              by at most the largest element change); 1e-12 against float64 statistics of the matrix the routine returned
Shapes: t = TILE; n = 1, 2, t, t + 1, 2 t + 3 and the limit 4096 (2080 tiles: more partials than the threads that add
them); d = 1, 7, 300, 512 and the limit 4096 (every register group of the row pass).  Every case contiguous and aligned,
and again with row_stride = d + 5 from a base one float into its allocation (no row group is 16-byte aligned
throughout: the scalar route), with NaNs in the gaps between rows.  Every raw call runs with guard elements around each
buffer.
"""
import json
import zlib

import numpy as np
import pytest
import torch

import embedding_refs as E

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -5
GUARD = 64
SENTINEL = -12345.5


def _mod():
    import athd.embedding_comparison as M
    return M


def _lib():
    from athd import native
    return native.lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """a device buffer of `count` elements with GUARD sentinel elements on either side"""

    def __init__(self, count, dtype=torch.float32):
        self.full = torch.full((count + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.count = count

    @property
    def view(self):
        return self.full[GUARD:GUARD + self.count]

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        return bool(torch.all(self.full[:GUARD] == SENTINEL)) and bool(torch.all(self.full[GUARD + self.count:] == SENTINEL))

    def untouched(self):
        return bool(torch.all(self.full == SENTINEL))


def _place(table: np.ndarray, strided: bool):
    """(device tensor holding the rows, pointer to row 0, row_stride).  strided: rows d + 5 apart from one float into
    the allocation, NaN between the rows."""
    n, d = table.shape
    if not strided:
        t = torch.from_numpy(table).cuda().contiguous()
        assert t.data_ptr() % 16 == 0
        return t, t.data_ptr(), d
    stride = d + 5
    buf = torch.full((n * stride + 8,), float("nan"), dtype=torch.float32, device="cuda")
    rows = buf[1:1 + n * stride].view(n, stride)
    rows[:, :d] = torch.from_numpy(table).cuda()
    assert rows.data_ptr() % 16 == 4
    return buf, rows.data_ptr(), stride


def raw_call(table, cats, strided=False, want=("normed", "sim", "dist", "stats")):
    """athd_embed_compare with guards around every buffer -> (rc, {name: numpy array})"""
    lib = _lib()
    n, d = table.shape
    keep, emb_ptr, stride = _place(table, strided)
    cat = torch.from_numpy(np.asarray(cats, dtype=np.int64).astype(np.int32)).cuda() if cats is not None else None
    need = lib.athd_embed_compare_scratch_bytes(n, d)
    assert need > 0 and need % 4 == 0
    bufs = {"normed": Guarded(n * d), "sim": Guarded(n * n), "dist": Guarded(n * n),
            "stats": Guarded(8, torch.float64)}
    scratch = Guarded((need + 7) // 8, torch.float64)
    p = lambda k: bufs[k].ptr() if k in want else None
    rc = lib.athd_embed_compare(emb_ptr, n, d, stride, cat.data_ptr() if cat is not None else None, p("normed"),
                                p("sim"), p("dist"), p("stats"), scratch.ptr(), need, _stream())
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.guards_intact(), f"guard elements around {k} were written"
        if k not in want:
            assert b.untouched(), f"{k} was not asked for and was written"
    assert scratch.guards_intact(), "guard elements around the scratch were written"
    shapes = {"normed": (n, d), "sim": (n, n), "dist": (n, n), "stats": (8,)}
    return rc, {k: bufs[k].view.cpu().numpy().reshape(shapes[k]).copy() for k in want}


# ------------------------------------------------------------------------------------------------------------ cases
def _all_cases():
    M = _mod()
    cases = dict(E.recorded_cases(M.TILE))
    cases.update(E.gpu_only_cases(M.TILE))
    prompts, categories = M.collect_all_prompts()
    table, cats = E.prompt_case(prompts, categories)
    cases["prompts18"] = (table, M.category_ids(cats))
    return cases


CASE_NAMES = ["n1_d512", "n2_d7", "nt_d300", "nt1_d1", "n2t3_d40", "zero_row", "parallel_duplicate", "one_category",
              "all_distinct", "odd_ids", "all_equal", "n2t3_d512", "n2t3_d300", "n3_d4096", "n4096_d3", "prompts18"]
_refs = {}


def _case(name):
    """(table, cats, restatement) - the restatement computed once per case and left unchanged"""
    if name not in _refs:
        table, cats = _all_cases()[name]
        _refs[name] = (table, np.asarray(cats), E.restatement(table, list(cats)))
    return _refs[name]


@pytest.fixture(scope="module")
def allow():
    a_sim, a_dist, _ = E.reference_gaps()
    return E.allowance(a_sim), E.allowance(a_dist)


def test_case_list_is_complete():
    M = _mod()
    assert sorted(CASE_NAMES) == sorted(_all_cases())
    t = M.TILE
    assert {len(_case(k)[0]) for k in CASE_NAMES} >= {1, 2, t, t + 1, 2 * t + 3}
    assert {_case(k)[0].shape[1] for k in CASE_NAMES} >= {1, 7, 300, 512}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(name, got, allow):
    table, cats, want = _case(name)
    a_sim, a_dist = allow
    n = len(table)
    zero = ~table.any(axis=1)
    normed, sim, dist, stats = got["normed"], got["sim"], got["dist"], got["stats"]
    # normed
    ulps = float((np.abs(normed.astype(np.float64) - want["normed"]) / E.ulp32(want["normed"])).max())
    e_sim = float(np.abs(sim.astype(np.float64) - want["similarity"]).max())
    e_dist = float(np.abs(dist.astype(np.float64) - want["distance"]).max())
    print(f"{name}: normed {ulps:.2f} ulp (<= 2), sim {e_sim:.3e} (<= {a_sim:.3e}), dist {e_dist:.3e} (<= {a_dist:.3e})")
    assert np.isfinite(normed).all() and np.isfinite(sim).all() and np.isfinite(dist).all()
    assert ulps <= 2.0
    assert not normed[zero].any()
    # matrices
    assert e_sim <= a_sim and e_dist <= a_dist
    assert np.array_equal(_bits(sim), _bits(sim.T)) and np.array_equal(_bits(dist), _bits(dist.T))
    assert not dist.diagonal().any()
    assert np.all(np.abs(sim.diagonal()[~zero].astype(np.float64) - 1.0) <= 2.0 ** -23)
    assert not sim[zero].any() and not sim[:, zero].any()
    # statistics
    host = E.stats_of(sim, list(cats))
    ref = want["stats"]
    print(f"{name}: stats {stats.tolist()} (host {np.abs(stats[:5] - host[:5]).tolist()})")
    assert stats[5] == ref[5] == host[5] and stats[6] == ref[6] == host[6] and stats[7] == 0.0
    assert stats[5] + stats[6] == n * (n - 1) // 2
    assert np.array_equal(np.isnan(stats), np.isnan(ref)), (stats, ref)
    assert np.array_equal(np.isnan(stats[:5]), [ref[5] == 0, ref[5] == 0, ref[6] == 0, ref[6] == 0,
                                                ref[5] == 0 or ref[6] == 0])
    ok = ~np.isnan(ref[:5])
    assert np.all(np.abs(stats[:5] - host[:5])[ok] <= 1e-12), (stats, host)
    assert np.all(np.abs(stats[:5] - ref[:5])[ok] <= (a_sim * np.array([1, 1, 1, 1, 2]))[ok]), (stats, ref)


@pytest.mark.parametrize("strided", [False, True], ids=["aligned", "stride_d5_unaligned"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_matches_restatement(name, strided, allow):
    table, cats, _ = _case(name)
    rc, got = raw_call(table, cats, strided=strided)
    assert rc == 0
    _check(name, got, allow)


def test_parallel_and_duplicate_rows(allow):
    table, cats, _ = _case("parallel_duplicate")
    rc, got = raw_call(table, cats)
    assert rc == 0
    assert abs(float(got["sim"][1, 3]) - 1.0) <= allow[0] and float(got["dist"][1, 3]) <= allow[1]
    assert np.array_equal(_bits(got["normed"][0]), _bits(got["normed"][4]))
    assert got["dist"][0, 4] == 0.0 and abs(float(got["sim"][0, 4]) - 1.0) <= 2.0 ** -23
    assert np.array_equal(_bits(got["sim"][0, [1, 2, 3, 5]]), _bits(got["sim"][4, [1, 2, 3, 5]]))


def test_all_rows_equal_have_zero_spread():
    table, cats, _ = _case("all_equal")
    for strided in (False, True):
        rc, got = raw_call(table, cats, strided=strided)
        assert rc == 0
        off = got["sim"][~np.eye(len(table), dtype=bool)]
        assert np.all(off == off[0])
        assert got["stats"][1] <= 1e-12 and got["stats"][3] <= 1e-12, got["stats"]


@pytest.mark.parametrize("name", ["n2t3_d300", "prompts18"])
def test_repeatable_and_capturable(name):
    M = _mod()
    table, cats, _ = _case(name)
    emb = torch.from_numpy(table).cuda()
    ids = torch.from_numpy(np.asarray(cats, dtype=np.int64).astype(np.int32)).cuda()
    cmp_ = M.EmbeddingComparer()
    a = cmp_.compare(emb, ids)
    b = cmp_.compare(emb, ids)
    torch.cuda.synchronize()
    eq = lambda x, y: all(torch.equal(x[k].view(torch.int32 if x[k].dtype == torch.float32 else torch.int64),
                                      y[k].view(torch.int32 if y[k].dtype == torch.float32 else torch.int64)) for k in x)
    assert eq(a, b)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = cmp_.compare(emb, ids)
    for _ in range(2):
        for v in c.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eq(a, c)


@pytest.mark.parametrize("want", [("normed",), ("sim",), ("dist",), ("stats",), ("sim", "stats"), ("normed", "dist"), ()])
def test_null_outputs_write_only_what_was_asked(want):
    table, cats, _ = _case("nt1_d1" if want == ("normed",) else "n2t3_d40")
    rc_all, full = raw_call(table, cats)
    rc, got = raw_call(table, cats, want=want)               # raw_call asserts that the others stay untouched
    assert rc == 0 and rc_all == 0
    for k in want:
        assert np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)), k


def test_stats_without_category_and_category_without_stats():
    table, cats, _ = _case("n2_d7")
    rc, _ = raw_call(table, None, want=("normed", "sim", "dist"))
    assert rc == 0
    rc, _ = raw_call(table, None, want=("stats",))
    assert rc == EINVAL


def test_limits_and_refusals_write_nothing():
    lib = _lib()
    assert lib.athd_embed_compare_scratch_bytes(0, 8) == 0 and lib.athd_embed_compare_scratch_bytes(4097, 8) == 0
    assert lib.athd_embed_compare_scratch_bytes(8, 0) == 0 and lib.athd_embed_compare_scratch_bytes(8, 4097) == 0
    assert lib.athd_embed_compare_scratch_bytes(4096, 4096) > 0 and lib.athd_embed_compare_scratch_bytes(1, 1) > 0
    n, d = 4, 8
    emb = torch.ones(n * d, device="cuda")
    cat = torch.zeros(n, dtype=torch.int32, device="cuda")
    need = lib.athd_embed_compare_scratch_bytes(n, d)
    out = {k: Guarded(c) for k, c in (("normed", 4097 * 8), ("sim", 64), ("dist", 64))}
    stats = Guarded(8, torch.float64)
    scratch = Guarded(lib.athd_embed_compare_scratch_bytes(4096, 8) // 8 + 1, torch.float64)

    def call(e=emb.data_ptr(), n=n, d=d, stride=d, c=cat.data_ptr(), st=stats.ptr(), sc=scratch.ptr(), nbytes=None):
        return lib.athd_embed_compare(e, n, d, stride, c, out["normed"].ptr(), out["sim"].ptr(), out["dist"].ptr(), st,
                                      sc, scratch.count * 8 if nbytes is None else nbytes, _stream())
    assert call(n=0) == EINVAL
    assert call(n=4097) == EINVAL
    assert call(d=0) == EINVAL
    assert call(d=4097) == EINVAL
    assert call(stride=d - 1) == EINVAL
    assert call(c=None) == EINVAL
    assert call(e=None) == EINVAL
    assert call(sc=None) == EINVAL
    assert call(nbytes=need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    assert all(b.untouched() for b in out.values()) and stats.untouched() and scratch.untouched()
    assert call(nbytes=need) == 0
    torch.cuda.synchronize()
    assert scratch.guards_intact() and bool(torch.all(scratch.view[(need + 7) // 8:] == SENTINEL))


# ---------------------------------------------------------------------------------------------------- Python layer
def test_python_functions(allow):
    M = _mod()
    table, cats, want = _case("prompts18")
    prompts, categories = M.collect_all_prompts()
    out = M.compare(torch.from_numpy(table).cuda(), categories)               # labels -> ids in first-seen order
    assert set(out) == {"normed", "similarity", "distance", "stats"} and all(v.is_cuda for v in out.values())
    assert out["stats"].dtype == torch.float64 and tuple(out["stats"].shape) == (8,)
    rc, raw = raw_call(table, cats)
    assert rc == 0
    for k, r in (("normed", "normed"), ("similarity", "sim"), ("distance", "dist"), ("stats", "stats")):
        assert np.array_equal(out[k].cpu().numpy().view(np.uint8), raw[r].view(np.uint8)), k
    assert M.compare(torch.from_numpy(table).cuda())["stats"] is None
    # the reference's three functions on unit rows, numpy and torch input
    unit = want["normed"]
    again = E.restatement(unit, list(cats))
    for x in (unit, torch.from_numpy(unit), torch.from_numpy(unit).cuda()):
        sim, dist = M.compute_similarity_matrix(x), M.compute_distance_matrix(x)
        assert isinstance(sim, np.ndarray) and sim.dtype == np.float32 and sim.shape == (18, 18)
        assert isinstance(dist, np.ndarray) and dist.dtype == np.float32 and dist.shape == (18, 18)
        assert np.abs(sim - again["similarity"]).max() <= allow[0] and np.abs(dist - again["distance"]).max() <= allow[1]
        res = M.analyze_clustering(x, categories)
        assert tuple(res) == E.STAT_KEYS and all(type(v) is float for v in res.values())
        tol = allow[0] * np.array([1, 1, 1, 1, 2])
        assert np.all(np.abs(np.array(list(res.values())) - again["stats"][:5]) <= tol)
    # a strided view goes in as it is
    wide = torch.full((18, 520), float("nan"), device="cuda")
    wide[:, :512] = torch.from_numpy(table).cuda()
    v = M.compare(wide[:, :512], categories)
    assert all(torch.equal(v[k], out[k]) for k in ("normed", "similarity", "distance"))
    with pytest.raises(ValueError, match="categories"):
        M.compare(torch.from_numpy(table).cuda(), categories[:-1])
    with pytest.raises(ValueError, match="4096"):
        M.compare(torch.zeros(4097, 2, device="cuda"))


def test_word2vec_route_normalises_on_the_device():
    M = _mod()
    f = E.fixture()
    ex = M.EmbeddingExtractor(word2vec_model=E.word2vec_model())
    emb, valid = ex.get_word2vec_embeddings([str(p) for p in f["prompts"]])
    assert valid == [str(p) for p in f["w2v_valid"]] and emb.dtype == np.float32 and emb.shape == (17, E.W2V_DIM)
    rows, _ = ex.word2vec_rows([str(p) for p in f["prompts"]])
    want = E.normalize_rows(rows)
    assert (np.abs(emb.astype(np.float64) - want) / E.ulp32(want)).max() <= 2.0


# ------------------------------------------------------------------------------------------------------ end to end
class WordTokenizer:
    """RoBERTa-shaped stand-in: <s> = 0, </s> = 2, pad = 1, one id in [3, 50265) per word, padded to the longest"""

    def __call__(self, prompts, padding=True, return_tensors="pt"):
        seqs = [[0] + [3 + zlib.crc32(w.encode()) % (50265 - 3) for w in p.split()] + [2] for p in prompts]
        n = max(map(len, seqs))
        ids = torch.tensor([s + [1] * (n - len(s)) for s in seqs])
        return {"input_ids": ids, "attention_mask": (ids != 1).long()}


@pytest.fixture(scope="module")
def tower():
    import clap_text_refs as R
    from athd.text import NativeClapText
    from athd.weights import synthetic_clap_text_state_dict
    sd = synthetic_clap_text_state_dict(R.SEED)
    nat = NativeClapText("cuda", dtype="f32")
    nat.load_state_dict(sd)
    return sd, nat


def test_tower_output_goes_straight_into_compare(tower, allow):
    from conftest import GOLDEN
    import os
    M = _mod()
    _, nat = tower
    with np.load(os.path.join(GOLDEN, "clap_text_ref.npz")) as z:
        ids, mask = z["five17_ids"], z["five17_mask"]
    cats = [0, 1, 0, 1, 2]
    emb = nat.encode(ids, mask, True)                          # (5, 512) on the device
    assert emb.is_cuda
    out = M.compare(emb, cats)
    host = emb.cpu().numpy()
    back = M.compare(torch.from_numpy(host).cuda(), cats)      # the same rows after a host round trip
    for k in out:
        assert np.array_equal(out[k].cpu().numpy().view(np.uint8), back[k].cpu().numpy().view(np.uint8)), k
    want = E.restatement(host, cats)
    normed = out["normed"].cpu().numpy()
    assert (np.abs(normed.astype(np.float64) - want["normed"]) / E.ulp32(want["normed"])).max() <= 2.0
    assert np.abs(out["similarity"].cpu().numpy() - want["similarity"]).max() <= allow[0]
    assert np.abs(out["distance"].cpu().numpy() - want["distance"]).max() <= allow[1]
    stats = out["stats"].cpu().numpy()
    assert stats[5] == 2 and stats[6] == 8
    assert np.all(np.abs(stats[:5] - want["stats"][:5]) <= allow[0] * np.array([1, 1, 1, 1, 2]))


def test_main_writes_the_analysis(tower, tmp_path, monkeypatch, capsys):
    """`main` on a checkpoint with the synthetic tower (handed over in memory instead of through a 0.5 GB file, as
    tests/test_gpu_clap_text.py does), a stand-in tokenizer and the stand-in Word2Vec table as --word2vec FILE.npz"""
    M = _mod()
    sd, nat = tower
    ckpt = {"model_state_dict": {"clap." + k: torch.from_numpy(v) for k, v in sd.items()}}
    monkeypatch.setattr(M.torch, "load", lambda path, **kw: ckpt)
    model = E.word2vec_model()
    np.savez(tmp_path / "w2v.npz", words=np.array(list(model)), vectors=np.stack(list(model.values())))
    try:
        import sklearn  # noqa: F401
        reduce_args = ["--method", "pca"]
    except ImportError:
        reduce_args = ["--no-reduce"]
    out_dir = tmp_path / "out"
    res = M.main(["--checkpoint", "synthetic.pt", "--word2vec", str(tmp_path / "w2v.npz"), "--output-dir", str(out_dir)]
                 + reduce_args, tokenizer=WordTokenizer())
    text = capsys.readouterr().out
    prompts, categories = M.collect_all_prompts()
    with open(out_dir / "embedding_analysis.json") as f:
        js = json.load(f)
    assert list(js) == ["clap", "word2vec", "prompts", "categories"]
    assert js["prompts"] == prompts and js["categories"] == categories
    assert js["clap"]["embeddings_shape"] == [18, 512] and list(js["clap"]["analysis"]) == list(E.STAT_KEYS)
    assert js["word2vec"]["embeddings_shape"] == [17, E.W2V_DIM] and list(js["word2vec"]["analysis"]) == list(E.STAT_KEYS)
    assert js["word2vec"]["valid_prompts"] == [p for p in prompts if p != "viola"]
    assert all(np.isfinite(v) for v in js["clap"]["analysis"].values()) and js["clap"] == res["clap"]
    with np.load(out_dir / "embeddings.npz") as z:
        assert z["clap_embeddings"].shape == (18, 512) and z["clap_similarity"].shape == (18, 18)
        assert z["clap_distance"].shape == (18, 18) and z["word2vec_similarity"].shape == (17, 17)
        assert [str(p) for p in z["prompts"]] == prompts and [str(c) for c in z["categories"]] == categories
        assert ("clap_2d" in z.files) == (reduce_args[0] == "--method")
        if "clap_2d" in z.files:
            assert z["clap_2d"].shape == (18, 2) and z["word2vec_2d"].shape == (17, 2)
        clap_emb = z["clap_embeddings"]
    # the rows are what the extractor gives for the same tower, and the analysis is the restatement's
    want_rows = M.EmbeddingExtractor(clap=nat, tokenizer=WordTokenizer()).get_clap_embeddings(prompts)
    assert np.array_equal(clap_emb.view(np.uint8), want_rows.view(np.uint8))
    a_sim = E.allowance(E.reference_gaps()[0])
    ref = E.restatement(clap_emb, categories)["stats"][:5]
    got = np.array([js["clap"]["analysis"][k] for k in E.STAT_KEYS])
    assert np.all(np.abs(got - ref) <= a_sim * np.array([1, 1, 1, 1, 2]))
    for line in ("Collected 18 prompts:", "Intra-category similarity:", "Separation (intra - inter):",
                 "SUMMARY COMPARISON", "CLAP separation:", "Word2Vec separation:", "clustering by instrument category."):
        assert line in text, line
