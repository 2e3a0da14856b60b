"""References of the embedding-comparison tests (tests/test_embedding_refs.py on the CPU, tests/test_gpu_embedding.py on
the GPU): the float64 restatement of the semantics stated in include/athd.h (`athd_embed_compare`), the seeded cases and
the allowances.  A plain helper module; numpy only.

Restatement, for a table e (n, d) float32 and category ids c (n):
  normed[i] = e[i] / (float32(sqrt(sum_k float64(e[i,k])^2)) + float32(1e-8))        float32 addition and division
  g         = float64(normed) float64(normed)^T
  sim[i,j]  = g_ij / (s_i s_j),  s_i = sqrt(g_ii), 1 where that is 0                 float64, not rounded
  dist[i,j] = sqrt(max(g_ii + g_jj - 2 g_ij, 0)), 0 on the diagonal                  float64, not rounded
  stats     = {intra_mean, intra_std, inter_mean, inter_std, separation, n_intra, n_inter, 0} over the pairs i < j of
              float32(sim), split by c_i == c_j, float64 (np.mean / np.std; NaN for an empty class)

Allowances (tests/test_gpu_embedding.py): `a_sim` / `a_dist` are the largest |reference - restatement| over the
recorded cases of tests/golden/embedding_ref.npz, i.e. the error scikit-learn's own float32 route has against this
restatement; a device value may differ from the restatement by max(4 a, 2^-23): the factor 4 is the margin the other
fp32 twins of this project get, 2^-23 is one rounding of a float32 near 1.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embedding_ref.npz")
STAT_KEYS = ("intra_category_mean", "intra_category_std", "inter_category_mean", "inter_category_std", "separation")
FLOOR = 2.0 ** -23
MARGIN = 4.0

# the 18 prompts the reference collects (its prompt table + three string instruments), recorded in the fixture too
N_PROMPTS, N_CATEGORIES = 18, 5


# ------------------------------------------------------------------------------------------------------ restatement
def normalize_rows(emb) -> np.ndarray:
    e = np.asarray(emb, dtype=np.float32)
    norm = np.sqrt((e.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    return (e / (norm + np.float32(1e-8))[:, None]).astype(np.float32)


def gram(normed) -> np.ndarray:
    v = np.asarray(normed, dtype=np.float32).astype(np.float64)
    return v @ v.T


def similarity(normed) -> np.ndarray:
    g = gram(normed)
    s = np.sqrt(np.diag(g))
    s = np.where(s == 0.0, 1.0, s)
    return g / (s[:, None] * s[None, :])


def distance(normed) -> np.ndarray:
    g = gram(normed)
    gd = np.diag(g)
    out = np.sqrt(np.maximum(gd[:, None] + gd[None, :] - 2.0 * g, 0.0))
    np.fill_diagonal(out, 0.0)
    return out


def pair_classes(categories):
    """(iu, ju, same): the pairs i < j in row-major order and whether their categories agree"""
    c = np.unique(np.asarray(list(categories)), return_inverse=True)[1].reshape(-1)
    iu, ju = np.triu_indices(len(c), k=1)
    return iu, ju, c[iu] == c[ju]


def stats_of(sim, categories) -> np.ndarray:
    """the 8 doubles of athd_embed_compare from a similarity matrix (rounded to float32 first, as the routine's is)"""
    s = np.asarray(sim).astype(np.float32).astype(np.float64)
    iu, ju, same = pair_classes(categories)
    x = s[iu, ju]
    intra, inter = x[same], x[~same]
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m0 = np.mean(intra) if intra.size else np.nan
            s0 = np.std(intra) if intra.size else np.nan
            m1 = np.mean(inter) if inter.size else np.nan
            s1 = np.std(inter) if inter.size else np.nan
    return np.array([m0, s0, m1, s1, m0 - m1, float(intra.size), float(inter.size), 0.0])


def restatement(emb, categories=None) -> dict:
    v = normalize_rows(emb)
    out = {"normed": v, "similarity": similarity(v), "distance": distance(v)}
    if categories is not None:
        out["stats"] = stats_of(out["similarity"], categories)
    return out


def ulp32(x) -> np.ndarray:
    """spacing of float32 at |x| (the smallest normal's spacing below it)"""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def allowance(a: float) -> float:
    return max(MARGIN * float(a), FLOOR)


# ------------------------------------------------------------------------------------------------------------ cases
def _table(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _cats(seed, n, k):
    return np.random.default_rng(1000 + seed).integers(0, k, size=n).astype(np.int64)


def shape_case(n, d, seed):
    return _table(seed, n, d), _cats(seed, n, 3)


def _zero_row():
    e = _table(21, 5, 7)
    e[2] = 0.0
    return e, np.array([0, 1, 0, 1, 0], dtype=np.int64)


def _parallel_duplicate():
    e = _table(22, 6, 300)
    e[3] = np.float32(2.5) * e[1]          # parallel to row 1
    e[4] = e[0]                            # an exact duplicate of row 0
    return e, np.array([0, 1, 2, 1, 0, 2], dtype=np.int64)


def _all_equal():
    e = np.repeat(_table(26, 1, 300), 7, axis=0)
    return e, np.array([0, 0, 1, 1, 0, 1, 0], dtype=np.int64)


def prompt_case(prompts, categories):
    """the reference's own 18 prompts with its 5 categories on a seeded (18, 512) table"""
    assert len(prompts) == N_PROMPTS and len(set(categories)) == N_CATEGORIES
    return _table(27, N_PROMPTS, 512), list(categories)


def recorded_cases(tile: int) -> dict:
    """name -> (table (n, d) float32, category ids): the cases the fixture records the reference's outputs for.  `tile`
    is the kernel's tile edge (athd.embedding_comparison.TILE): n = 1, 2, t, t + 1, 2 t + 3 and d = 1, 7, 300, 512."""
    t = int(tile)
    return {
        "n1_d512": shape_case(1, 512, 1),
        "n2_d7": shape_case(2, 7, 2),
        "nt_d300": shape_case(t, 300, 3),
        "nt1_d1": shape_case(t + 1, 1, 4),
        "n2t3_d40": shape_case(2 * t + 3, 40, 5),
        "zero_row": _zero_row(),
        "parallel_duplicate": _parallel_duplicate(),
        "one_category": (_table(23, 9, 7), np.zeros(9, dtype=np.int64)),
        "all_distinct": (_table(24, 9, 7), np.arange(9, dtype=np.int64) * 7 - 20),
        "odd_ids": (_table(25, 12, 7), np.array([-2 ** 31, 2 ** 31 - 1, -1, 0, -2 ** 31, 2 ** 31 - 1, -1, 0, 5, 5,
                                                 -1, 2 ** 31 - 1], dtype=np.int64)),
        "all_equal": _all_equal(),
    }


def gpu_only_cases(tile: int) -> dict:
    """larger shapes checked against the restatement alone (not recorded: they would triple the fixture)"""
    t = int(tile)
    return {"n2t3_d512": shape_case(2 * t + 3, 512, 6), "n2t3_d300": shape_case(2 * t + 3, 300, 7),
            # the limits: d = 4096 fills every register group of the row pass (d = 512 uses the first only); n = 4096
            # gives 2080 tiles, more than the 256 threads that add their partials
            "n3_d4096": shape_case(3, 4096, 8), "n4096_d3": shape_case(4096, 3, 9)}


# ---- Word2Vec stand-in of the fixture: a dict is "any object with `in` and `[]`" ----
W2V_DIM = 300


def word2vec_model() -> dict:
    words = ["drums", "drum", "kit", "percussion", "the", "bass", "guitar", "line", "other", "instruments",
             "accompaniment", "vocals", "voice", "singing", "violin", "cello"]          # "viola" is unknown
    rng = np.random.default_rng(28)
    return {w: rng.standard_normal(W2V_DIM).astype(np.float32) for w in words}


# ------------------------------------------------------------------------------------------------------- the fixture
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(GOLDEN) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def reference_gaps():
    """(a_sim, a_dist, per case {name: (a_sim, a_dist)}): |reference - restatement| on the recorded cases, each the
    reference's own float32 route against the float64 restatement of its own input rows."""
    f = fixture()
    per = {}
    for name in [str(s) for s in f["case_names"]]:
        v = f[f"{name}_normed"]
        per[name] = (float(np.abs(f[f"{name}_similarity"].astype(np.float64) - similarity(v)).max()),
                     float(np.abs(f[f"{name}_distance"].astype(np.float64) - distance(v)).max()))
    return max(p[0] for p in per.values()), max(p[1] for p in per.values()), per
