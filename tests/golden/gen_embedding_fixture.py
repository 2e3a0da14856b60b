"""Generator of tests/golden/embedding_ref.npz: the reference's own `embedding_comparison.py` functions on the seeded
cases of tests/embedding_refs.py.  Run once by hand where the reference checkout is available; never run by a test:

    python tests/golden/gen_embedding_fixture.py --reference /path/to/reference/checkout

The reference module imports matplotlib, scikit-learn and transformers at its top (all needed here: scikit-learn does the
work being recorded); `src.dataloader` imports stempeg and soundfile, which are satisfied by empty stand-ins when they
are not installed, as tests/golden/gen_loss_fixture.py does.  seaborn, umap and gensim are optional in the reference.

The file holds data only:
  prompts, categories (18,) strings                   `collect_all_prompts()`
  case_names                                          the cases of embedding_refs.recorded_cases(TILE) + "prompts18"
  per case <name>:
    <name>_input (n, d) float32, <name>_categories    the seeded table and category ids (labels for prompts18)
    <name>_normed (n, d) float32                      `EmbeddingExtractor.get_clap_embeddings` with a stand-in model
                                                      whose `get_text_features` returns the table (its normalisation)
    <name>_similarity, <name>_distance (n, n) float32 `compute_similarity_matrix` / `compute_distance_matrix` of _normed
    <name>_analysis (5,) float64                      `analyze_clustering(_normed, categories)` in the order of STAT_KEYS
  w2v_words, w2v_vectors                              the stand-in Word2Vec table (embedding_refs.word2vec_model)
  w2v_embeddings, w2v_valid                           `get_word2vec_embeddings(prompts)` with that table ("viola" unknown)
  tile, sklearn_version, numpy_version
"""
import argparse
import importlib
import importlib.machinery
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "audio-to-sheet-music_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _stand_in(name: str):
    try:
        importlib.import_module(name)
    except ImportError:
        mod = types.ModuleType(name)
        mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
        sys.modules[name] = mod


def import_reference(root: str):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, os.path.abspath(root))
    _stand_in("stempeg")
    _stand_in("soundfile")
    return importlib.import_module("embedding_comparison")


class _Features:
    """stand-in CLAP model: `get_text_features` returns the seeded table"""

    def __init__(self, table):
        self.table = torch.from_numpy(np.asarray(table, dtype=np.float32))

    def get_text_features(self, **inputs):
        assert inputs["input_ids"].shape[0] == self.table.shape[0]
        return self.table.clone()


def _tokenizer(texts, padding=True, return_tensors="pt"):
    return {"input_ids": torch.zeros((len(texts), 1), dtype=torch.long)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="directory of the reference checkout (holds embedding_comparison.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "embedding_ref.npz"))
    args = ap.parse_args()
    ref = import_reference(args.reference)

    import sklearn

    import embedding_refs as E
    from athd.embedding_comparison import TILE

    prompts, categories = ref.collect_all_prompts()
    arrays = {"prompts": np.array(prompts), "categories": np.array(categories), "tile": np.array(TILE),
              "sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    cases = dict(E.recorded_cases(TILE))
    cases["prompts18"] = E.prompt_case(prompts, categories)
    arrays["case_names"] = np.array(list(cases))
    for name, (table, cats) in cases.items():
        ex = ref.EmbeddingExtractor(device="cpu")
        ex.clap_model, ex.clap_tokenizer = _Features(table), _tokenizer
        normed = ex.get_clap_embeddings(["x"] * len(table))
        assert normed.dtype == np.float32 and normed.shape == table.shape
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")            # np.mean([]) of an empty class
            analysis = ref.analyze_clustering(normed, list(cats))
        assert tuple(analysis) == E.STAT_KEYS, tuple(analysis)
        arrays.update({f"{name}_input": table, f"{name}_categories": np.array(cats), f"{name}_normed": normed,
                       f"{name}_similarity": ref.compute_similarity_matrix(normed),
                       f"{name}_distance": ref.compute_distance_matrix(normed),
                       f"{name}_analysis": np.array([analysis[k] for k in E.STAT_KEYS], dtype=np.float64)})
        assert arrays[f"{name}_similarity"].dtype == np.float32 and arrays[f"{name}_distance"].dtype == np.float32

    model = E.word2vec_model()
    ex = ref.EmbeddingExtractor(device="cpu")
    ex.word2vec_model = model
    emb, valid = ex.get_word2vec_embeddings(prompts)
    assert len(valid) == len(prompts) - 1 and "viola" not in valid
    arrays.update(w2v_words=np.array(list(model)), w2v_vectors=np.stack(list(model.values())),
                  w2v_embeddings=emb, w2v_valid=np.array(valid))
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
