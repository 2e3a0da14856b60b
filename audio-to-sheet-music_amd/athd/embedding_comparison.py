"""The reference's `embedding_comparison.py` by name: do CLAP's text embeddings cluster the stem prompts better than
Word2Vec's?

  * `compare`                       <- one `athd_embed_compare` (include/athd.h): the normalised table (`:109-111`), the
                                       cosine-similarity and Euclidean-distance matrices (`:177-184`) and the intra /
                                       inter category statistics (`:307-333`), fp64-accumulated, as device tensors
  * `compute_similarity_matrix`, `compute_distance_matrix`, `analyze_clustering`
                                    <- `:177-184`, `:307-333`: numpy or torch in, numpy / Python floats out
  * `EmbeddingExtractor`            <- `:66-154`; the CLAP rows come from the native text tower (`NativeClapText`) or
                                       from anything `PromptEmbedder` accepts, the Word2Vec rows from any object with
                                       `in` and `[]`; both are normalised by the device routine
  * `collect_all_prompts`           <- `:157-174`, on `athd.musdb.STEM_PROMPTS`
  * `convert_to_native_types`       <- `:289-304`
  * `reduce_dimensions`             <- `:187-210`, delegated to scikit-learn on the host when it is importable
  * `main`                          <- `:378-538` without the figures and the TensorBoard export: the arrays they would
                                       show go to `embeddings.npz` beside `embedding_analysis.json`

The device routine normalises its input rows before it compares them, as the reference's pipeline does (every table
it compares went through `emb / (norm + 1e-8)` first).  The three wrappers are therefore meant for unit rows, which is
all the reference passes them: on other rows the similarity is the same up to rounding (a cosine does not see a row's
length), but `compute_distance_matrix` returns the distances of the NORMALISED rows.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .musdb import STEM_PROMPTS

TILE = 64                 # tile edge of the pair pass (EC_TILE of csrc/embed_compare.hip)
MAX_ROWS = 4096           # 1 <= n <= 4096
MAX_DIM = 4096            # 1 <= d <= 4096
STATS = ("intra_category_mean", "intra_category_std", "inter_category_mean", "inter_category_std", "separation")
STRING_INSTRUMENTS = ("violin", "viola", "cello")        # `:169`


def category_ids(categories: Sequence) -> np.ndarray:
    """Category labels (any hashables: strings, ints) -> int32 ids in first-seen order."""
    seen: Dict = {}
    return np.array([seen.setdefault(c, len(seen)) for c in categories], dtype=np.int32)


class EmbeddingComparer:
    """Owns the scratch of `athd_embed_compare` (grown on demand, like `NativeClapText._ws`)."""

    def __init__(self):
        self._ws: Optional[torch.Tensor] = None

    def compare(self, emb: torch.Tensor, categories=None, normed: bool = True, similarity: bool = True,
                distance: bool = True) -> Dict[str, Optional[torch.Tensor]]:
        """emb: (n, d) float32 on a HIP device (rows may be strided: stride(1) == 1, stride(0) >= d).  categories: None
        (no statistics), a sequence of labels, or an integer tensor / array of n ids.  Returns device tensors `normed`
        (n, d), `similarity` (n, n), `distance` (n, n) float32 and `stats` (8,) float64 = {intra_mean, intra_std,
        inter_mean, inter_std, separation, n_intra, n_inter, 0}; an output that was not asked for is None.  One
        `athd_embed_compare` on the current torch stream, no synchronisation."""
        from . import native
        if not isinstance(emb, torch.Tensor) or emb.dim() != 2:
            raise ValueError("compare: emb must be a 2-D torch tensor (n, d)")
        if emb.device.type != "cuda":
            raise ValueError("compare: emb must be on a HIP device (there is no CPU path)")
        if emb.dtype != torch.float32:
            emb = emb.float()
        n, d = emb.shape
        if not (1 <= n <= MAX_ROWS and 1 <= d <= MAX_DIM):
            raise ValueError(f"compare: n must be in [1, {MAX_ROWS}] and d in [1, {MAX_DIM}], got ({n}, {d})")
        if emb.stride(1) != 1 or (n > 1 and emb.stride(0) < d):
            emb = emb.contiguous()
        row_stride = emb.stride(0) if n > 1 else d
        dev = emb.device
        cat = None
        if categories is not None:
            if isinstance(categories, torch.Tensor):
                cat = categories.to(dev, torch.int32).contiguous()
            elif (isinstance(categories, np.ndarray) and categories.dtype.kind in "iu" and categories.size
                  and -2 ** 31 <= int(categories.min()) and int(categories.max()) < 2 ** 31):
                cat = torch.from_numpy(categories.astype(np.int32)).to(dev)
            else:
                cat = torch.from_numpy(category_ids(list(categories))).to(dev)
            if cat.dim() != 1 or cat.numel() != n:
                raise ValueError(f"compare: {cat.numel()} categories for {n} rows")
        need = int(native.lib.athd_embed_compare_scratch_bytes(n, d))
        if self._ws is None or self._ws.device != dev or self._ws.numel() * 8 < need:
            self._ws = None
            self._ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        out = {
            "normed": torch.empty((n, d), dtype=torch.float32, device=dev) if normed else None,
            "similarity": torch.empty((n, n), dtype=torch.float32, device=dev) if similarity else None,
            "distance": torch.empty((n, n), dtype=torch.float32, device=dev) if distance else None,
            "stats": torch.empty(8, dtype=torch.float64, device=dev) if cat is not None else None,
        }
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(dev):
            rc = native.lib.athd_embed_compare(emb.data_ptr(), n, d, row_stride, ptr(cat), ptr(out["normed"]),
                                               ptr(out["similarity"]), ptr(out["distance"]), ptr(out["stats"]),
                                               self._ws.data_ptr(), self._ws.numel() * 8,
                                               torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise native.AthdError(f"athd_embed_compare failed ({rc})")
        return out


_default = EmbeddingComparer()


def compare(emb: torch.Tensor, categories=None) -> Dict[str, Optional[torch.Tensor]]:
    """`EmbeddingComparer.compare` on a module-level comparer: normed, similarity, distance and (with categories) stats."""
    return _default.compare(emb, categories)


def _on_device(embeddings, device=None) -> torch.Tensor:
    t = embeddings if isinstance(embeddings, torch.Tensor) else torch.from_numpy(np.asarray(embeddings, np.float32))
    if t.device.type != "cuda":
        t = t.to(device or "cuda")
    return t.float()


def compute_similarity_matrix(embeddings) -> np.ndarray:
    """`:177-179`: cosine similarity (n, n) float32 of unit rows (see the module text)."""
    out = _default.compare(_on_device(embeddings), None, normed=False, distance=False)
    return out["similarity"].cpu().numpy()


def compute_distance_matrix(embeddings) -> np.ndarray:
    """`:182-184`: Euclidean distance (n, n) float32 of unit rows (see the module text)."""
    out = _default.compare(_on_device(embeddings), None, normed=False, similarity=False)
    return out["distance"].cpu().numpy()


def stats_dict(stats) -> Dict[str, float]:
    """The reference's five keys (`:325-331`) from the 8 doubles of `compare`."""
    s = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    return {k: float(s[i]) for i, k in enumerate(STATS)}


def analyze_clustering(embeddings, categories: Sequence) -> Dict[str, float]:
    """`:307-333`: mean and population std of the similarities of the pairs i < j inside a category and across
    categories, and their separation, as Python floats (NaN for a class without pairs)."""
    out = _default.compare(_on_device(embeddings), categories, normed=False, similarity=False, distance=False)
    return stats_dict(out["stats"])


def collect_all_prompts() -> Tuple[List[str], List[str]]:
    """`:157-174`: every prompt of STEM_PROMPTS with its stem as category, then the three string instruments under
    "strings"."""
    prompts = [p for ps in STEM_PROMPTS.values() for p in ps]
    categories = [stem for stem, ps in STEM_PROMPTS.items() for _ in ps]
    return prompts + list(STRING_INSTRUMENTS), categories + ["strings"] * len(STRING_INSTRUMENTS)


def convert_to_native_types(obj):
    """`:289-304`: numpy scalars and arrays -> Python numbers and lists, through dicts, lists and tuples."""
    if isinstance(obj, np.integer):
        return int(obj)
    if isinstance(obj, np.floating):
        return float(obj)
    if isinstance(obj, np.ndarray):
        return obj.tolist()
    if isinstance(obj, dict):
        return {k: convert_to_native_types(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(convert_to_native_types(v) for v in obj)
    return obj


def reduce_dimensions(embeddings, method: str = "tsne", n_components: int = 2, random_state: int = 42) -> np.ndarray:
    """`:187-210` on the host with scikit-learn (t-SNE, PCA; UMAP when umap-learn is installed, t-SNE otherwise as in
    the reference).  Not a device routine and not part of any parity claim."""
    if method not in ("tsne", "pca", "umap"):
        raise ValueError(f"Unknown method: {method}")
    x = embeddings.detach().cpu().numpy() if isinstance(embeddings, torch.Tensor) else np.asarray(embeddings)
    try:
        from sklearn.decomposition import PCA
        from sklearn.manifold import TSNE
    except ImportError as e:
        raise ImportError(f"reduce_dimensions needs scikit-learn on the host ({e}); run with --no-reduce, or install "
                          f"it: the similarity, distance and clustering results do not depend on it") from e
    if method == "umap":
        try:
            import umap
            return umap.UMAP(n_components=n_components, random_state=random_state).fit_transform(x)
        except ImportError:
            print("Warning: UMAP not available. Falling back to t-SNE.")
            method = "tsne"
    if method == "pca":
        return PCA(n_components=n_components, random_state=random_state).fit_transform(x)
    return TSNE(n_components=n_components, random_state=random_state, perplexity=min(30, len(x) - 1),
                max_iter=1000).fit_transform(x)


def load_word2vec_npz(path) -> Dict[str, np.ndarray]:
    """A Word2Vec table exported to .npz: `words` (V,) strings and `vectors` (V, dim) floats -> {word: vector}."""
    with np.load(path) as z:
        words, vectors = z["words"], np.asarray(z["vectors"], dtype=np.float32)
    if vectors.ndim != 2 or len(words) != len(vectors):
        raise ValueError(f"{path}: expected words (V,) and vectors (V, dim), got {words.shape} and {vectors.shape}")
    return {str(w): v for w, v in zip(words, vectors)}


class EmbeddingExtractor:
    """`:66-154`.  `clap`: a `NativeClapText` (its output stays on the device and goes straight into the device
    normalisation) or anything `PromptEmbedder` accepts (a Hugging Face ClapModel / ClapTextModelWithProjection) with
    `tokenizer`; with neither, `load_clap` takes both from the local Hugging Face cache.  `word2vec_model`: any object
    with `in` and `[]` (a gensim KeyedVectors, a dict).  The gensim download of `:84-96` is out of scope."""

    def __init__(self, device=None, clap=None, tokenizer=None, word2vec_model=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("athd runs on a HIP device only (there is no CPU path)")
        self.clap_model = clap
        self.clap_tokenizer = tokenizer
        self.word2vec_model = word2vec_model
        self._cmp = EmbeddingComparer()

    def load_clap(self):
        from .text import load_clap
        self.clap_model, self.clap_tokenizer = load_clap()

    def load_word2vec(self, model_name: str = "word2vec-google-news-300"):
        raise RuntimeError(f"Word2Vec model '{model_name}' is fetched over the network by the reference (gensim's "
                           f"downloader); pass word2vec_model= (any object with `in` and `[]`) or --word2vec FILE.npz")

    def _normalize(self, rows: torch.Tensor) -> torch.Tensor:
        return self._cmp.compare(rows, None, similarity=False, distance=False)["normed"]

    def clap_embeddings_device(self, texts: List[str]) -> torch.Tensor:
        """`get_clap_embeddings` with the (N, 512) rows left on the device."""
        from .text import NativeClapText, PromptEmbedder
        if self.clap_model is None:
            self.load_clap()
        if self.clap_tokenizer is None:
            raise ValueError("EmbeddingExtractor: a tokenizer is needed to embed prompts")
        if isinstance(self.clap_model, NativeClapText):
            if self.clap_model.device is None:
                self.clap_model.to(self.device)
            feats = self.clap_model.embed(list(texts), self.clap_tokenizer, True)      # get_text_features rows
        else:
            feats = PromptEmbedder(self.clap_model, self.clap_tokenizer)._clap_embed(list(texts)).to(self.device)
        return self._normalize(feats)

    def get_clap_embeddings(self, texts: List[str]) -> np.ndarray:
        """`:98-113`: (N, 512) float32 rows, `emb / (norm + 1e-8)`."""
        return self.clap_embeddings_device(texts).cpu().numpy()

    def word2vec_rows(self, texts: List[str]) -> Tuple[np.ndarray, List[str]]:
        """`:125-148` on the host: per prompt the mean of the vectors of its known lower-cased words; a prompt with
        none is reported and skipped."""
        if self.word2vec_model is None:
            self.load_word2vec()
        rows, valid = [], []
        for text in texts:
            vecs = [self.word2vec_model[w] for w in text.lower().split() if w in self.word2vec_model]
            if vecs:
                rows.append(np.mean(vecs, axis=0))
                valid.append(text)
            else:
                print(f"Warning: Could not embed '{text}' - no words found in vocabulary")
        if not rows:
            raise ValueError("No valid embeddings could be generated")
        return np.array(rows), valid

    def word2vec_embeddings_device(self, texts: List[str]) -> Tuple[torch.Tensor, List[str]]:
        rows, valid = self.word2vec_rows(texts)
        return self._normalize(torch.from_numpy(np.asarray(rows, dtype=np.float32)).to(self.device)), valid

    def get_word2vec_embeddings(self, texts: List[str]) -> Tuple[np.ndarray, List[str]]:
        """`:115-154`: (embeddings (M, dim) float32 normalised on the device, the M prompts that embedded)."""
        emb, valid = self.word2vec_embeddings_device(texts)
        return emb.cpu().numpy(), valid


def build_results(clap_shape, clap_analysis, prompts, categories, w2v_shape=None, w2v_analysis=None,
                  valid_prompts=None) -> dict:
    """The layout of embedding_analysis.json (`:507-522`)."""
    return convert_to_native_types({
        "clap": {"embeddings_shape": list(clap_shape), "analysis": clap_analysis},
        "word2vec": {"embeddings_shape": list(w2v_shape) if w2v_shape is not None else None,
                     "analysis": w2v_analysis, "valid_prompts": valid_prompts},
        "prompts": prompts,
        "categories": categories,
    })


def _print_analysis(a: Dict[str, float]):
    print(f"Intra-category similarity: {a['intra_category_mean']:.3f} ± {a['intra_category_std']:.3f}")
    print(f"Inter-category similarity: {a['inter_category_mean']:.3f} ± {a['inter_category_std']:.3f}")
    print(f"Separation (intra - inter): {a['separation']:.3f}")


def main(argv=None, tokenizer=None, word2vec_model=None) -> dict:
    """`python -m athd.embedding_comparison --checkpoint PATH --tokenizer DIR [--word2vec FILE.npz] [--output-dir DIR]
    [--method pca|tsne|umap] [--no-reduce] [--dtype f32|bf16]`.  `tokenizer` / `word2vec_model` replace --tokenizer /
    --word2vec for callers that hold them.  Returns the dict written to embedding_analysis.json."""
    ap = argparse.ArgumentParser(prog="python -m athd.embedding_comparison",
                                 description="Compare CLAP vs Word2Vec embeddings of the stem prompts")
    ap.add_argument("--checkpoint", required=True, help="checkpoint with the clap.text_model.* / clap.text_projection.* keys")
    ap.add_argument("--tokenizer", default=None, help="directory of the CLAP tokenizer (RobertaTokenizerFast files)")
    ap.add_argument("--word2vec", default=None, help=".npz with `words` and `vectors` (no download here)")
    ap.add_argument("--output-dir", default="embedding_comparisons")
    ap.add_argument("--method", default="tsne", choices=["tsne", "pca", "umap"])
    ap.add_argument("--no-reduce", action="store_true", help="skip the 2-D projection (needs scikit-learn on the host)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="precision of the text tower")
    args = ap.parse_args(argv)

    from .text import NativeClapText
    if tokenizer is None:
        if args.tokenizer is None:
            ap.error("--tokenizer DIR is required")
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(args.tokenizer, local_files_only=True)
    if word2vec_model is None and args.word2vec:
        word2vec_model = load_word2vec_npz(args.word2vec)
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    sd = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt
    tower = NativeClapText("cuda", dtype=args.dtype)
    tower.load_state_dict({k: v for k, v in sd.items() if "text_model." in k or "text_projection." in k})

    output_dir = Path(args.output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    prompts, categories = collect_all_prompts()
    print(f"\nCollected {len(prompts)} prompts:")
    for prompt, cat in zip(prompts, categories):
        print(f"  {cat}: {prompt}")
    extractor = EmbeddingExtractor("cuda", clap=tower, tokenizer=tokenizer, word2vec_model=word2vec_model)
    arrays = {"prompts": np.array(prompts), "categories": np.array(categories)}

    def analyse(tag, emb, cats):
        out = _default.compare(emb, cats, normed=False)
        analysis = stats_dict(out["stats"])
        arrays.update({f"{tag}_embeddings": emb.cpu().numpy(), f"{tag}_similarity": out["similarity"].cpu().numpy(),
                       f"{tag}_distance": out["distance"].cpu().numpy()})
        _print_analysis(analysis)
        if not args.no_reduce:
            arrays[f"{tag}_2d"] = np.asarray(reduce_dimensions(arrays[f"{tag}_embeddings"], method=args.method))
        return analysis

    print("\n" + "=" * 60 + "\nAnalyzing CLAP embeddings...\n" + "=" * 60)
    clap_emb = extractor.clap_embeddings_device(prompts)
    print(f"CLAP embeddings shape: {tuple(clap_emb.shape)}")
    clap_analysis = analyse("clap", clap_emb, categories)

    w2v_emb = w2v_analysis = valid = None
    if word2vec_model is not None:
        print("\n" + "=" * 60 + "\nAnalyzing Word2Vec embeddings...\n" + "=" * 60)
        try:
            w2v_emb, valid = extractor.word2vec_embeddings_device(prompts)
        except ValueError as e:
            print(f"Error extracting Word2Vec embeddings: {e}")
        if w2v_emb is not None:
            valid_categories = [c for p, c in zip(prompts, categories) if p in valid]
            print(f"Word2Vec embeddings shape: {tuple(w2v_emb.shape)}")
            print(f"Valid prompts: {len(valid)}/{len(prompts)}")
            w2v_analysis = analyse("word2vec", w2v_emb, valid_categories)
            arrays.update(word2vec_prompts=np.array(valid), word2vec_categories=np.array(valid_categories))

    results = build_results(clap_emb.shape, clap_analysis, prompts, categories,
                            w2v_emb.shape if w2v_emb is not None else None, w2v_analysis, valid)
    results_file = output_dir / "embedding_analysis.json"
    with open(results_file, "w") as f:
        json.dump(results, f, indent=2)
    np.savez(output_dir / "embeddings.npz", **arrays)
    print(f"\nResults saved to {results_file}")
    print(f"\nAll outputs saved to {output_dir}")
    if w2v_analysis is not None:
        print("\n" + "=" * 60 + "\nSUMMARY COMPARISON\n" + "=" * 60)
        print(f"CLAP separation:     {clap_analysis['separation']:.3f}")
        print(f"Word2Vec separation: {w2v_analysis['separation']:.3f}")
        better = "better" if clap_analysis["separation"] > w2v_analysis["separation"] else "worse"
        print(f"\nCLAP shows {better} clustering by instrument category.")
    return results


if __name__ == "__main__":
    main()
