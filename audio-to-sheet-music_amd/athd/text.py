"""Prompt -> 512-d text embedding (the CLAP side of `ATHTDemucs_v2.py:238-248`).

The CLAP text tower is frozen and its output depends only on the prompt string, so it is evaluated once per
distinct prompt and cached; the per-segment hot path only sees embedding rows.  Sources, in order:
  1. an explicit table {prompt: (512,) vector} (used when no CLAP weights exist offline - synthetic runs);
  2. a real CLAP model + tokenizer passed like the reference (`ClapModel.get_text_features` for ClapModel,
     `.forward(...).text_embeds` otherwise, exactly the branch logic of `_get_clap_embeddings`);
  3. the native tower (`NativeClapText`, `athd_text_*` of include/athd.h) + a tokenizer: the same two branches computed
     by libathd.so from the tower weights a checkpoint carries under `clap.`, without a Hugging Face model.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Union

import numpy as np
import torch

from .weights import STEMS, synthetic_text_table


CLAP_NAME = "laion/clap-htsat-unfused"     # test_inference.py:27-28


def load_clap(name: str = CLAP_NAME):
    """The reference's `ClapModel.from_pretrained(name)` + `AutoTokenizer.from_pretrained(name)`
    (`test_inference.py:26-28`), from the local Hugging Face cache only (`local_files_only=True`: there is no
    network on the target nodes).  Raises a RuntimeError naming the missing model and the `text_table=` alternative
    when the cache lacks its files."""
    try:
        from transformers import AutoTokenizer, ClapModel
    except ImportError as e:   # pragma: no cover - transformers is in the image
        raise RuntimeError(f"CLAP '{name}' needs transformers ({e}); pass text_table={{prompt: 512-vector}} "
                           f"instead") from e
    try:
        clap = ClapModel.from_pretrained(name, local_files_only=True)
        tokenizer = AutoTokenizer.from_pretrained(name, local_files_only=True)
    except (OSError, ValueError) as e:
        raise RuntimeError(
            f"CLAP model '{name}' is not in the local Hugging Face cache ({type(e).__name__}: {e}). The reference "
            f"downloads it (test_inference.py:27-28); offline, either place its files in the cache (HF_HOME) or pass "
            f"text_table={{prompt: 512-vector}} (e.g. precomputed ClapModel.get_text_features rows) or "
            f"clap=/tokenizer=") from e
    clap.eval()
    for p in clap.parameters():          # frozen, as ATHTDemucs_v2.py:174-176
        p.requires_grad = False
    return clap, tokenizer


class NativeClapText:
    """The CLAP text tower in libathd.so (`athd_text_*`): RoBERTa-base, pooler and projection as HIP kernels.

    `dtype` "f32" (default: a prompt is embedded once and cached, so accuracy is worth more than the time) or "bf16".
    The device context is built on the first `encode` (or `to`) from the weights given to `load_state_dict`.  The
    tokenizer stays the caller's (`RobertaTokenizerFast` for laion/clap-htsat-unfused): its vocabulary files are not
    part of a checkpoint."""

    def __init__(self, device=None, dtype: str = "f32"):
        if dtype not in ("bf16", "f32"):
            raise ValueError("dtype must be 'bf16' or 'f32'")
        self.dtype = dtype
        self.device: Optional[torch.device] = None
        self._weights: Optional[Dict[str, np.ndarray]] = None
        self._ctx = None
        self._ws: Optional[torch.Tensor] = None
        self.calls = 0                      # native encode calls (the cache tests count them)
        if device is not None:
            self.to(device)

    @property
    def loaded(self) -> bool:
        return self._weights is not None or self._ctx is not None

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("athd runs on a HIP device only (there is no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_initialized() else 0)
        if self.device != device and self._ctx is not None:
            raise RuntimeError("the text tower is already on %s; load_state_dict again to move it" % self.device)
        self.device = device
        return self

    def load_state_dict(self, state) -> int:
        """A checkpoint's `clap.*` keys, or a `ClapModel` / `ClapTextModelWithProjection` state dict (torch tensors
        or arrays; a leading `clap.` is optional).  Raises a KeyError listing the missing tower keys.  Returns the
        number of tensors taken."""
        from . import native
        need = native.text_required_keys()
        got = {}
        for k, v in state.items():
            if k.startswith("module."):
                k = k[len("module."):]
            if k.startswith("clap."):
                k = k[len("clap."):]
            got[k] = v
        missing = [k for k in need if k not in got]
        if missing:
            raise KeyError(f"CLAP text tower: {len(missing)} of {len(need)} weights missing: "
                           f"{missing[:6]}{' ...' if len(missing) > 6 else ''}")
        w = {}
        for k in need:
            v = got[k]
            if isinstance(v, torch.Tensor):
                v = v.detach().to("cpu", torch.float32).numpy()
            w[k] = np.asarray(v, dtype=np.float32)
        self._weights = w
        self._ctx = None
        return len(need)

    def _ensure_ctx(self):
        if self._ctx is not None:
            return self._ctx
        from . import native
        if self._weights is None:
            raise RuntimeError("NativeClapText has no weights: call load_state_dict with the tower's keys first")
        if self.device is None:
            self.to("cuda")
        ctx = native.TextContext(self.device.index, native.BF16 if self.dtype == "bf16" else native.F32)
        for k, v in self._weights.items():
            ctx.set_weight(k, v)
        ctx.finalize()
        self._weights = None                # packed on the device now
        self._ctx = ctx
        return ctx

    @torch.no_grad()
    def encode(self, input_ids, attention_mask, normalize: bool) -> torch.Tensor:
        """(P, L) token ids and attention mask (any integer tensors) -> (P, 512) f32 on the tower's device, enqueued
        on the current torch stream (no synchronisation)."""
        ctx = self._ensure_ctx()
        ids = torch.as_tensor(input_ids)
        mask = torch.as_tensor(attention_mask)
        if ids.dim() != 2 or tuple(mask.shape) != tuple(ids.shape):
            raise ValueError(f"input_ids and attention_mask must be (P, L), got {tuple(ids.shape)}, "
                             f"{tuple(mask.shape)}")
        P, L = ids.shape
        if not (1 <= P <= 256 and 1 <= L <= 128):
            raise ValueError(f"the native text tower takes 1..256 prompts of 1..128 tokens, got {P} x {L}")
        ids = ids.to(self.device, torch.int32).contiguous()
        mask = mask.to(self.device, torch.int32).contiguous()
        out = torch.empty((P, TEXT_DIM), dtype=torch.float32, device=self.device)
        need = ctx.workspace_bytes(P, L)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        ctx.encode(ids.data_ptr(), mask.data_ptr(), P, L, normalize, out.data_ptr(), self._ws.data_ptr(),
                   self._ws.numel(), stream)
        self.calls += 1
        return out

    def embed(self, prompts: List[str], tokenizer, normalize: bool) -> torch.Tensor:
        inputs = tokenizer(list(prompts), padding=True, return_tensors="pt")
        return self.encode(inputs["input_ids"], inputs["attention_mask"], normalize)


class PromptEmbedder:
    def __init__(self, clap=None, tokenizer=None, table: Optional[Dict[str, np.ndarray]] = None,
                 native: Optional[NativeClapText] = None, native_source: Optional[str] = None):
        """`native`: a NativeClapText that computes the embeddings instead of `clap` (which may then be None).  Its
        branch is the reference's: L2-normalised `get_text_features` rows when the source is a ClapModel - the attached
        `clap`, or with none attached the declared `native_source` class name (default "ClapModel", what the
        reference's load_model builds) - and un-normalised `text_embeds` otherwise."""
        self.clap = clap
        self.tokenizer = tokenizer
        self.native = native
        self.native_source = native_source
        self.table: Dict[str, torch.Tensor] = {}
        self._from_clap: set = set()      # table entries computed by the CLAP model (invalidated on weight loads)
        if table:
            for k, v in table.items():
                self.table[k] = torch.as_tensor(np.asarray(v, dtype=np.float32)).reshape(-1)

    def load_clap_state(self, state: Dict[str, torch.Tensor]):
        """The `clap.*` part of a reference checkpoint, loaded into the CLAP model non-strictly as the reference's
        `model.load_state_dict(..., strict=False)` does for its `self.clap` submodule (`test_inference.py:34-35`).
        Embeddings computed with the previous weights are dropped.  Returns the number of tensors loaded.  With a
        native tower the same keys also go to it (a partial set of tower keys raises, listing the missing ones)."""
        if state and self.native is not None and any(k.startswith(("text_model.", "text_projection.")) for k in state):
            self.native.load_state_dict(state)
            for p in self._from_clap:
                self.table.pop(p, None)
            self._from_clap.clear()
        if not state or self.clap is None or not hasattr(self.clap, "load_state_dict"):
            return 0
        own = self.clap.state_dict() if hasattr(self.clap, "state_dict") else {}
        sub = {k: v for k, v in state.items() if k in own}    # a shape mismatch raises, as in torch's strict=False
        if sub:
            self.clap.load_state_dict(sub, strict=False)
            for p in self._from_clap:
                self.table.pop(p, None)
            self._from_clap.clear()
        return len(sub)

    @classmethod
    def synthetic(cls, seed: int = 7) -> "PromptEmbedder":
        t = synthetic_text_table(len(STEMS), seed=seed)
        return cls(table={s: t[i] for i, s in enumerate(STEMS)})

    def _native_normalize(self) -> bool:
        if self.clap is not None:
            return _is_clap_model(self.clap)
        return (self.native_source or "ClapModel") == "ClapModel"

    def _clap_embed(self, prompts: List[str]) -> torch.Tensor:
        if self.native is not None and self.tokenizer is not None:
            inputs = self.tokenizer(prompts, padding=True, return_tensors="pt")
            out = self.native.encode(inputs["input_ids"], inputs["attention_mask"], self._native_normalize())
            return out.float().cpu()
        if self.clap is None or self.tokenizer is None:
            raise KeyError(f"no embedding for prompts {prompts} and no CLAP model/tokenizer to compute one")
        inputs = self.tokenizer(prompts, padding=True, return_tensors="pt")
        params = getattr(self.clap, "parameters", None)
        dev = next(params()).device if params is not None else "cpu"
        inputs = {k: v.to(dev) for k, v in inputs.items()}
        with torch.no_grad():
            if _is_clap_model(self.clap):
                out = _text_features(self.clap.get_text_features(**inputs))
            else:                                             # ClapTextModelWithProjection (:245-248)
                out = self.clap.forward(**inputs).text_embeds
        if not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape[0] != len(prompts):
            raise ValueError(f"CLAP returned {type(out).__name__} {tuple(getattr(out, 'shape', ()))}, expected "
                             f"({len(prompts)}, {TEXT_DIM})")
        return out.float().cpu()

    def rows(self, text: Union[str, List[str]], batch: int) -> torch.Tensor:
        """(batch, 512) f32 CPU tensor for the reference's `text` argument (str broadcast or list of B)."""
        prompts = [text] * batch if isinstance(text, str) else list(text)
        if len(prompts) != batch:
            raise ValueError(f"{len(prompts)} prompts for a batch of {batch}")
        missing = sorted({p for p in prompts if p not in self.table})
        if missing:
            emb = self._clap_embed(missing)
            for p, e in zip(missing, emb):
                self.table[p] = e
                self._from_clap.add(p)
        out = torch.stack([self.table[p] for p in prompts])
        if out.shape != (batch, TEXT_DIM):
            raise ValueError(f"prompt embeddings must be {TEXT_DIM}-d (text_dim, config.yaml:16), got "
                             f"{tuple(out.shape[1:])}")
        return out


TEXT_DIM = 512


def _is_clap_model(m) -> bool:
    """`isinstance(self.clap, ClapModel)` of ATHTDemucs_v2.py:241 (by class name when transformers is absent)."""
    try:
        from transformers import ClapModel
        if isinstance(m, ClapModel):
            return True
    except ImportError:
        pass
    return any(c.__name__ == "ClapModel" for c in type(m).__mro__)


def _text_features(out) -> torch.Tensor:
    """`ClapModel.get_text_features` result -> (P, 512) projected, L2-normalised text features.  transformers 4.x
    (the reference's pin, requirements.txt:14) returns that tensor directly; transformers >= 5 returns a
    BaseModelOutputWithPooling whose `pooler_output` holds it (its `last_hidden_state` is the 768-d RoBERTa
    output, not an embedding)."""
    if isinstance(out, torch.Tensor):
        return out
    pooled = getattr(out, "pooler_output", None)
    if isinstance(pooled, torch.Tensor):
        return pooled
    emb = getattr(out, "text_embeds", None)
    if isinstance(emb, torch.Tensor):
        return emb
    raise TypeError(f"unrecognised get_text_features output {type(out).__name__}")
