"""The trainable half of the reference model as a plain torch module, fed by the native frozen half.

The reference trains only `text_attn`, `freq_decoder`, `time_decoder`, `freq_out` and `time_out` (`ATHTDemucs_v2.py:170-188`);
the HTDemucs encoders, the cross-transformer and CLAP run frozen under `no_grad` (`:277-279`).  `AudioTextHTDemucs.encode`
(athd/model.py, `athd_encode`) computes that frozen half in libathd.so; `TrainableHead` is the rest (`:21-139, 282-324`),
differentiable by autograd on any device and dtype; `HeadTrainer` joins the two behind the `model(mixture, prompts)`
call that `athd.train.train_epoch` expects.  The model's backward stays torch's, except for the output
stage (mask, iSTFT, denormalisation), which `native_output=True` runs natively in both directions (`NativeOutputStage`),
the text-conditioning stage, which `native_cond=True` does (`NativeCondStage`), the two decoders, which
`native_decoders=True` does level by level (`NativeDecoderLevel`), and what is left between them, which
`native_proj=True` does: the attention vector (`NativeAttnVector`) and `freq_out` / `time_out`, fused with the output
stage into one node (`NativeProjOutput`).  With all four options on, every forward and backward kernel of the head is the
library's; torch allocates the tensors and runs the Function plumbing.

`TrainableHead.state_dict()` has exactly the 50 reference key names and shapes outside `htdemucs.` / `clap.`
(`athd.weights.hot_path_spec`), so a trained head drops into a reference-format checkpoint and loads straight back into
the native inference path (`HeadTrainer.sync`).

Dead parameters.  The text cross-attention has ONE key (the prompt embedding), so its softmax is identically 1 and the
attention output does not depend on the query or the key.  `text_attn.q_proj.*`, `text_attn.k_proj.*`,
`text_attn.norm_q.*` and the query and key thirds of `text_attn.attn.in_proj_*` therefore get a mathematically zero
gradient (rounding leaves values around 1e-24 of the live gradients).  They stay parameters with `requires_grad=True`, as
in the reference: an optimizer with weight decay moves them exactly as it does there.  The native conditioning stage
never computes the query side; it hands these tensors exact zeros as gradients (`_DeadParams`), so `.grad` is a tensor,
not `None`, and such an optimizer does not skip them.
"""
from __future__ import annotations

import math
import weakref
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .model import EncodedFeatures
from .weights import DEC_CH, MODEL_DIM, TEXT_DIM, hot_path_spec

N_FFT, HOP = 4096, 1024


def head_keys():
    """[(key, shape)] of the 50 reference-owned tensors, in `hot_path_spec` order"""
    return [(k, tuple(s)) for k, s, _ in hot_path_spec() if not k.startswith("htdemucs.")]


class _TextAttention(nn.Module):
    """`ATHTDemucs_v2.py:21-58`: every feature row attends to the one prompt token, then a residual MLP and a LayerNorm"""

    def __init__(self, dim: int = MODEL_DIM, text_dim: int = TEXT_DIM, heads: int = 8):
        super().__init__()
        self.q_proj = nn.Linear(dim, dim)
        self.k_proj = nn.Linear(text_dim, dim)
        self.v_proj = nn.Linear(text_dim, dim)
        self.attn = nn.MultiheadAttention(dim, heads, batch_first=True)
        self.out_mlp = nn.Sequential(nn.Linear(dim, dim), nn.GELU(), nn.Linear(dim, dim))
        self.norm_q = nn.LayerNorm(dim)
        self.norm_out = nn.LayerNorm(dim)

    def rows(self, seq: torch.Tensor, text: torch.Tensor) -> torch.Tensor:
        """seq (B, N, D), text (B, 1, text_dim)"""
        q = self.q_proj(self.norm_q(seq))
        a, _ = self.attn(q, self.k_proj(text), self.v_proj(text), need_weights=False)
        u = seq + a
        return self.norm_out(u + self.out_mlp(u))

    def attn_vector(self, text: torch.Tensor) -> torch.Tensor:
        """text (B, text_dim) -> (B, D): what `attn` returns for every row when there is one key (the softmax is 1):
        out_proj(in_proj_v(v_proj(text))).  The slices hand the query and key thirds of `in_proj_*` exact zeros."""
        D = self.attn.embed_dim
        v = F.linear(text, self.v_proj.weight, self.v_proj.bias)
        v = F.linear(v, self.attn.in_proj_weight[2 * D:], self.attn.in_proj_bias[2 * D:])
        return F.linear(v, self.attn.out_proj.weight, self.attn.out_proj.bias)

    def dead_parameters(self):
        """the six tensors the output does not depend on (the query and key thirds of `in_proj_*` are the other dead
        values)"""
        return [self.q_proj.weight, self.q_proj.bias, self.k_proj.weight, self.k_proj.bias, self.norm_q.weight,
                self.norm_q.bias]

    def forward_native(self, x: torch.Tensor, xt: torch.Tensor, text_emb: torch.Tensor, nctx, native_vec: bool = False):
        """`forward` through `NativeCondStage`: x, xt contiguous float32 channel-first; float32 whatever autocast says.
        `native_vec`: the attention vector by `NativeAttnVector` instead of `attn_vector`'s three `F.linear`."""
        with torch.autocast(device_type=x.device.type, enabled=False):
            text = text_emb.reshape(text_emb.shape[0], -1).float()
            if native_vec:
                a = NativeAttnVector.apply(text, self.v_proj.weight, self.v_proj.bias, self.attn.in_proj_weight,
                                           self.attn.in_proj_bias, self.attn.out_proj.weight, self.attn.out_proj.bias,
                                           nctx)
            else:
                a = self.attn_vector(text)
            a = _DeadParams.apply(a, *self.dead_parameters())
            w = (self.out_mlp[0].weight, self.out_mlp[0].bias, self.out_mlp[2].weight, self.out_mlp[2].bias,
                 self.norm_out.weight, self.norm_out.bias)
            return NativeCondStage.apply(x, a, *w, nctx), NativeCondStage.apply(xt, a, *w, nctx)

    def forward(self, x: torch.Tensor, xt: torch.Tensor, text_emb: torch.Tensor):
        text = text_emb[:, None, :] if text_emb.dim() == 2 else text_emb
        B, C, Fr, Ts = x.shape
        xs = self.rows(x.flatten(2).transpose(1, 2), text)            # (B, Fr * Ts, C), frequency-major as the reference
        xts = self.rows(xt.transpose(1, 2), text)
        return xs.transpose(1, 2).reshape(B, C, Fr, Ts), xts.transpose(1, 2)


class _Decoder(nn.Module):
    """`ATHTDemucs_v2.py:61-139`: four ConvTranspose (k 8, s 4, p 2) levels along the frequency axis (freq) or time (time);
    GroupNorm(1) + GELU on all but the last; each level resized to its target length, then the encoder skip of that
    level (its first C_out channels, resized the same way) added times 0.1."""

    def __init__(self, freq: bool):
        super().__init__()
        self.freq = freq
        self.layers = nn.ModuleList()
        for i in range(len(DEC_CH) - 1):
            ci, co = DEC_CH[i], DEC_CH[i + 1]
            conv = (nn.ConvTranspose2d(ci, co, (8, 1), (4, 1), (2, 0)) if freq else nn.ConvTranspose1d(ci, co, 8, 4, 2))
            # index 0: the ConvT; index 1: the GroupNorm (absent on the last level), as the reference's key names
            self.layers.append(nn.Sequential(conv) if i == len(DEC_CH) - 2 else nn.Sequential(conv, nn.GroupNorm(1, co)))

    def _resize(self, x: torch.Tensor, n: int) -> torch.Tensor:
        if x.shape[2] == n:
            return x
        if self.freq:
            return F.interpolate(x, size=(n, x.shape[3]), mode="bilinear", align_corners=False)
        return F.interpolate(x, size=n, mode="linear", align_corners=False)

    def forward(self, x: torch.Tensor, skips: List[torch.Tensor], targets: List[int]) -> torch.Tensor:
        """skips / targets from the deepest level outwards"""
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if len(layer) > 1:
                x = F.gelu(x)
            if i < len(targets):
                x = self._resize(x, targets[i])
            if i < len(skips):
                x = x + 0.1 * self._resize(skips[i][:, :x.shape[1]], x.shape[2])
        return x

    def forward_native(self, x: torch.Tensor, skips: List[torch.Tensor], targets: List[int], nctx) -> torch.Tensor:
        """`forward` through `NativeDecoderLevel`, level by level on the channel-first layout as it is (no permute): x
        (B, 384, F, Ts) or (B, 384, L) float32; float32 whatever autocast says"""
        with torch.autocast(device_type=x.device.type, enabled=False):
            x = x.float().contiguous()
            for i, layer in enumerate(self.layers):
                conv, norm = layer[0], (layer[1] if len(layer) > 1 else None)
                co = conv.out_channels
                target = targets[i] if i < len(targets) else 4 * x.shape[2]
                skip = skips[i][:, :co].float().contiguous() if i < len(skips) else None
                x = NativeDecoderLevel.apply(x, conv.weight, conv.bias, norm.weight if norm is not None else None,
                                             norm.bias if norm is not None else None, skip, i, int(target), nctx)
        return x


class NativeDecoderLevel(torch.autograd.Function):
    """One decoder level in libathd.so, both directions (`athd_head_dec_level`, `athd_head_dec_level_backward`,
    include/athd.h): `x (B, Ci, M[, inner])` contiguous float32, the level's ConvTranspose weight and bias, its GroupNorm
    weight and bias (None on the last level) and the encoder skip `(B, Co, S[, inner])` (or None) -> `y (B, Co, Lt[,
    inner])` = resize(gelu(norm(convT(x)))) + 0.1 resize(skip).  The skip gets no gradient (it comes from the frozen
    half).  The backward recomputes the level from `x`: besides `x`, the parameters and the two statistics per item
    nothing is saved, none of the level's (Co, 4 M, inner) tensors; the workspace lives only inside each call."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, skip, level, target, nctx):
        B, _, M = x.shape[:3]
        inner = x.shape[3] if x.dim() == 4 else 1
        params = [p.detach().float().contiguous() if p is not None else None for p in (w, b, gamma, beta)]
        ptr = lambda t: t.data_ptr() if t is not None else None
        S = skip.shape[2] if skip is not None else 0
        y = torch.empty((B, w.shape[1], target) + tuple(x.shape[3:]), dtype=torch.float32, device=x.device)
        stats = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        ws = torch.empty(max(nctx.head_dec_workspace_bytes(level, B, M, inner, target), 16), dtype=torch.uint8,
                         device=x.device)
        nctx.head_dec_level(level, x.data_ptr(), *[ptr(p) for p in params], ptr(skip), B, M, inner, S, target,
                            y.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                            torch.cuda.current_stream(x.device).cuda_stream)
        ctx.save_for_backward(x, stats, *[p for p in params if p is not None])
        ctx.nctx, ctx.args = nctx, (level, B, M, inner, target)
        ctx.dtypes = [p.dtype if p is not None else None for p in (w, b, gamma, beta)]
        return y

    @staticmethod
    def backward(ctx, g):
        x, stats, w, b, *gn = ctx.saved_tensors
        gamma, beta = gn if gn else (None, None)
        level, B, M, inner, target = ctx.args
        g = g.float().contiguous()
        ptr = lambda t: t.data_ptr() if t is not None else None
        grads = [torch.empty_like(p) if p is not None else None for p in (x, w, b, gamma, beta)]
        ws = torch.empty(max(ctx.nctx.head_dec_workspace_bytes(level, B, M, inner, target), 16), dtype=torch.uint8,
                         device=g.device)
        ctx.nctx.head_dec_level_backward(level, g.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), ptr(gamma),
                                         ptr(beta), stats.data_ptr(), B, M, inner, target, *[ptr(t) for t in grads],
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream(g.device).cuda_stream)
        return (grads[0],) + tuple(t.to(d) if t is not None else None for t, d in zip(grads[1:], ctx.dtypes)) + (
            None, None, None, None)


class _DeadParams(torch.autograd.Function):
    """`a` unchanged, with the dead parameters attached to the graph: the backward hands each of them an exact zero
    tensor.  Without this the native conditioning stage, which never touches the query side, would leave their `.grad`
    at `None`, and an optimizer skips a parameter without a gradient, weight decay included."""

    @staticmethod
    def forward(ctx, a, *dead):
        ctx.save_for_backward(*dead)
        return a.view_as(a)

    @staticmethod
    def backward(ctx, g):
        return (g,) + tuple(torch.zeros_like(p) for p in ctx.saved_tensors)


class NativeAttnVector(torch.autograd.Function):
    """`_TextAttention.attn_vector` in libathd.so, both directions (`athd_head_attn_vec`, `athd_head_attn_vec_backward`,
    include/athd.h): `text (B, 512)` and the raw `v_proj`, `attn.in_proj_*` (whole) and `attn.out_proj` parameters ->
    `a (B, 384)`.  The backward writes whole-tensor gradients, the query and key thirds of `in_proj_*` as exact zeros (no
    slicing autograd); `text` gets no gradient.  Saved: `text` and the two (B, 384) intermediates."""

    @staticmethod
    def forward(ctx, text, wv, bv, w_in, b_in, wo, bo, nctx):
        B = text.shape[0]
        params = (wv, bv, w_in, b_in, wo, bo)
        t = [p.detach().float().contiguous() for p in (text,) + params]
        a = torch.empty((B, MODEL_DIM), dtype=torch.float32, device=text.device)
        keep = torch.empty((B, 2, MODEL_DIM), dtype=torch.float32, device=text.device)
        nctx.head_attn_vec(*[p.data_ptr() for p in t], B, a.data_ptr(), keep.data_ptr(),
                           torch.cuda.current_stream(text.device).cuda_stream)
        ctx.save_for_backward(t[0], keep, t[3], t[5])
        ctx.nctx, ctx.dtypes = nctx, [p.dtype for p in params]
        return a

    @staticmethod
    def backward(ctx, g):
        text, keep, w_in, wo = ctx.saved_tensors
        g = g.float().contiguous()
        D = MODEL_DIM
        shapes = ((D, text.shape[1]), (D,), (3 * D, D), (3 * D,), (D, D), (D,))
        grads = [torch.empty(sh, dtype=torch.float32, device=g.device) for sh in shapes]
        ctx.nctx.head_attn_vec_backward(g.data_ptr(), text.data_ptr(), keep.data_ptr(), w_in.data_ptr(), wo.data_ptr(),
                                        text.shape[0], *[t.data_ptr() for t in grads],
                                        torch.cuda.current_stream(g.device).cuda_stream)
        return (None,) + tuple(t.to(d) for t, d in zip(grads, ctx.dtypes)) + (None,)


class NativeProjOutput(torch.autograd.Function):
    """`freq_out`, `time_out` and the output stage as one node in libathd.so: `(xd (B, 4, Ts, Ts), xtd (B, 4, T))`, the
    decoders' channel-first outputs, -> `(B, 2, T)`.  Forward: `athd_head_proj` twice, straight into the layouts
    `athd_head_output` reads, then `athd_head_output`.  Backward: `athd_head_output_backward`, then
    `athd_head_proj_backward` on its `grad_logits` and on the incoming gradient itself (channel-first, scaled per item by
    `stdt` inside the kernel).  No permute, no copy and no elementwise torch op in between.  `spec`, `meant` and `stdt`
    get no gradient (they come from the frozen half).  Saved: the two inputs, the logits, `spec`, `stdt`, the two weights."""

    @staticmethod
    def forward(ctx, xd, xtd, wf, bf, wt, bt, spec, meant, stdt, nctx):
        B, _, R, S = xd.shape
        T = xtd.shape[2]
        dev = xd.device
        params = (wf, bf, wt, bt)
        wf_, bf_, wt_, bt_ = [p.detach().float().contiguous() for p in params]
        std = stdt.detach().reshape(B).float().contiguous()
        tnorm = torch.stack((meant.detach().reshape(B).float(), std), dim=1).contiguous()
        logits = torch.empty((B, S, R, 2), dtype=torch.float32, device=dev)
        xt = torch.empty((B, T, 2), dtype=torch.float32, device=dev)
        out = torch.empty((B, 2, T), dtype=torch.float32, device=dev)
        ws = torch.empty(max(nctx.head_output_workspace_bytes(B, T), 16), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        nctx.head_proj(xd.data_ptr(), wf_.data_ptr(), bf_.data_ptr(), B, R, S, logits.data_ptr(), stream)
        nctx.head_proj(xtd.data_ptr(), wt_.data_ptr(), bt_.data_ptr(), B, 1, T, xt.data_ptr(), stream)
        nctx.head_output(logits.data_ptr(), spec.data_ptr(), xt.data_ptr(), tnorm.data_ptr(), B, T, out.data_ptr(),
                         ws.data_ptr(), ws.numel(), stream)
        ctx.save_for_backward(xd, xtd, wf_, wt_, logits, spec, std)
        ctx.nctx, ctx.dtypes = nctx, [p.dtype for p in params]
        return out

    @staticmethod
    def backward(ctx, g):
        xd, xtd, wf, wt, logits, spec, std = ctx.saved_tensors
        B, _, R, S = xd.shape
        T = xtd.shape[2]
        nctx, dev = ctx.nctx, g.device
        g = g.float().contiguous()
        stream = torch.cuda.current_stream(dev).cuda_stream
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        grad_logits, gxd, gxtd = torch.empty_like(logits), torch.empty_like(xd), torch.empty_like(xtd)
        gwf, gbf, gwt, gbt = new(*wf.shape), new(2), new(*wt.shape), new(2)
        nws = max(nctx.head_proj_workspace_bytes(B, R, S), nctx.head_proj_workspace_bytes(B, 1, T), 16)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        nctx.head_output_backward(g.data_ptr(), logits.data_ptr(), spec.data_ptr(), B, T, grad_logits.data_ptr(), stream)
        nctx.head_proj_backward(grad_logits.data_ptr(), 0, None, xd.data_ptr(), wf.data_ptr(), B, R, S, gxd.data_ptr(),
                                gwf.data_ptr(), gbf.data_ptr(), ws.data_ptr(), nws, stream)
        # (the same stream orders the two calls, so they share the workspace)
        nctx.head_proj_backward(g.data_ptr(), 1, std.data_ptr(), xtd.data_ptr(), wt.data_ptr(), B, 1, T, gxtd.data_ptr(),
                                gwt.data_ptr(), gbt.data_ptr(), ws.data_ptr(), nws, stream)
        return (gxd, gxtd) + tuple(t.to(d) for t, d in zip((gwf, gbf, gwt, gbt), ctx.dtypes)) + (None, None, None, None)


class NativeCondStage(torch.autograd.Function):
    """The text-conditioning stage after the attention vector, in libathd.so, both directions (`athd_head_cond`,
    `athd_head_cond_backward`, include/athd.h): `x (B, 384, ...)` channel-first float32 as `athd_encode` exports it,
    `a (B, 384)` the attention output per item, `out_mlp.0`, `out_mlp.2` and `norm_out` -> `y` of x's shape =
    `norm_out(u + out_mlp(u))`, `u = x + a`.  `x` gets no gradient (it comes from the frozen half).  The backward
    recomputes the forward from `x`: besides `x`, `a` and the six parameters nothing is saved, no (rows x 384) tensor; its
    workspace lives only inside the backward call."""

    @staticmethod
    def forward(ctx, x, a, w0, b0, w2, b2, gamma, beta, nctx):
        B = x.shape[0]
        N = x.numel() // (B * MODEL_DIM)
        t = [p.detach().float().contiguous() for p in (a, w0, b0, w2, b2, gamma, beta)]
        y = torch.empty_like(x)
        nctx.head_cond(x.data_ptr(), *[p.data_ptr() for p in t], B, N, y.data_ptr(), 0, 0,
                       torch.cuda.current_stream(x.device).cuda_stream)
        ctx.save_for_backward(x, *t[:6])
        ctx.nctx, ctx.BN, ctx.dtypes = nctx, (B, N), [p.dtype for p in (a, w0, b0, w2, b2, gamma, beta)]
        return y

    @staticmethod
    def backward(ctx, g):
        x, a, w0, b0, w2, b2, gamma = ctx.saved_tensors
        B, N = ctx.BN
        g = g.float().contiguous()
        grads = [torch.empty_like(p) for p in (a, w0, b0, w2, b2, gamma, gamma)]
        ga, gw0, gb0, gw2, gb2, ggamma, gbeta = grads
        ws = torch.empty(max(ctx.nctx.head_cond_workspace_bytes(B, N), 16), dtype=torch.uint8, device=g.device)
        ctx.nctx.head_cond_backward(g.data_ptr(), x.data_ptr(), a.data_ptr(), w0.data_ptr(), b0.data_ptr(), w2.data_ptr(),
                                    b2.data_ptr(), gamma.data_ptr(), B, N, gw0.data_ptr(), gb0.data_ptr(), gw2.data_ptr(),
                                    gb2.data_ptr(), ggamma.data_ptr(), gbeta.data_ptr(), ga.data_ptr(), ws.data_ptr(),
                                    ws.numel(), torch.cuda.current_stream(g.device).cuda_stream)
        return (None,) + tuple(t.to(d) for t, d in zip(grads, ctx.dtypes)) + (None,)


class NativeOutputStage(torch.autograd.Function):
    """The output stage of `TrainableHead.forward` in libathd.so, both directions: `(xd (B, 2, Ts, Ts), xtd (B, 2, T))
    -> (B, 2, T)` = iSTFT(sigmoid mask on the spectrogram) + (xtd stdt + meant) by `athd_head_output` (the inference
    path's fused kernel, no 2048 x Ts intermediate in memory), and the gradient with respect to the logits by
    `athd_head_output_backward` (an STFT of the incoming gradient, include/athd.h).  The permutes to the kernels'
    frame-major layouts are torch's.  `spec` is `athd_pack_spectrum` of the features' `z`; it, `meant` and `stdt` get no
    gradient (they come from the frozen half)."""

    @staticmethod
    def forward(ctx, xd, xtd, spec, meant, stdt, nctx):
        B, _, T = xtd.shape
        # (.float(): under autocast the 1x1 convolutions hand over half-precision tensors)
        logits = xd.detach().float().permute(0, 3, 2, 1).contiguous()      # (B, frame, row, channel)
        xt = xtd.detach().float().transpose(1, 2).contiguous()             # (B, T, 2)
        tnorm = torch.stack((meant.reshape(B), stdt.reshape(B)), dim=1).float().contiguous()
        out = torch.empty((B, 2, T), dtype=torch.float32, device=xd.device)
        ws = torch.empty(max(nctx.head_output_workspace_bytes(B, T), 16), dtype=torch.uint8, device=xd.device)
        stream = torch.cuda.current_stream(xd.device).cuda_stream
        nctx.head_output(logits.data_ptr(), spec.data_ptr(), xt.data_ptr(), tnorm.data_ptr(), B, T, out.data_ptr(),
                         ws.data_ptr(), ws.numel(), stream)
        ctx.save_for_backward(logits, spec, stdt)
        ctx.nctx, ctx.T, ctx.dtypes = nctx, T, (xd.dtype, xtd.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        logits, spec, stdt = ctx.saved_tensors
        g = g.float().contiguous()
        grad_logits = torch.empty_like(logits)
        ctx.nctx.head_output_backward(g.data_ptr(), logits.data_ptr(), spec.data_ptr(), logits.shape[0], ctx.T,
                                      grad_logits.data_ptr(), torch.cuda.current_stream(g.device).cuda_stream)
        return (grad_logits.permute(0, 3, 2, 1).to(ctx.dtypes[0]), (g * stdt.reshape(-1, 1, 1)).to(ctx.dtypes[1]), None,
                None, None, None)


class TrainableHead(nn.Module):
    """(EncodedFeatures, text_emb (B, 512)) -> (B, 2, T): text conditioning, both decoders, the sigmoid mask on the
    mixture's spectrogram, the inverse STFT and the time branch's denormalisation, summed (`ATHTDemucs_v2.py:282-324`).
    Computes in the dtype of its parameters (features are cast to it).

    `native_output=True` runs the last stage (mask, iSTFT, denormalisation) and its gradient in libathd.so
    (`NativeOutputStage`) instead of as torch ops.  It needs the native model for its context (`bind`; `HeadTrainer`
    does that), float32 parameters on the model's GPU and at most 2048 frames, and raises otherwise: a float64 or CPU
    head uses the torch stage by leaving the option off, never by a silent fallback.

    `native_cond=True` does the same for the first stage, the text conditioning (`NativeCondStage`: the residual MLP and
    LayerNorm on the features' channel-first layout, no permute, and their gradients; the attention vector per item stays
    torch's).  Same requirements (bound model, float32 parameters on its GPU) plus contiguous float32 features on that
    GPU, as `encode` returns them; it raises otherwise.  Under autocast it computes and returns float32.

    `native_decoders=True` does the same for both decoders (`NativeDecoderLevel`, four levels each, on the conditioned
    features' channel-first layout as it is; `freq_out` / `time_out` stay torch's).  Same requirements and refusals as
    `native_cond` (bound model, float32 parameters on its GPU, float32 features and skips on that GPU); float32 under
    autocast.  The three options are independent and compose; with all three on torch's autograd is left with
    `freq_out` / `time_out` and the attention vector, unless `native_proj` is on as well.

    `native_proj=True` does the same for what is left: the attention vector (`NativeAttnVector`) and `freq_out` /
    `time_out`, which become one node with the output stage (`NativeProjOutput`).  Its inputs and outputs exist only in
    those stages' layouts, so it needs `native_output` and `native_cond` to be on, and what they need; it raises
    otherwise, and when a decoder emits another length than the segment's (the torch resize is not kept inside).  It is
    independent of `native_decoders` (torch's channel-first decoder output is taken after `.float().contiguous()`);
    float32 under autocast.  With it the six wholly dead tensors keep their exact-zero gradients (`_DeadParams`)."""

    def __init__(self, native_output: bool = False, native_cond: bool = False, native_decoders: bool = False,
                 native_proj: bool = False):
        super().__init__()
        self.text_attn = _TextAttention()
        self.freq_decoder = _Decoder(True)
        self.time_decoder = _Decoder(False)
        self.freq_out = nn.Conv2d(DEC_CH[-1], 2, 1)
        self.time_out = nn.Conv1d(DEC_CH[-1], 2, 1)
        self.native_output = bool(native_output)
        self.native_cond = bool(native_cond)
        self.native_decoders = bool(native_decoders)
        self.native_proj = bool(native_proj)
        object.__setattr__(self, "_native_model", None)      # a plain attribute, not a submodule
        object.__setattr__(self, "_spec_cache", None)        # (weakref to z, its version, packed spectrum)

    def bind(self, model) -> "TrainableHead":
        """The native `AudioTextHTDemucs` whose context (FFT and window tables, dtype) the native output stage uses.  The
        context is looked up per call, so `HeadTrainer.sync()` (which re-finalises it) needs no re-binding."""
        object.__setattr__(self, "_native_model", model)
        return self

    def packed_spectrum(self, z: torch.Tensor) -> torch.Tensor:
        """`athd_pack_spectrum` of an `EncodedFeatures.z`, (B, Ts, 2048, 4) float32; computed once per `z` tensor (the
        last one is kept, keyed on the tensor's identity and version)"""
        c = self._spec_cache
        if c is not None and c[0]() is z and c[1] == z._version:
            return c[2]
        B, _, _, Ts = z.shape
        zr = torch.view_as_real(z).contiguous()
        spec = torch.empty((B, Ts, 2048, 4), dtype=torch.float32, device=z.device)
        self._native_model._ensure_ctx().pack_spectrum(zr.data_ptr(), B, Ts, spec.data_ptr(),
                                                       torch.cuda.current_stream(z.device).cuda_stream)
        object.__setattr__(self, "_spec_cache", (weakref.ref(z), z._version, spec))
        return spec

    def _check_native_output(self, f: EncodedFeatures, opt: str = "native_output=True"):
        model, p = self._native_model, self.freq_out.weight
        if model is None:
            raise RuntimeError(f"{opt} needs the native model: call head.bind(model) (HeadTrainer does)")
        if p.dtype != torch.float32 or p.device.type != "cuda" or p.device != model.device:
            raise RuntimeError(f"{opt} needs float32 parameters on the model's device {model.device}, got "
                               f"{p.dtype} on {p.device}; leave the option off for the torch output stage")
        z = f.z
        if z.dtype != torch.complex64 or z.device != p.device or z.shape[1:3] != (2, 2048):
            raise RuntimeError(f"{opt} needs the features' z as complex64 (B, 2, 2048, Ts) on the model's "
                               "device")
        if z.shape[3] > 2048 or z.shape[3] != -(-f.length // HOP):
            raise RuntimeError(f"{opt} covers segments of at most 2048 frames, got {z.shape[3]} frames "
                               f"for {f.length} samples")

    def _native_stage(self, f: EncodedFeatures, xd: torch.Tensor, xtd: torch.Tensor) -> torch.Tensor:
        model = self._native_model
        self._check_native_output(f)
        return NativeOutputStage.apply(xd, xtd, self.packed_spectrum(f.z), self._cast(f.meant), self._cast(f.stdt),
                                       model._ensure_ctx())

    def _check_native_proj(self):
        model, p = self._native_model, self.time_out.weight
        if not (self.native_output and self.native_cond):
            raise RuntimeError("native_proj=True needs native_output=True and native_cond=True: its inputs and outputs "
                               "exist only in those stages' layouts")
        if model is None:
            raise RuntimeError("native_proj=True needs the native model: call head.bind(model) (HeadTrainer does)")
        if p.dtype != torch.float32 or p.device.type != "cuda" or p.device != model.device:
            raise RuntimeError(f"native_proj=True needs float32 parameters on the model's device {model.device}, got "
                               f"{p.dtype} on {p.device}; leave the option off for the torch projections")

    def _native_proj_stage(self, f: EncodedFeatures, xd: torch.Tensor, xtd: torch.Tensor) -> torch.Tensor:
        """`freq_out`, `time_out` and the output stage on the decoders' outputs xd (B, 4, Ts, Ts), xtd (B, 4, T)"""
        p = self.freq_out.weight
        self._check_native_output(f, "native_proj=True")
        B, Ts, T = f.z.shape[0], f.z.shape[3], f.length
        if tuple(xd.shape) != (B, DEC_CH[-1], Ts, Ts):
            raise RuntimeError(f"native_proj=True needs the frequency decoder's output as (B, {DEC_CH[-1]}, {Ts}, {Ts}), "
                               f"got {tuple(xd.shape)}")
        if tuple(xtd.shape) != (B, DEC_CH[-1], T):
            raise RuntimeError(f"native_proj=True needs the time decoder to emit the segment's length {T}, got "
                               f"{tuple(xtd.shape)}: the resize in front of the output stage is not part of it")
        with torch.autocast(device_type=p.device.type, enabled=False):
            return NativeProjOutput.apply(xd.float().contiguous(), xtd.float().contiguous(), self.freq_out.weight,
                                          self.freq_out.bias, self.time_out.weight, self.time_out.bias,
                                          self.packed_spectrum(f.z), self._cast(f.meant), self._cast(f.stdt),
                                          self._native_model._ensure_ctx())

    def _native_cond_stage(self, f: EncodedFeatures, text_emb: torch.Tensor):
        model, p = self._native_model, self.text_attn.norm_out.weight
        if model is None:
            raise RuntimeError("native_cond=True needs the native model: call head.bind(model) (HeadTrainer does)")
        if p.dtype != torch.float32 or p.device.type != "cuda" or p.device != model.device:
            raise RuntimeError(f"native_cond=True needs float32 parameters on the model's device {model.device}, got "
                               f"{p.dtype} on {p.device}; leave the option off for the torch conditioning stage")
        for name, t in (("x_enc", f.x_enc), ("xt_enc", f.xt_enc)):
            if (t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous() or t.dim() < 3
                    or t.shape[1] != MODEL_DIM or t.numel() == 0):
                raise RuntimeError(f"native_cond=True needs the features' {name} as contiguous float32 (B, {MODEL_DIM}, "
                                   f"...) on the model's device, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return self.text_attn.forward_native(f.x_enc, f.xt_enc, text_emb.to(p.device), model._ensure_ctx(),
                                             native_vec=self.native_proj)

    def _native_decoder_stage(self, f: EncodedFeatures, x_cond: torch.Tensor, xt_cond: torch.Tensor):
        model, p = self._native_model, self.freq_decoder.layers[0][0].weight
        if model is None:
            raise RuntimeError("native_decoders=True needs the native model: call head.bind(model) (HeadTrainer does)")
        if p.dtype != torch.float32 or p.device.type != "cuda" or p.device != model.device:
            raise RuntimeError(f"native_decoders=True needs float32 parameters on the model's device {model.device}, got "
                               f"{p.dtype} on {p.device}; leave the option off for the torch decoders")
        feats = [("x_enc", f.x_enc), ("xt_enc", f.xt_enc)]
        feats += [(f"skips[{i}]", t) for i, t in enumerate(f.skips)] + [(f"skips_t[{i}]", t)
                                                                        for i, t in enumerate(f.skips_t)]
        for name, t in feats:
            if t.dtype != torch.float32 or t.device != p.device or t.dim() < 3 or t.numel() == 0:
                raise RuntimeError(f"native_decoders=True needs the features' {name} as float32 (B, C, ...) on the "
                                   f"model's device, got {t.dtype} {tuple(t.shape)} on {t.device}")
        nctx = model._ensure_ctx()
        xd = self.freq_decoder.forward_native(x_cond, list(f.skips[::-1]), list(f.lengths[::-1]), nctx)
        xtd = self.time_decoder.forward_native(xt_cond, list(f.skips_t[::-1]), list(f.lengths_t[::-1]), nctx)
        return xd, xtd

    @classmethod
    def from_model(cls, model) -> "TrainableHead":
        """The 50 head tensors of a loaded `AudioTextHTDemucs` (float32, on the CPU; move it with `.to`)"""
        head = cls()
        head.load_state_dict({k: torch.as_tensor(model._weights[k]).clone() for k, _ in head_keys()}, strict=True)
        return head

    def _ispec(self, z: torch.Tensor, length: int) -> torch.Tensor:
        """demucs' `_ispec`: one zero bin on top, two zero frames on each side, the normalised Hann iSTFT, the crop"""
        B, C, Fr, Ts = z.shape
        z = F.pad(F.pad(z, (0, 0, 0, 1)), (2, 2))
        pad = HOP // 2 * 3
        le = HOP * int(math.ceil(length / HOP)) + 2 * pad
        # the window is built in float32 and then cast, as demucs' `ispectro` does (`hann_window(n_fft).to(z.real)`): in
        # float64 a window built there directly differs from it at 1e-8, which shows as 150 dB against the oracle
        win = torch.hann_window(N_FFT).to(device=z.device, dtype=z.real.dtype)
        x = torch.istft(z.reshape(B * C, Fr + 1, Ts + 4), N_FFT, HOP, window=win, win_length=N_FFT, normalized=True,
                        length=le, center=True)
        return x.reshape(B, C, le)[..., pad:pad + length]

    def _cast(self, t: torch.Tensor) -> torch.Tensor:
        p = self.freq_out.weight
        return t.to(device=p.device, dtype=p.dtype)

    def decoded(self, f: EncodedFeatures, text_emb: torch.Tensor):
        """(x_cond, xt_cond, freq_decoder(..), time_decoder(..)): everything before `freq_out` / `time_out`"""
        cast = self._cast
        if self.native_proj:
            self._check_native_proj()
        if self.native_cond:
            x_cond, xt_cond = self._native_cond_stage(f, text_emb)
        else:
            x_cond, xt_cond = self.text_attn(cast(f.x_enc), cast(f.xt_enc), cast(text_emb))
        # frequency branch: logits on a (Ts, Ts) grid (the reference resizes the FREQUENCY axis to `lengths`, the frame
        # counts)
        if self.native_decoders:
            xd, xtd = self._native_decoder_stage(f, x_cond, xt_cond)
        else:
            xd = self.freq_decoder(x_cond, [cast(s) for s in f.skips[::-1]], list(f.lengths[::-1]))
            xtd = self.time_decoder(xt_cond, [cast(s) for s in f.skips_t[::-1]], list(f.lengths_t[::-1]))
        return x_cond, xt_cond, xd, xtd

    def branches(self, f: EncodedFeatures, text_emb: torch.Tensor):
        """(x_cond, xt_cond, freq_out(freq_decoder(..)), time_out(time_decoder(..))): everything before the mask, the
        two projections as torch's channel-first convolutions whatever `native_proj` says"""
        x_cond, xt_cond, xd, xtd = self.decoded(f, text_emb)
        return x_cond, xt_cond, self.freq_out(xd), self.time_out(xtd)

    def forward(self, f: EncodedFeatures, text_emb: torch.Tensor) -> torch.Tensor:
        p = self.freq_out.weight
        cast = self._cast
        if self.native_proj:
            _, _, xd, xtd = self.decoded(f, text_emb)
            return self._native_proj_stage(f, xd, xtd)
        _, _, xd, xtd = self.branches(f, text_emb)
        if self.native_output:
            # (the time branch's resize, when the head emits another length, stays torch's, in front of the Function)
            if xtd.shape[-1] != f.length:
                xtd = F.interpolate(xtd, size=f.length, mode="linear", align_corners=False)
            return self._native_stage(f, xd, xtd)
        z = f.z.to(device=p.device, dtype=torch.complex128 if p.dtype == torch.float64 else torch.complex64)
        # the logits stretched to the spectrogram's (2048, Ts)
        mask = torch.sigmoid(F.interpolate(xd, size=(z.shape[2], z.shape[3]), mode="bilinear", align_corners=False))
        # `mag[:, :2]` of the complex-as-channels magnitude is (Re, Im) of the LEFT channel: kept as the reference has it
        mag_stereo = torch.stack((z[:, 0].real, z[:, 0].imag), dim=1)
        phase = z / (mag_stereo + 1e-8)
        freq_wav = self._ispec((mag_stereo * mask) * phase, f.length)
        # time branch
        if xtd.shape[-1] != f.length:
            xtd = F.interpolate(xtd, size=f.length, mode="linear", align_corners=False)
        return freq_wav + (xtd * cast(f.stdt) + cast(f.meant))


class HeadTrainer(nn.Module):
    """`model(mixture, prompts)` for `athd.train.train_epoch`: the native frozen half, then the torch head.  The native
    model is a plain attribute (not a submodule): `parameters()`, `train()` and `eval()` are the head's."""

    def __init__(self, model, head: Optional[TrainableHead] = None, native_output: bool = False,
                 native_cond: bool = False, native_decoders: bool = False, native_proj: bool = False):
        super().__init__()
        object.__setattr__(self, "model", model)
        if head is None:
            if model.device is None:
                model.to("cuda")
            head = TrainableHead.from_model(model).to(model.device)
        # native_output / native_cond / native_decoders / native_proj: the head's last / first / middle stage and the
        # projections between them, with their gradients, in libathd.so (TrainableHead); a head that was built with an
        # option keeps it.  Only such a head holds a reference to the native model.
        head.native_output = bool(native_output or head.native_output)
        head.native_cond = bool(native_cond or head.native_cond)
        head.native_decoders = bool(native_decoders or head.native_decoders)
        head.native_proj = bool(native_proj or head.native_proj)
        if head.native_output or head.native_cond or head.native_decoders or head.native_proj:
            head.bind(model)
        self.head = head

    def forward(self, mixture: torch.Tensor, prompts) -> torch.Tensor:
        feats = self.model.encode(mixture)
        emb = self.model.embedder.rows(prompts, mixture.shape[0])
        return self.head(feats, emb)

    def state_dict(self, *args, **kwargs):
        """the head's 50 reference keys (no `head.` prefix)"""
        return self.head.state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict: bool = True):
        return self.head.load_state_dict(state_dict, strict=strict)

    def sync(self):
        """Load the head's current weights into the native model.  This re-finalises the native context (weights are
        packed again), so call it once per validation, not per step."""
        self.model.load_state_dict(self.head.state_dict())
        return self
