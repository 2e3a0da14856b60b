"""References for head training's native decoder level (csrc/head_dec.hip, include/athd.h `athd_head_dec_level*`); a helper
module of tests/test_head_dec_refs.py and tests/test_gpu_head_dec.py, not a test file.

  * `case`: seeded inputs of one level (weights about 0.05 randn, GroupNorm weights near 1, an incoming gradient `gy` with
    a per-item power-of-two scale); every value is float32-representable;
  * `torch_level`: one level of `_Decoder` itself (its ConvTranspose2d / GroupNorm modules, `F.gelu`, its `_resize` and
    the scaled skip, the frequency decoder's ops with `inner` columns), in any dtype and on any device; `autograd`
    differentiates `sum(y * gy)` through it;
  * `closed_form`: the level as include/athd.h states it, in numpy, float64 or float32.  The float32 variant follows the
    kernel's sequence of operations (both taps of a position in one product, then the bias; the mean, then the variance
    of the centred values; 1 / sqrt; torch's resize rule in the working precision; the resize's adjoint gathered per
    source position; `r (D - mean D - ch mean(D ch))`), with numpy's own order inside each sum.  `mut` plants the defects
    the tests' bound must separate;
  * `gap`: the worst |got - want| over the tensor's largest |want|.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from athd.head import _Decoder

LEVELS = [(384, 192), (192, 96), (96, 48), (48, 4)]          # (Ci, Co)
# (level, B, M, inner, Lt, S)
CASES = [
    (0, 1, 1, 1, 4, 1),          # one input position; Lt == 4 M and a one-position skip: blind to align_corners
    (3, 2, 70, 1, 280, 70),      # no norm (blind to the GELU and GroupNorm defects), no resize of h (the skip is
                                 # resized 4x), a token tile boundary crossed with inner = 1
    (0, 2, 16, 1, 63, 16),       # near-identity resize 64 -> 63, skip upsampled about 4x
    (1, 2, 63, 1, 250, 63),      # near-identity resize 252 -> 250
    (0, 2, 8, 5, 5, 8),          # downsample 32 -> 5, rows not 16-byte aligned
    (1, 1, 5, 5, 5, 32),         # resize 20 -> 5, skip 32 -> 5
    (0, 1, 8, 37, 37, 8),        # upsample 32 -> 37; the halo of 37 tokens crosses tiles
    (2, 2, 37, 37, 37, 128),     # 1369 tokens per item: 11 column tiles, 86 K steps of dW per item against 32 slices
    (3, 1, 37, 37, 37, 512),     # skip downsampled 512 -> 37; no norm
    (0, 1, 1, 3, 1, 8),          # Lt = 1
    (0, 2, 40, 5, 150, 40),      # 200 tokens per item: 13 K steps of dW per item against 8 slices, a slice and a K step
                                 # that straddle the two items; resize 160 -> 150, skip 40 -> 150
    (1, 1, 3, 2, 192, 3),        # upsample 16x (12 -> 192): the adjoint gathers about 32 outputs per source position
]
ALLOW = 4.0          # a float32 evaluation may sit at this many times the reference's own f32-against-f64 gap
MUTS = ["tanh_gelu", "gn_no_proj", "align_corners", "unscaled_skip", "taps_swapped"]


def names(level):
    """the output, then the gradients, in `athd_head_dec_level_backward`'s order"""
    return ["y", "x", "w", "b"] + (["gamma", "beta"] if level < 3 else [])


def blind(shape, mut):
    """True where the case cannot see the defect at all"""
    level, B, M, inner, Lt, S = shape
    if mut in ("tanh_gelu", "gn_no_proj"):
        return level == 3
    if mut == "align_corners":
        return Lt == 4 * M and (S == Lt or S <= 1)
    return False


def case(level, B, M, inner, Lt, S, seed=0):
    """dict of float64 CPU tensors: x (B, Ci, M, inner), w (Ci, Co, 8, 1), b, gamma, beta (Co), skip (B, Co, S, inner),
    gy (B, Co, Lt, inner)"""
    Ci, Co = LEVELS[level]
    g = torch.Generator().manual_seed(9000 + 131 * seed + 1009 * level + 17 * B + 7 * M + 3 * inner + Lt)
    r32 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    f32 = lambda t: t.float().double()
    gy = r32(B, Co, Lt, inner) * torch.as_tensor(np.ldexp(1.0, np.arange(B) % 3 - 1)).reshape(B, 1, 1, 1)
    return dict(level=level, B=B, M=M, inner=inner, Lt=Lt, S=S, x=r32(B, Ci, M, inner), w=f32(0.05 * r32(Ci, Co, 8, 1)),
                b=f32(0.05 * r32(Co)), gamma=f32(1.0 + 0.1 * r32(Co)), beta=f32(0.05 * r32(Co)), skip=r32(B, Co, S, inner),
                gy=gy)


@functools.lru_cache(maxsize=None)
def _decoder(dtype, device):
    return _Decoder(True).to(device=device, dtype=dtype)


def torch_level(dec, level, x, skip, Lt):
    """level `level` of `_Decoder.forward` on x (B, Ci, M, inner) with the skip (B, Co, S, inner) and target length Lt"""
    layer = dec.layers[level]
    y = layer(x)
    if len(layer) > 1:
        y = F.gelu(y)
    y = dec._resize(y, Lt)
    return y + 0.1 * dec._resize(skip[:, :y.shape[1]], y.shape[2])


def autograd(c, dtype, device="cpu"):
    """{name: float64 numpy} of names(level) for L = sum(y * gy) through `torch_level` in `dtype` on `device`"""
    dec = _decoder(dtype, device)
    layer = dec.layers[c["level"]]
    to = lambda t: t.to(device=device, dtype=dtype)
    with torch.no_grad():
        layer[0].weight.copy_(to(c["w"]))
        layer[0].bias.copy_(to(c["b"]))
        if len(layer) > 1:
            layer[1].weight.copy_(to(c["gamma"]))
            layer[1].bias.copy_(to(c["beta"]))
    dec.zero_grad()
    x = to(c["x"]).detach().clone().requires_grad_(True)
    y = torch_level(dec, c["level"], x, to(c["skip"]), c["Lt"])
    y.backward(to(c["gy"]))
    n = lambda t: t.detach().double().cpu().numpy()
    out = dict(y=n(y), x=n(x.grad), w=n(layer[0].weight.grad), b=n(layer[0].bias.grad))
    if len(layer) > 1:
        out.update(gamma=n(layer[1].weight.grad), beta=n(layer[1].bias.grad))
    return out


_erf = np.vectorize(math.erf, otypes=[np.float64])


def lin(n_in, n_out, R, align=False):
    """torch's linear resize rule n_in -> n_out in precision R: (i0, i1, w0, w1) per output position"""
    l = np.arange(n_out).astype(R)
    if align:
        scale = R(n_in - 1) / R(n_out - 1) if n_out > 1 else R(0)
        src = (scale * l).astype(R)
    else:
        scale = R(n_in) / R(n_out)
        src = np.maximum((scale * (l + R(0.5))).astype(R) - R(0.5), R(0)).astype(R)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = np.clip((src - i0.astype(R)).astype(R), R(0), R(1))
    return i0, i1, (R(1) - w1).astype(R), w1


def closed_form(c, dtype=np.float64, mut=None):
    """{name: float64 numpy} of names(level) by the closed form.  mut: one of MUTS"""
    R = dtype
    level, B, M, inner, Lt, S = (c[k] for k in ("level", "B", "M", "inner", "Lt", "S"))
    Ci, Co = LEVELS[level]
    norm = level < 3
    n_ = lambda k: c[k].numpy().astype(R)
    X, W, bias, gamma, beta, SK, GY = n_("x"), n_("w").reshape(Ci, Co, 8), n_("b"), n_("gamma"), n_("beta"), n_("skip"), \
        n_("gy")
    Wf = W[:, :, [4, 5, 6, 7, 0, 1, 2, 3]] if mut == "taps_swapped" else W      # the forward's taps; the backward's stay
    align = mut == "align_corners"
    i0, i1, w0, w1 = lin(4 * M, Lt, R, align)
    s0, s1, v0, v1 = lin(S, Lt, R, align)
    col = lambda v: v[None, :, None]
    out = dict(y=np.zeros((B, Co, Lt, inner)), x=np.zeros((B, Ci, M, inner)))
    gw = np.zeros((B, Ci, Co, 8), dtype=R)
    gb, gg, gbe = (np.zeros((B, Co), dtype=R) for _ in range(3))
    for b in range(B):
        x2 = X[b].reshape(Ci, M * inner)
        pad = np.zeros((Co, 4 * M + 4, inner), dtype=R)                          # position o sits at o + 2 = 4 m + k
        for k in range(8):
            pad[:, k:k + 4 * M:4] += (Wf[:, :, k].T @ x2).astype(R).reshape(Co, M, inner)
        cc = (pad[:, 2:4 * M + 2] + bias[:, None, None]).astype(R)
        if norm:
            mu = R(cc.sum(dtype=R) / R(cc.size))
            d = (cc - mu).astype(R)
            r = R(1) / np.sqrt(R((d * d).sum(dtype=R) / R(cc.size)) + R(1e-5))
            ch = (d * r).astype(R)
            z = (gamma[:, None, None] * ch + beta[:, None, None]).astype(R)
            if mut == "tanh_gelu":
                k0, k1 = R(math.sqrt(2.0 / math.pi)), R(0.044715)
                th = np.tanh(k0 * (z + k1 * z * z * z)).astype(R)
                h = (R(0.5) * z * (R(1) + th)).astype(R)
                gp = (R(0.5) * (R(1) + th) + R(0.5) * z * (R(1) - th * th) * k0 * (R(1) + R(3) * k1 * z * z)).astype(R)
            else:
                cdf = (R(0.5) * (R(1) + _erf(z * R(math.sqrt(0.5))).astype(R))).astype(R)
                h = (z * cdf).astype(R)
                gp = (cdf + z * (R(1.0 / math.sqrt(2.0 * math.pi)) * np.exp(R(-0.5) * z * z).astype(R))).astype(R)
        else:
            h = cc
        y = (col(w0) * h[:, i0] + col(w1) * h[:, i1]).astype(R)
        sk = (col(v0) * SK[b][:, s0] + col(v1) * SK[b][:, s1]).astype(R)
        out["y"][b] = y + (R(1.0) if mut == "unscaled_skip" else R(0.1)) * sk
        # the adjoint of the resize, gathered per source position
        dh = np.zeros((4 * M, Co, inner), dtype=R)
        gyt = GY[b].transpose(1, 0, 2)
        np.add.at(dh, i0, (w0[:, None, None] * gyt).astype(R))
        np.add.at(dh, i1, (w1[:, None, None] * gyt).astype(R))
        dh = dh.transpose(1, 0, 2)
        if norm:
            dz = (dh * gp).astype(R)
            gg[b] = (dz * ch).sum(axis=(1, 2), dtype=R)
            gbe[b] = dz.sum(axis=(1, 2), dtype=R)
            D = (gamma[:, None, None] * dz).astype(R)
            m1 = R(D.sum(dtype=R) / R(D.size))
            m2 = R((D * ch).sum(dtype=R) / R(D.size))
            dc = (r * (D - m1 - (ch * m2 if mut != "gn_no_proj" else R(0)))).astype(R)
        else:
            dc = dh.astype(R)
        gb[b] = dc.sum(axis=(1, 2), dtype=R)
        dpad = np.zeros((Co, 4 * M + 4, inner), dtype=R)
        dpad[:, 2:4 * M + 2] = dc
        dx = np.zeros((Ci, M * inner), dtype=R)
        for k in range(8):
            Dk = np.ascontiguousarray(dpad[:, k:k + 4 * M:4][:, :M]).reshape(Co, M * inner)
            gw[b, :, :, k] = (x2 @ Dk.T).astype(R)
            dx = (dx + (W[:, :, k] @ Dk).astype(R)).astype(R)
        out["x"][b] = dx.reshape(Ci, M, inner)
    tot = lambda a: functools.reduce(lambda s, v: (s + v).astype(R), list(a))    # the items in order
    out.update(w=tot(gw).reshape(Ci, Co, 8, 1), b=tot(gb))
    if norm:
        out.update(gamma=tot(gg), beta=tot(gbe))
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def gap(got, want):
    """max |got - want| / max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def gaps(got, want):
    return {k: gap(got[k], want[k]) for k in want}


def ratios(g, a):
    """gap over allowance unit per tensor; a tensor torch's float32 hits exactly must be hit exactly"""
    return {k: (g[k] / a[k] if a[k] > 0 else (0.0 if g[k] == 0 else float("inf"))) for k in a}


@functools.lru_cache(maxsize=None)
def refs(shape):
    """(case, float64 autograd, torch-CPU's own f32-against-f64 gap per tensor) of a CASES entry, computed once and shared
    by the tests.  Treat the arrays as read-only."""
    c = case(*shape)
    g64 = autograd(c, torch.float64)
    return c, g64, gaps(autograd(c, torch.float32), g64)
