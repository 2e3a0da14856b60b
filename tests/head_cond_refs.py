"""References for head training's native text-conditioning stage (csrc/head_cond.hip, include/athd.h `athd_head_cond*`); a
helper module of tests/test_head_cond_refs.py and tests/test_gpu_head_cond.py, not a test file.

  * `case`: a seeded `_TextAttention` (weights about 0.05 randn, LayerNorm weights near 1), features `x` (B, 384, N)
    channel-first, a prompt embedding per item and an incoming gradient `gy` with a per-item power-of-two scale; every
    value is float32-representable;
  * `torch_stage`: `_TextAttention.rows` itself (the full `nn.MultiheadAttention` over every row), in any dtype and on
    any device; `autograd` differentiates `sum(y * gy)` through it;
  * `closed_form`: the stage as include/athd.h states it, in numpy, float64 or float32.  The float32 variant follows the
    kernel's sequence of operations (two-pass LayerNorm statistics, 1 / sqrt, `r (D - mean D - Vh mean(D Vh))`, token
    sums per 64-token tile, then per item, then over the items), with numpy's own order inside each matrix product.
    `mut` plants the defects the tests' bound must separate;
  * `gap`: the worst |got - want| over the tensor's largest |want|.
"""
import functools
import math

import numpy as np
import torch

from athd.head import _TextAttention

C, TEXT = 384, 512
TN = 64                                     # the kernel's token tile
# (B, N): one column; one full tile per item; a ragged tail (70 = 64 + 6: items share no tile); an odd N, so rows are
# not 16-byte aligned and the kernel takes its scalar loads; ten tiles per item (the grid is one workgroup per tile, not
# persistent: at least three tiles per item, and more tiles (40) than the 14 split-K slices of the weight gradients)
CASES = [(1, 1), (2, 64), (3, 70), (2, 257), (4, 600)]
ALLOW = 4.0          # a float32 evaluation may sit at this many times the reference's own f32-against-f64 gap
NAMES = ["y", "w0", "b0", "w2", "b2", "gamma", "beta", "a"]      # the output, then the gradients


def case(B, N, seed=0):
    """dict: `mod` a float64 CPU `_TextAttention`, `x` (B, 384, N), `text` (B, 512), `gy` (B, 384, N) float64 CPU tensors"""
    g = torch.Generator().manual_seed(7000 + 131 * seed + 17 * B + N)
    r32 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    mod = _TextAttention().double()
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name in ("norm_q.weight", "norm_out.weight"):
                p.copy_((1.0 + 0.1 * r32(*p.shape).float()).double())
            else:
                p.copy_((0.05 * r32(*p.shape).float()).double())
    gy = r32(B, C, N) * torch.as_tensor(np.ldexp(1.0, np.arange(B) % 3 - 1)).reshape(B, 1, 1)
    return dict(B=B, N=N, mod=mod, x=r32(B, C, N), text=r32(B, TEXT), gy=gy)


def torch_stage(mod, x, text):
    """x (B, 384, N) channel-first, text (B, 512) -> (B, 384, N): `_TextAttention.rows` on the rows of x"""
    return mod.rows(x.transpose(1, 2), text[:, None, :]).transpose(1, 2)


def autograd(c, dtype, device="cpu"):
    """{name: float64 numpy} of NAMES for L = sum(y * gy) through `torch_stage` in `dtype` on `device`.  dL/da is the
    gradient that reaches the attention output, summed over the item's rows."""
    import copy
    mod = copy.deepcopy(c["mod"]).to(device=device, dtype=dtype)
    mod.zero_grad()
    got = {}
    hook = mod.attn.register_forward_hook(lambda m, i, o: (o[0].retain_grad(), got.__setitem__("attn", o[0]))[0])
    y = torch_stage(mod, c["x"].to(device=device, dtype=dtype), c["text"].to(device=device, dtype=dtype))
    hook.remove()
    y.backward(c["gy"].to(device=device, dtype=dtype))
    n = lambda t: t.detach().double().cpu().numpy()
    return dict(y=n(y), w0=n(mod.out_mlp[0].weight.grad), b0=n(mod.out_mlp[0].bias.grad),
                w2=n(mod.out_mlp[2].weight.grad), b2=n(mod.out_mlp[2].bias.grad), gamma=n(mod.norm_out.weight.grad),
                beta=n(mod.norm_out.bias.grad), a=n(got["attn"].grad.double().sum(dim=1)))


def weights(c, R=np.float64):
    """the six tensors the kernels read, as numpy arrays of type R"""
    m = c["mod"]
    n = lambda t: t.detach().numpy().astype(R)
    return dict(w0=n(m.out_mlp[0].weight), b0=n(m.out_mlp[0].bias), w2=n(m.out_mlp[2].weight), b2=n(m.out_mlp[2].bias),
                gamma=n(m.norm_out.weight), beta=n(m.norm_out.bias))


def attn_vector(c, R=np.float64):
    """a (B, 384) = out_proj(in_proj_v(v_proj(text)))"""
    m = c["mod"]
    n = lambda t: t.detach().numpy().astype(R)
    v = c["text"].numpy().astype(R) @ n(m.v_proj.weight).T + n(m.v_proj.bias)
    v = v @ n(m.attn.in_proj_weight)[2 * C:].T + n(m.attn.in_proj_bias)[2 * C:]
    return (v @ n(m.attn.out_proj.weight).T + n(m.attn.out_proj.bias)).astype(R)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def closed_form(c, dtype=np.float64, mut=None):
    """{name: float64 numpy} of NAMES by the closed form.  mut: 'tanh_gelu' (the tanh approximation in place of erf, value
    and derivative), 'ln_no_proj' (a LayerNorm backward without the Vh mean(D Vh) term)"""
    R = dtype
    B, N = c["B"], c["N"]
    w = weights(c, R)
    a = attn_vector(c, R)
    X, GY = c["x"].numpy().astype(R), c["gy"].numpy().astype(R)
    out = dict(y=np.zeros((B, C, N)), a=np.zeros((B, C)))
    ntile = -(-N // TN)
    part = {k: np.zeros((B, ntile, C), dtype=R) for k in ("gamma", "beta", "dv", "dh")}
    gw0, gw2 = np.zeros((C, C), dtype=R), np.zeros((C, C), dtype=R)
    for b in range(B):
        U = (X[b] + a[b][:, None]).astype(R)
        H = (w["w0"] @ U + w["b0"][:, None]).astype(R)
        if mut == "tanh_gelu":
            k0, k1 = R(math.sqrt(2.0 / math.pi)), R(0.044715)
            th = np.tanh(k0 * (H + k1 * H * H * H)).astype(R)
            G = (R(0.5) * H * (R(1) + th)).astype(R)
            GP = (R(0.5) * (R(1) + th) + R(0.5) * H * (R(1) - th * th) * k0 * (R(1) + R(3) * k1 * H * H)).astype(R)
        else:
            cdf = (R(0.5) * (R(1) + _erf(H * R(math.sqrt(0.5))).astype(R))).astype(R)
            G = (H * cdf).astype(R)
            GP = (cdf + H * (R(1.0 / math.sqrt(2.0 * math.pi)) * np.exp(R(-0.5) * H * H).astype(R))).astype(R)
        V = ((w["w2"] @ G + w["b2"][:, None]).astype(R) + U).astype(R)       # the residual after the product, as the kernel
        mu = (V.sum(axis=0, dtype=R) * R(1.0 / C)).astype(R)
        Dc = (V - mu).astype(R)
        r = (R(1) / np.sqrt((Dc * Dc).sum(axis=0, dtype=R) * R(1.0 / C) + R(1e-5))).astype(R)
        Vh = (Dc * r).astype(R)
        out["y"][b] = w["gamma"][:, None] * Vh + w["beta"][:, None]
        D = (w["gamma"][:, None] * GY[b]).astype(R)
        m1 = (D.sum(axis=0, dtype=R) * R(1.0 / C)).astype(R)
        m2 = ((D * Vh).sum(axis=0, dtype=R) * R(1.0 / C)).astype(R)
        dV = (r * (D - m1 - (Vh * m2 if mut != "ln_no_proj" else R(0)))).astype(R)
        dH = ((w["w2"].T @ dV) * GP).astype(R)
        gw2 += (dV @ G.T).astype(R)
        gw0 += (dH @ U.T).astype(R)
        for t in range(ntile):
            s = slice(t * TN, min(N, (t + 1) * TN))
            part["gamma"][b, t] = (GY[b][:, s] * Vh[:, s]).sum(axis=1, dtype=R)
            part["beta"][b, t] = GY[b][:, s].sum(axis=1, dtype=R)
            part["dv"][b, t] = dV[:, s].sum(axis=1, dtype=R)
            part["dh"][b, t] = dH[:, s].sum(axis=1, dtype=R)
    item = {k: np.zeros((B, C), dtype=R) for k in part}
    for k in part:                                   # tiles in order per item, then the items in order
        for t in range(ntile):
            item[k] = (item[k] + part[k][:, t]).astype(R)
    tot = {k: np.zeros(C, dtype=R) for k in part}
    for k in part:
        for b in range(B):
            tot[k] = (tot[k] + item[k][b]).astype(R)
    out["a"] = ((item["dh"] @ w["w0"]).astype(R) + item["dv"]).astype(np.float64)
    out.update(w0=gw0, b0=tot["dh"], w2=gw2, b2=tot["dv"], gamma=tot["gamma"], beta=tot["beta"])
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def gap(got, want):
    """max |got - want| / max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def gaps(got, want):
    return {k: gap(got[k], want[k]) for k in NAMES}


@functools.lru_cache(maxsize=None)
def refs(shape):
    """(case, float64 autograd, torch-CPU's own f32-against-f64 gap per tensor) of a (B, N) shape, computed once and shared
    by the tests.  Treat the arrays as read-only."""
    c = case(*shape)
    g64 = autograd(c, torch.float64)
    return c, g64, gaps(autograd(c, torch.float32), g64)
