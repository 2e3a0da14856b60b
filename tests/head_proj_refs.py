"""References for head training's output projections and attention vector (csrc/head_proj.hip, include/athd.h
`athd_head_proj*`, `athd_head_attn_vec*`); a helper module of tests/test_head_proj_refs.py and tests/test_gpu_head_proj.py,
not a test file.

  * `proj_case` / `attn_case`: seeded float32-representable inputs (weights about 0.3 randn for the 4 -> 2 projection and
    0.05 randn for the attention's matrices, a per-item `scale` drawn between 0.5 and 2, so no power of two);
  * `proj_autograd` / `attn_autograd`: torch itself, `nn.Conv2d(4, 2, 1)` (R > 1) or `nn.Conv1d(4, 2, 1)` (R == 1) and
    `_TextAttention.attn_vector`, differentiated through L = sum(y gy) (item b's term times scale[b]), in any dtype and
    on any device;
  * `proj_closed_form` / `attn_closed_form`: the two primitives as include/athd.h states them, in numpy.  The float32
    variants follow the kernels' sequence of operations: fused multiply-adds become a product and a sum in float32,
    `scale` multiplies the gradient first, every sum over positions or items is kept in double and rounded once.  `mut`
    plants the defects the tests' bound must separate;
  * `proj_floor` / `attn_floor`: the rounding floor of the allowance per tensor, see below;
  * `gap`, `ratios` from head_dec_refs: the worst |got - want| over the tensor's largest |want|, over the unit.

The allowance.  A tensor may sit at ALLOW = 4 units from the float64 reference; its unit is max(a, floor), `a` torch's own
float32-against-float64 gap on the same case.  Without `floor` a tensor that torch happens to hit exactly (one product, a
bias sum) would demand exact equality of an evaluation that rounds elsewhere.  `floor` is k u with u = 2^-24 (half an ulp
of the tensor's largest value, the scale of `gap`) and k the float32 roundings a straightforward evaluation of one
element goes through:

  y       four products and four additions: 8
  grad_x  two products and one addition, one more product when `scale` is given: 3 + s
  grad_w, grad_b   the scale product and the rounding of the result: 1 + s.  The sum over the positions is not counted: a
          float32 chain's error grows with the number of terms, which is what `a` measures on torch's own sum; the floor
          is what remains when the sum is exact
  a       three chained layers, each at least one rounding: 3
  the attention's gradients: wo, w_in (value third), wv and bv 3 (two rounded factors and the result), b_in 2, bo 1.
The dead thirds of w_in / b_in must be exact zeros: their unit is 0.
"""
import functools

import numpy as np
import torch
import torch.nn as nn

from athd.head import _TextAttention
from head_dec_refs import gap, ratios  # noqa: F401 (re-exported)

ALLOW = 4.0
U = 2.0 ** -24
CHUNK = 4096                                # the stream kernels' positions per workgroup
# (B, R, S, grad_channel_first, scale): one position; the grids of T = 4096 and T = 5000; R != S, both across a 32-wide
# tile; S no multiple of the vector width; one more than three chunks, so that the tail adds partials of several
# workgroups per item; 70001 with both gradient layouts and a scale; 65 items of five chunks, 325 workgroups: the tail
# stages 256 workgroups' partials at a time, so it takes a second batch and carries its sums across
PROJ_CASES = [
    (1, 1, 1, 0, False),
    (2, 4, 4, 0, False),
    (2, 5, 5, 0, True),
    (3, 33, 37, 0, False),
    (3, 33, 37, 1, True),
    (2, 1, 4099, 0, False),
    (2, 1, 3 * CHUNK + 1, 0, True),
    (2, 1, 70001, 0, True),
    (2, 1, 70001, 1, True),
    (65, 1, 4 * CHUNK + 1, 0, True),
]
PROJ_NAMES = ["y", "x", "w", "b"]           # the output, then the gradients
PROJ_MUTS = ["rs_swapped", "w_transposed", "no_bias", "scale_ignored", "scale_w_only"]
ATTN_CASES = [1, 2, 7, 130]                 # B
ATTN_NAMES = ["a", "wv", "bv", "w_in", "b_in", "wo", "bo", "w_in_dead", "b_in_dead"]
ATTN_MUTS = ["k_third", "dead_nonzero"]
D, TEXT = 384, 512


def proj_blind(shape, mut):
    """True where the case cannot see the defect at all"""
    B, R, S, cf, scale = shape
    if mut == "rs_swapped":
        return R == 1 or S == 1
    if mut in ("scale_ignored", "scale_w_only"):
        return not scale
    return False


def proj_sees(mut):
    """the tensors a defect shows in"""
    return {"rs_swapped": ["y"], "w_transposed": PROJ_NAMES[:3], "no_bias": ["y"], "scale_ignored": ["x", "w", "b"],
            "scale_w_only": ["x"]}[mut]


def proj_case(B, R, S, cf, scale, seed=0):
    """dict of float64 CPU tensors: x (B, 4, R, S), w (2, 4), b (2), gy in y's layout (B, S, R, 2) or, cf, (B, 2, R, S),
    scale (B) or None"""
    g = torch.Generator().manual_seed(11000 + 131 * seed + 17 * B + 7 * R + 3 * S + cf)
    r32 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    f32 = lambda t: t.float().double()
    gy = r32(B, 2, R, S) if cf else r32(B, S, R, 2)
    sc = f32(0.5 + 1.5 * torch.rand(B, generator=g, dtype=torch.float32).double()) if scale else None
    return dict(B=B, R=R, S=S, cf=cf, x=r32(B, 4, R, S), w=f32(0.3 * r32(2, 4)), b=f32(0.3 * r32(2)), gy=gy, scale=sc)


def _gy_cf(c, gy):
    """the incoming gradient as (B, 2, R, S), whatever its layout"""
    return gy if c["cf"] else gy.permute(0, 3, 2, 1)


def proj_autograd(c, dtype, device="cpu"):
    """{name: float64 numpy} of PROJ_NAMES through torch's own 1x1 convolution in `dtype` on `device`"""
    to = lambda t: t.to(device=device, dtype=dtype)
    B, R, S = c["B"], c["R"], c["S"]
    conv = (nn.Conv1d(4, 2, 1) if R == 1 else nn.Conv2d(4, 2, 1)).to(device=device, dtype=dtype)
    with torch.no_grad():
        conv.weight.copy_(to(c["w"]).reshape(conv.weight.shape))
        conv.bias.copy_(to(c["b"]))
    x = to(c["x"]).detach().clone().requires_grad_(True)
    out = conv(x.reshape(B, 4, S)).reshape(B, 2, R, S) if R == 1 else conv(x)       # (B, 2, R, S)
    g = _gy_cf(c, to(c["gy"]))
    if c["scale"] is not None:
        g = g * to(c["scale"]).reshape(B, 1, 1, 1)
    out.backward(g.contiguous())
    n = lambda t: t.detach().double().cpu().numpy()
    return dict(y=n(out.permute(0, 3, 2, 1)), x=n(x.grad), w=n(conv.weight.grad).reshape(2, 4), b=n(conv.bias.grad))


def proj_closed_form(c, dtype=np.float64, mut=None):
    """{name: float64 numpy} of PROJ_NAMES by the closed form of include/athd.h.  mut: one of PROJ_MUTS"""
    Rt = dtype
    n_ = lambda t: t.numpy().astype(Rt)
    B, R, S = c["B"], c["R"], c["S"]
    X, W, bias = n_(c["x"]), n_(c["w"]), n_(c["b"])
    if mut == "w_transposed":
        W = W.reshape(4, 2).T.copy()                                   # the same memory read as [in][out]
    GY = n_(_gy_cf(c, c["gy"]).contiguous())
    acc = (np.zeros(2, dtype=Rt) if mut == "no_bias" else bias)[None, :, None, None] * np.ones((B, 2, R, S), dtype=Rt)
    for ch in range(4):
        acc = (acc + (W[:, ch][None, :, None, None] * X[:, ch][:, None]).astype(Rt)).astype(Rt)
    y = acc.transpose(0, 3, 2, 1)                                      # (B, S, R, 2)
    if mut == "rs_swapped":
        y = np.ascontiguousarray(acc.transpose(0, 2, 3, 1)).reshape(B, S, R, 2)        # written as [r][s], read as [s][r]
    sc = n_(c["scale"])[:, None, None, None] if c["scale"] is not None else None
    G = GY if sc is None or mut == "scale_ignored" else (GY * sc).astype(Rt)
    Gx = GY if mut == "scale_w_only" else G
    gx = ((W[0][None, :, None, None] * Gx[:, 0][:, None]).astype(Rt) +
          (W[1][None, :, None, None] * Gx[:, 1][:, None]).astype(Rt)).astype(Rt)
    # the sums: products and additions in double, rounded once
    gw = np.einsum("bors,bcrs->oc", G.astype(np.float64), X.astype(np.float64)).astype(Rt)
    gb = G.astype(np.float64).sum(axis=(0, 2, 3)).astype(Rt)
    return {k: np.asarray(v, np.float64) for k, v in dict(y=y, x=gx, w=gw, b=gb).items()}


def proj_floor(c):
    """{name: k u}, k the roundings of the module docstring"""
    s = 1 if c["scale"] is not None else 0
    return dict(y=8 * U, x=(3 + s) * U, w=(1 + s) * U, b=(1 + s) * U)


def units(a, floor):
    return {k: max(a[k], floor[k]) for k in a}


@functools.lru_cache(maxsize=None)
def proj_refs(shape):
    """(case, float64 autograd, torch-CPU's own f32-against-f64 gap per tensor, floor) of a PROJ_CASES entry, computed
    once and shared by the tests.  Treat the arrays as read-only."""
    c = proj_case(*shape)
    g64 = proj_autograd(c, torch.float64)
    g32 = proj_autograd(c, torch.float32)
    return c, g64, {k: gap(g32[k], g64[k]) for k in PROJ_NAMES}, proj_floor(c)


# ------------------------------------------------------------------------------------------ the attention vector
def attn_case(B, seed=0):
    """dict: `mod` a float64 CPU `_TextAttention` (weights about 0.05 randn), text (B, 512) and ga (B, 384) float64"""
    g = torch.Generator().manual_seed(12000 + 131 * seed + 17 * B)
    r32 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    mod = _TextAttention().double()
    with torch.no_grad():
        for name, p in mod.named_parameters():
            p.copy_((0.05 * r32(*p.shape).float()).double())
    return dict(B=B, mod=mod, text=r32(B, TEXT), ga=r32(B, D))


def _split(out):
    """w_in / b_in into their live value third and the dead query and key thirds"""
    out["w_in_dead"], out["w_in"] = out["w_in"][:2 * D], out["w_in"][2 * D:]
    out["b_in_dead"], out["b_in"] = out["b_in"][:2 * D], out["b_in"][2 * D:]
    return out


def attn_autograd(c, dtype, device="cpu"):
    """{name: float64 numpy} of ATTN_NAMES for L = sum(a ga) through `_TextAttention.attn_vector`"""
    import copy
    mod = copy.deepcopy(c["mod"]).to(device=device, dtype=dtype)
    mod.zero_grad()
    a = mod.attn_vector(c["text"].to(device=device, dtype=dtype))
    a.backward(c["ga"].to(device=device, dtype=dtype))
    n = lambda t: t.detach().double().cpu().numpy()
    return _split(dict(a=n(a), wv=n(mod.v_proj.weight.grad), bv=n(mod.v_proj.bias.grad),
                       w_in=n(mod.attn.in_proj_weight.grad), b_in=n(mod.attn.in_proj_bias.grad),
                       wo=n(mod.attn.out_proj.weight.grad), bo=n(mod.attn.out_proj.bias.grad)))


def attn_weights(c, Rt=np.float64):
    m = c["mod"]
    n = lambda t: t.detach().numpy().astype(Rt)
    return dict(wv=n(m.v_proj.weight), bv=n(m.v_proj.bias), w_in=n(m.attn.in_proj_weight), b_in=n(m.attn.in_proj_bias),
                wo=n(m.attn.out_proj.weight), bo=n(m.attn.out_proj.bias))


def attn_closed_form(c, dtype=np.float64, mut=None):
    """{name: float64 numpy} of ATTN_NAMES by the closed form.  Every product sum in double, rounded once to `dtype`.
    mut: one of ATTN_MUTS"""
    Rt = dtype
    w = attn_weights(c, Rt)
    d = lambda t: t.astype(np.float64)
    rnd = lambda t: t.astype(Rt)
    text, ga = c["text"].numpy().astype(Rt), c["ga"].numpy().astype(Rt)
    third = slice(D, 2 * D) if mut == "k_third" else slice(2 * D, 3 * D)
    wi, bi = w["w_in"][third], w["b_in"][third]
    v1 = rnd(d(text) @ d(w["wv"]).T + d(w["bv"]))
    v2 = rnd(d(v1) @ d(wi).T + d(bi))
    a = rnd(d(v2) @ d(w["wo"]).T + d(w["bo"]))
    gwo, gbo = rnd(d(ga).T @ d(v2)), rnd(d(ga).sum(axis=0))
    gv2 = rnd(d(ga) @ d(w["wo"]))
    gwi, gbi = rnd(d(gv2).T @ d(v1)), rnd(d(gv2).sum(axis=0))
    gv1 = rnd(d(gv2) @ d(wi))
    gwv, gbv = rnd(d(gv1).T @ d(text)), rnd(d(gv1).sum(axis=0))
    w_in, b_in = np.zeros((3 * D, D), dtype=Rt), np.zeros(3 * D, dtype=Rt)
    w_in[third], b_in[third] = gwi, gbi
    if mut == "dead_nonzero":                                           # rounding noise where exact zeros belong
        w_in[0, 0] = Rt(1e-30)
        b_in[D] = Rt(1e-30)
    out = _split(dict(a=a, wv=gwv, bv=gbv, w_in=w_in, b_in=b_in, wo=gwo, bo=gbo))
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def attn_floor(c):
    """{name: k u}, k the roundings of the module docstring; 0 for the dead thirds"""
    k = dict(a=3, wv=3, bv=3, w_in=3, b_in=2, wo=3, bo=1, w_in_dead=0, b_in_dead=0)
    return {n: v * U for n, v in k.items()}


def attn_gaps(got, want):
    """`gap` per tensor; a dead third (want all zero) has gap max |got|"""
    out = {}
    for k in ATTN_NAMES:
        out[k] = float(np.abs(got[k]).max()) if k.endswith("_dead") else gap(got[k], want[k])
    return out


@functools.lru_cache(maxsize=None)
def attn_refs(B):
    """(case, float64 autograd, torch-CPU's f32-against-f64 gap per tensor, floor) of an ATTN_CASES entry, shared"""
    c = attn_case(B)
    g64 = attn_autograd(c, torch.float64)
    return c, g64, attn_gaps(attn_autograd(c, torch.float32), g64), attn_floor(c)
