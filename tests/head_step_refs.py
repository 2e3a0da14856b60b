"""References for head training's update step (`athd_head_step`, athd/optim.py `HeadAdamW`): clip + AdamW.

  * `ref64(case, K)`         the step as include/athd.h states it, in float64 numpy: global norm, clip_grad_norm_'s clamped
                             coefficient, decoupled decay, the moments, the bias-corrected update.  `store=np.float32`
                             keeps parameters and moments in float32 (arithmetic in float64, one rounding per stored
                             value: what the kernel does); `arith=np.float32` does the arithmetic in float32 too.
                             `mut=` plants one defect (MUTATIONS).
  * `torch_step(case, K, dtype, device)`   `clip_grad_norm_` + `torch.optim.AdamW(foreach=False)`, torch's own kernels
  * `gaps(got, want)`        the project's gap (worst |got - want| over the tensor's largest |want|, pooled by maximum
                             over the tensors) for the displacement p_K - p_0, for m and for v

A test allows a float32 implementation ALLOW times the gaps of torch's own float32 step to `ref64`
(tests/test_head_step_refs.py shows that float32 evaluations reach that and that every planted defect misses it by
orders of magnitude in the regime named for it in MUTATIONS).

Not claimed by any test: the `+ 1e-6` in the clip coefficient's denominator.  Dropping it moves the result by 1e-9
relative where the clip is active; float32 storage cannot see that.
"""
import functools

import numpy as np
import torch

ALLOW = 4.0
SIZES = [1, 3, 4, 5, 255, 4095, 4096, 4097, 8195, 1, 384, 12289]     # one element, non-multiples of 4, both sides of a
#                                     chunk edge (4096), two chunks plus a tail, three chunks plus one element, a repeat
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, max_norm=1.0)
KMAX = 4                    # gradient sets per case: the tests take K = 1 and 3 steps, one test a fourth
# gradient scale -> what it exercises
REGIMES = {"inactive": 1e-3,       # total norm about 0.4: the clip coefficient is 1
           "active": 1.0,          # the clip is active: the only regime that exposes a per-tensor norm
           "eps": 1e-7}            # gradients comparable to eps: exposes where eps sits
# planted defect -> the regime in which a test must see it
MUTATIONS = {"per_tensor_norm": "active",      # each tensor clipped by its own norm
             "l2_decay": "inactive",           # coupled decay: g += wd p, no p *= 1 - lr wd
             "no_bc1": "inactive",             # step size lr, not lr / (1 - beta1^t)
             "no_bc2": "inactive",             # sqrt(v) not divided by sqrt(1 - beta2^t)
             "eps_in_sqrt": "eps",             # sqrt(v / bc2 + eps)
             "eps_unscaled": "eps"}            # (sqrt(v) + eps) / sqrt(bc2): eps divided by sqrt(bc2)


@functools.lru_cache(maxsize=None)
def case(regime, sizes=tuple(SIZES), seed=0):
    """{"p0": [float32 arrays], "grads": [KMAX lists of float32 arrays]}: parameters 0.05 randn, gradient i of a step
    scale randn 2^(i % 5 - 2)"""
    scale = REGIMES[regime]
    rng = np.random.default_rng(seed)
    p0 = [(0.05 * rng.standard_normal(n)).astype(np.float32) for n in sizes]
    grads = [[(scale * rng.standard_normal(n) * 2.0 ** (i % 5 - 2)).astype(np.float32) for i, n in enumerate(sizes)]
             for _ in range(KMAX)]
    return {"p0": p0, "grads": grads}


def ref64(c, K, hp=None, mut=None, store=np.float64, arith=np.float64, grad_scale=None):
    """K steps -> {"p", "m", "v": lists of float64 arrays, "norm", "coef": per step}"""
    hp = dict(HP, **(hp or {}))
    A = arith
    # the step's scalars are formed from the Python doubles and then cast, as torch does: 1 - float32(0.999) would carry
    # a relative 1.3e-5 into every v
    lr, b1, b2, wd = hp["lr"], hp["beta1"], hp["beta2"], hp["weight_decay"]
    eps, max_norm, one = A(hp["eps"]), A(hp["max_norm"]), A(1.0)
    p = [x.astype(store) for x in c["p0"]]
    m = [np.zeros(x.shape, store) for x in c["p0"]]
    v = [np.zeros(x.shape, store) for x in c["p0"]]
    norms, coefs = [], []
    inv = one if grad_scale is None else A(1.0 / grad_scale)
    for t in range(1, K + 1):
        g = [x.astype(A) for x in c["grads"][t - 1]]
        per = [np.sqrt(np.sum(x * x, dtype=A)) * inv for x in g]
        norm = np.sqrt(A(sum(np.sum(x * x, dtype=A) for x in g))) * inv
        clip = lambda nv: min(one, max_norm / (nv + A(1e-6))) if max_norm > 0 else one
        coef = clip(norm)
        norms.append(float(norm))
        coefs.append(float(coef))
        bc1 = 1.0 - b1 ** t if mut != "no_bc1" else 1.0
        bc2 = A(1.0 - b2 ** t if mut != "no_bc2" else 1.0)
        for i in range(len(p)):
            gi = g[i] * inv * (clip(per[i]) if mut == "per_tensor_norm" else coef)
            pi, mi, vi = p[i].astype(A), m[i].astype(A), v[i].astype(A)
            if mut == "l2_decay":
                gi = gi + A(wd) * pi
            else:
                pi = pi * A(1.0 - lr * wd)
            mi = A(b1) * mi + A(1.0 - b1) * gi
            vi = A(b2) * vi + A(1.0 - b2) * gi * gi
            if mut == "eps_in_sqrt":
                denom = np.sqrt(vi / bc2 + eps)
            elif mut == "eps_unscaled":
                denom = (np.sqrt(vi) + eps) / np.sqrt(bc2)
            else:
                denom = np.sqrt(vi) / np.sqrt(bc2) + eps
            pi = pi - A(lr / bc1) * mi / denom
            p[i], m[i], v[i] = pi.astype(store), mi.astype(store), vi.astype(store)
    f = lambda xs: [x.astype(np.float64) for x in xs]
    return {"p": f(p), "m": f(m), "v": f(v), "norm": norms, "coef": coefs}


def torch_step(c, K, dtype=torch.float32, device="cpu", hp=None):
    """torch's own step: `clip_grad_norm_` then `torch.optim.AdamW(foreach=False).step()`, K times"""
    hp = dict(HP, **(hp or {}))
    params = [torch.nn.Parameter(torch.tensor(x).to(device=device, dtype=dtype)) for x in c["p0"]]      # (copies)
    opt = torch.optim.AdamW(params, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"],
                            weight_decay=hp["weight_decay"], foreach=False)
    for t in range(K):
        for q, g in zip(params, c["grads"][t]):
            q.grad = torch.tensor(g).to(device=device, dtype=dtype)       # a copy: the clip rewrites it
        if hp["max_norm"] > 0:
            torch.nn.utils.clip_grad_norm_(params, hp["max_norm"], foreach=False)
        opt.step()
    f = lambda xs: [x.detach().double().cpu().numpy() for x in xs]
    return {"p": f(params), "m": f([opt.state[q]["exp_avg"] for q in params]),
            "v": f([opt.state[q]["exp_avg_sq"] for q in params])}, opt, params


def gap(got, want):
    """worst |got - want| over the tensor's largest |want|, the maximum over the tensors"""
    return max(float(np.abs(g - w).max()) / float(np.abs(w).max()) for g, w in zip(got, want))


def gaps(got, want, p0):
    """{"disp", "m", "v"}: the gap of the displacement p_K - p_0 and of the two moments"""
    p0 = [x.astype(np.float64) for x in p0]
    disp = lambda r: [x - y for x, y in zip(r["p"], p0)]
    return {"disp": gap(disp(got), disp(want)), "m": gap(got["m"], want["m"]), "v": gap(got["v"], want["v"])}
