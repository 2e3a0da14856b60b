"""Time of head training's update step alone: gradient clipping plus AdamW over the head's 50 tensors (2 983 804 float32
parameters), three paths alternating in one process under device events:

    torch          `clip_grad_norm_` + the default `torch.optim.AdamW` (foreach; what the reference runs)
    torch_fused    the same with `torch.optim.AdamW(fused=True)`
    native         `athd.optim.HeadAdamW.step(grad_clip=1.0)`: one `athd_head_step` call (csrc/head_step.hip)

    python tools/head_step_time.py [--iters 50] [--reps 10] [--warmup 5] [--out FILE.json]

A timed window is `--reps` consecutive steps of one path between two events (the host enqueues them back to back, as a
training loop does, so a path that is bound by its launches shows it); the figure is the window over `--reps`.  The
seeded gradients are copied back before every window, outside it (torch's clip rewrites them).  It prints the median
and the spread of each path in ms, the ratios, the native kernels' times from one profiled window, the bytes the native
step moves with the time they take at the HBM rate, and checks that three steps of the three paths from one start agree
(the displacement gap of tests/head_step_refs.py to torch's float64 step, native within 4 x torch's own float32 gap).  Needs the GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-to-sheet-music_amd"))

HBM_BYTES_PER_S = 8.0e12          # MI355X peak HBM3E rate
LR, WD, CLIP = 1e-3, 1e-2, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_step_time: no GPU (times are taken on the device only)")
    from athd.head import head_keys
    from athd.optim import HeadAdamW
    from athd.weights import synthetic_state_dict

    sd = synthetic_state_dict(seed=0)
    start = [torch.as_tensor(sd[k]).cuda() for k, _ in head_keys()]
    gen = torch.Generator().manual_seed(0)
    grads = [[(0.01 * torch.randn(p.shape, generator=gen)).cuda() for p in start] for _ in range(3)]
    n = sum(p.numel() for p in start)

    def make(name):
        params = [torch.nn.Parameter(p.clone()) for p in start]
        if name == "native":
            opt = HeadAdamW(params, lr=LR, weight_decay=WD)
            step = lambda: opt.step(grad_clip=CLIP)
        else:
            opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD, **({"fused": True} if name == "torch_fused" else {}))

            def step():
                torch.nn.utils.clip_grad_norm_(params, CLIP)
                opt.step()
        return params, step

    def set_grads(params, k):
        for p, g in zip(params, grads[k]):
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)

    names = ["torch", "torch_fused", "native"]
    # the three agree: three steps from one start with fresh gradients each, every path against torch's float64 step
    # (`clip_grad_norm_` + `AdamW(foreach=False)` on float64 copies), by the displacement gap of tests/head_step_refs.py
    p64 = [torch.nn.Parameter(p.double()) for p in start]
    o64 = torch.optim.AdamW(p64, lr=LR, weight_decay=WD, foreach=False)
    for k in range(3):
        for p, g in zip(p64, grads[k]):
            p.grad = g.double()
        torch.nn.utils.clip_grad_norm_(p64, CLIP, foreach=False)
        o64.step()
    want = [p.detach() - s.double() for p, s in zip(p64, start)]
    agree = {}
    for name in names:
        params, step = make(name)
        for k in range(3):
            set_grads(params, k)
            step()
        got = [p.detach().double() - s.double() for p, s in zip(params, start)]
        agree[name] = max(float((u - w).abs().max() / w.abs().max()) for u, w in zip(got, want))
    print("displacement gap to the float64 step after 3 steps:", json.dumps(agree))
    # timing paths that disagree is moot: the tests' allowance, ALLOW = 4 times the gap of torch's own float32 step
    assert agree["torch"] > 0 and agree["native"] <= 4.0 * agree["torch"], agree

    paths = {name: make(name) for name in names}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in names}
    for it in range(a.warmup + a.iters):
        for name in names:
            params, step = paths[name]
            set_grads(params, 0)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.reps):
                step()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1) / a.reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    # where the native time goes: one profiled window, on its own
    kernels = "not measured"
    try:
        from torch.profiler import ProfilerActivity, profile
        params, step = paths["native"]
        set_grads(params, 0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(a.reps):
                step()
            torch.cuda.synchronize()
        kernels = {}
        for ev in prof.key_averages():
            if "head_step" in ev.key:
                total_us = getattr(ev, "device_time_total", None)
                if total_us is None:
                    total_us = ev.cuda_time_total
                kernels[ev.key.split("(")[0].split("::")[-1]] = round(total_us / ev.count / 1000.0, 5)
        kernels = kernels or "not measured"
    except Exception as e:          # the profiler is optional; the step times above do not depend on it
        kernels = "not measured (%s)" % type(e).__name__
    moved = n * (4 + 16 + 12)         # the norm launch reads g; the update reads p, g, m, v and writes p, m, v
    result = {"tensors": len(start), "parameters": n, "iters": a.iters, "reps_per_window": a.reps,
              "ms_per_step": {k: med[k] for k in names},
              "ms_per_step_min_max": {k: [min(times[k]), max(times[k])] for k in names},
              "torch_over_native": med["torch"] / med["native"],
              "torch_fused_over_native": med["torch_fused"] / med["native"],
              "native_kernels_ms": kernels,
              "native_bytes_per_step": moved, "native_ms_at_hbm_rate": moved / HBM_BYTES_PER_S * 1e3,
              "displacement_gap_to_float64_after_3_steps": agree}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
