"""Time of what `native_proj` replaces in head training, forward plus backward, two paths alternating in one process under
device events, at B = 8 and 6 s (T = 264600, a 259 x 259 logit grid):

  stage    torch     `freq_out` / `time_out` as torch convolutions, the permutes and `.contiguous()` into the output
                     stage's layouts, `g * stdt`, and `NativeOutputStage` (what `native_output` alone runs today)
           native    `NativeProjOutput`: `athd_head_proj` twice + `athd_head_output`, `athd_head_output_backward` +
                     `athd_head_proj_backward` twice (csrc/head_proj.hip)
  attn     torch     `_TextAttention.attn_vector`: three `F.linear` on (B, 512), two weight slices, their backward
           native    `NativeAttnVector`: `athd_head_attn_vec` / `athd_head_attn_vec_backward`

    python tools/head_proj_time.py [--iters 30] [--reps 5] [--warmup 5] [--out FILE.json]

A timed window is `--reps` consecutive forward + backward passes of one path between two events; the figure is the window
over `--reps`.  It prints the median and the range of each path in ms, the peak memory of one pass above the inputs, the
native projection kernels' times from one profiled window with the bytes they move and the time those take at the HBM
rate, and checks first that the two paths agree.  Needs the GPU; there is no CPU fallback.
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
B, T = 8, 264600


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_proj_time: no GPU (times are taken on the device only)")
    from athd.head import NativeAttnVector, NativeOutputStage, NativeProjOutput, TrainableHead
    from athd.model import AudioTextHTDemucs
    from athd.weights import STEMS, synthetic_state_dict, synthetic_text_table

    table = synthetic_text_table(4, seed=7)
    model = AudioTextHTDemucs(dtype="f32", text_table={s: table[i] for i, s in enumerate(STEMS)})
    model.load_state_dict(synthetic_state_dict(seed=0))
    model.to("cuda").eval()
    nctx = model._ensure_ctx()
    head = TrainableHead.from_model(model).cuda()
    Ts = -(-T // 1024)
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    xd, xtd = rnd(B, 4, Ts, Ts).requires_grad_(True), rnd(B, 4, T).requires_grad_(True)
    spec, g = rnd(B, Ts, 2048, 4), rnd(B, 2, T)
    meant, stdt = 0.01 * rnd(B, 1, 1), 0.5 + torch.rand(B, 1, 1, generator=gen).cuda()
    text, ga = rnd(B, 512), rnd(B, 384)
    ta = head.text_attn
    proj_params = [head.freq_out.weight, head.freq_out.bias, head.time_out.weight, head.time_out.bias]
    attn_params = [ta.v_proj.weight, ta.v_proj.bias, ta.attn.in_proj_weight, ta.attn.in_proj_bias, ta.attn.out_proj.weight,
                   ta.attn.out_proj.bias]

    def stage_torch():
        y = NativeOutputStage.apply(head.freq_out(xd), head.time_out(xtd), spec, meant, stdt, nctx)
        return torch.autograd.grad(y, [xd, xtd] + proj_params, g)

    def stage_native():
        y = NativeProjOutput.apply(xd, xtd, *proj_params, spec, meant, stdt, nctx)
        return torch.autograd.grad(y, [xd, xtd] + proj_params, g)

    def attn_torch():
        return torch.autograd.grad(ta.attn_vector(text), attn_params, ga)

    def attn_native():
        return torch.autograd.grad(NativeAttnVector.apply(text, *attn_params, nctx), attn_params, ga)

    paths = {"stage": {"torch": stage_torch, "native": stage_native}, "attn": {"torch": attn_torch, "native": attn_native}}
    # the two paths agree: the worst gradient gap over the tensor's largest value (float32 against float32)
    agree = {}
    for what, p in paths.items():
        gt, gn = p["torch"](), p["native"]()
        agree[what] = max(float((u - w).abs().max() / w.abs().max()) for u, w in zip(gn, gt))
    print("native against torch, worst gradient gap:", json.dumps(agree))
    assert max(agree.values()) <= 1e-4, agree

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {w: {k: [] for k in p} for w, p in paths.items()}
    for it in range(a.warmup + a.iters):
        for what, p in paths.items():
            for name, fn in p.items():
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[what][name].append(e0.elapsed_time(e1) / a.reps)
    peak = {}
    for what, p in paths.items():
        peak[what] = {}
        for name, fn in p.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak[what][name] = torch.cuda.max_memory_allocated() - base
            del out
    # where the native stage's time goes: one profiled window, on its own
    kernels = "not measured"
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(a.reps):
                stage_native()
            torch.cuda.synchronize()
        kernels = {}
        for ev in prof.key_averages():
            if "head_proj" in ev.key:
                total_us = getattr(ev, "device_time_total", None)
                if total_us is None:
                    total_us = ev.cuda_time_total
                # (per pass: the forward kernel runs twice in it, the tail twice, each backward kernel once)
                kernels[ev.key.split("(")[0].split("::")[-1]] = round(total_us / a.reps / 1000.0, 5)
        kernels = kernels or "not measured"
    except Exception as e:          # the profiler is optional; the times above do not depend on it
        kernels = "not measured (%s)" % type(e).__name__
    n_t, n_f = B * T, B * Ts * Ts
    moved = (n_t + n_f) * 4 * (6 + 10)          # forward: 4 read + 2 written per position; backward: 2 + 4 read, 4 written
    med = {w: {k: statistics.median(v) for k, v in t.items()} for w, t in times.items()}
    result = {"B": B, "T": T, "grid": [Ts, Ts], "iters": a.iters, "reps_per_window": a.reps,
              "ms_per_pass": med,
              "ms_per_pass_min_max": {w: {k: [min(v), max(v)] for k, v in t.items()} for w, t in times.items()},
              "torch_over_native": {w: med[w]["torch"] / med[w]["native"] for w in med},
              "peak_bytes_above_inputs": peak,
              "native_proj_kernels_ms_per_pass": kernels,
              "native_proj_bytes_per_pass": moved, "native_proj_ms_at_hbm_rate": moved / HBM_BYTES_PER_S * 1e3,
              "worst_gradient_gap_native_against_torch": agree}
    if isinstance(kernels, dict):
        result["native_proj_hbm_fraction"] = result["native_proj_ms_at_hbm_rate"] / sum(kernels.values())
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
