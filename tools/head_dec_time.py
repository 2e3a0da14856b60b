"""Time and memory of head training's two decoders alone, forward plus backward: the torch ops of `_Decoder.forward`
against `_Decoder.forward_native` (`NativeDecoderLevel`, athd/head.py) on identical inputs, with device events, the two
alternating in one process; per branch (frequency, time) and for both together.

    python tools/head_dec_time.py [--batch 8] [--samples 264600] [--iters 10] [--warmup 2] [--out FILE.json]

The inputs have the shapes `athd_encode` exports for the segment (the conditioned features (B, 384, 8, Ts) and
(B, 384, L4), the skips with the decoders' channel counts) with seeded values; the head is float32.  It prints, per
branch, the median time of each path in ms, their ratio, the peak of `torch.cuda.max_memory_allocated` over one forward
plus backward of each path above what was allocated before it (inputs, parameters), the native path's per-kernel
times, and checks that the two paths agree (output SDR, gradient gap over the largest |gradient|).  The native kernels
are the same f32 code under an f32 and a bf16 context and the torch path does not see the context, so one context (f32)
is measured.  Needs the GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-to-sheet-music_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=264600)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_dec_time: no GPU (times are taken on the device only)")
    from athd.head import TrainableHead
    from athd.model import FREQ_ROWS, SKIP_CH, AudioTextHTDemucs, time_lengths
    from athd.weights import STEMS, synthetic_state_dict, synthetic_text_table

    B, T = a.batch, a.samples
    Ts, L = -(-T // 1024), time_lengths(T)
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    sd, table = synthetic_state_dict(seed=0), synthetic_text_table(4, seed=7)
    model = AudioTextHTDemucs(dtype="f32", text_table={s: table[i] for i, s in enumerate(STEMS)})
    model.load_state_dict(sd)
    model.to("cuda:0").eval()
    head = TrainableHead.from_model(model).cuda().bind(model)
    nctx = model._ensure_ctx()
    # (decoder, input, skips and targets from the deepest level outwards, incoming gradient)
    branches = {
        "freq": (head.freq_decoder, rnd(B, 384, 8, Ts), [rnd(B, SKIP_CH[i], FREQ_ROWS[i], Ts) for i in (3, 2, 1, 0)],
                 [Ts] * 4, rnd(B, 4, Ts, Ts)),
        "time": (head.time_decoder, rnd(B, 384, L[4]), [rnd(B, SKIP_CH[i], L[i + 1]) for i in (3, 2, 1, 0)],
                 [L[3], L[2], L[1], L[0]], rnd(B, 4, T)),
    }
    result = {"batch": B, "samples": T, "frames": Ts, "iters": a.iters}

    def make(names):
        parts = [branches[n] for n in names]
        params = [p for d, *_ in parts for p in d.parameters()]

        def step(native):
            for p in params:
                p.grad = None
            xs = [x.detach().requires_grad_(True) for _, x, *_ in parts]
            ys = [d.forward_native(x, sk, tg, nctx) if native else d(x, sk, tg)
                  for (d, _, sk, tg, _), x in zip(parts, xs)]
            torch.autograd.backward(ys, [g for *_, g in parts])
            return [y.detach() for y in ys], [x.grad for x in xs] + [p.grad for p in params]

        return step

    for name, names in (("freq", ["freq"]), ("time", ["time"]), ("both", ["freq", "time"])):
        step = make(names)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {"torch": [], "native": []}
        keep = {}
        for it in range(a.warmup + a.iters):
            for path in times:
                torch.cuda.synchronize()
                e0.record()
                out = step(path == "native")
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[path].append(e0.elapsed_time(e1))
                keep[path] = out
                del out
        (yt, gt), (yn, gn) = keep["torch"], keep["native"]
        sdr = min(float(10 * torch.log10(p.double().pow(2).sum() / (p.double() - q.double()).pow(2).sum()))
                  for p, q in zip(yt, yn))
        ggap = max(float((p - q).abs().max() / p.abs().max()) for p, q in zip(gt, gn))
        del keep, yt, gt, yn, gn
        # peak memory of one forward plus backward, above what is allocated before it (inputs, parameters)
        peak = {}
        for path in times:
            for d in (branches[n][0] for n in names):
                d.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = step(path == "native")
            torch.cuda.synchronize()
            peak[path] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
            del out
        # where the native time goes
        nctx.profile_start(None)
        step(True)
        kernels = {k["kernel"]: round(k["ms"], 3) for k in nctx.profile_stop() if k["kernel"].startswith("head_dec")}
        med = {k: statistics.median(v) for k, v in times.items()}
        result[name] = {"torch_ms": med["torch"], "native_ms": med["native"], "torch_over_native": med["torch"] / med["native"],
                        "torch_ms_min_max": [min(times["torch"]), max(times["torch"])],
                        "native_ms_min_max": [min(times["native"]), max(times["native"])],
                        "torch_peak_mib": peak["torch"], "native_peak_mib": peak["native"],
                        "native_kernels_ms": kernels, "output_sdr_db": sdr, "grad_gap_over_max": ggap}
        print(name, json.dumps(result[name]), flush=True)
        assert np.isfinite(sdr) and sdr > 90.0 and ggap < 1e-2, (sdr, ggap)    # timing two paths that disagree is moot
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
