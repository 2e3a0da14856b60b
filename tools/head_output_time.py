"""Time of head training's output stage alone, forward plus backward: the torch ops of `TrainableHead.forward` against
`NativeOutputStage` (athd/head.py) on identical inputs, with device events, the two alternating in one process.

    python tools/head_output_time.py [--batch 8] [--samples 264600] [--iters 20] [--warmup 3] [--out FILE.json]

Per context dtype (f32: the double-FFT forward; bf16: the fast one; the backward kernel is the same) it prints the median
time of each path in ms, their ratio and the one-off `athd_pack_spectrum` time, and checks that the two paths agree
(output SDR, gradient gap over the largest |gradient|).  Needs the GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-to-sheet-music_amd"))


def torch_stage(head, xd, xtd, z, meant, stdt, T):
    """`TrainableHead.forward` from the mask on, as it stands in athd/head.py"""
    mask = torch.sigmoid(F.interpolate(xd, size=(z.shape[2], z.shape[3]), mode="bilinear", align_corners=False))
    mag_stereo = torch.stack((z[:, 0].real, z[:, 0].imag), dim=1)
    phase = z / (mag_stereo + 1e-8)
    freq_wav = head._ispec((mag_stereo * mask) * phase, T)
    return freq_wav + (xtd * stdt + meant)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=264600)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_output_time: no GPU (times are taken on the device only)")
    from athd.head import NativeOutputStage, TrainableHead
    from athd.model import AudioTextHTDemucs
    from athd.weights import STEMS, synthetic_state_dict, synthetic_text_table

    B, T = a.batch, a.samples
    Ts = -(-T // 1024)
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    # |Re z_0|, |Im z_0| away from the mask formula's singularity at -1e-8, as the parity inputs
    zr = rnd(B, 2, 2048, Ts, 2)
    zr[:, 0] = (0.25 + zr[:, 0].abs()) * torch.where(rnd(B, 2048, Ts, 2) < 0, -1.0, 1.0)
    z = torch.view_as_complex(zr.contiguous()).cuda()
    xd0, xtd0 = (2.0 * rnd(B, 2, Ts, Ts)).cuda(), rnd(B, 2, T).cuda()
    meant, stdt = (0.01 * rnd(B, 1, 1)).cuda(), (0.2 + 0.05 * rnd(B, 1, 1).abs()).cuda()
    g = rnd(B, 2, T).cuda()
    sd, table = synthetic_state_dict(seed=0), synthetic_text_table(4, seed=7)
    result = {"batch": B, "samples": T, "frames": Ts, "iters": a.iters}
    for dt in ("f32", "bf16"):
        model = AudioTextHTDemucs(dtype=dt, text_table={s: table[i] for i, s in enumerate(STEMS)})
        model.load_state_dict(sd)
        model.to("cuda:0").eval()
        head = TrainableHead(native_output=True).cuda().bind(model)
        nctx = model._ensure_ctx()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        spec = head.packed_spectrum(z)
        e1.record()
        torch.cuda.synchronize()
        object.__setattr__(head, "_spec_cache", None)
        e0.record()
        spec = head.packed_spectrum(z)
        e1.record()
        torch.cuda.synchronize()
        pack_ms = e0.elapsed_time(e1)
        paths = {"torch": lambda xd, xtd: torch_stage(head, xd, xtd, z, meant, stdt, T),
                 "native": lambda xd, xtd: NativeOutputStage.apply(xd, xtd, spec, meant, stdt, nctx)}
        times = {k: [] for k in paths}
        keep = {}
        for it in range(a.warmup + a.iters):
            for name, fn in paths.items():
                xd, xtd = xd0.clone().requires_grad_(True), xtd0.clone().requires_grad_(True)
                torch.cuda.synchronize()
                e0.record()
                out = fn(xd, xtd)
                out.backward(g)
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
                keep[name] = (out.detach(), xd.grad, xtd.grad)
        (ot, gt, xt), (on, gn, xn) = keep["torch"], keep["native"]
        sdr = float(10 * torch.log10(ot.double().pow(2).sum() / (ot.double() - on.double()).pow(2).sum()))
        ggap = float((gt - gn).abs().max() / gt.abs().max())
        med = {k: statistics.median(v) for k, v in times.items()}
        result[dt] = {"torch_ms": med["torch"], "native_ms": med["native"], "torch_over_native": med["torch"] / med["native"],
                      "torch_ms_min_max": [min(times["torch"]), max(times["torch"])],
                      "native_ms_min_max": [min(times["native"]), max(times["native"])], "pack_spectrum_ms": pack_ms,
                      "output_sdr_db": sdr, "logit_grad_gap_over_max": ggap,
                      "time_grad_equal": bool(torch.equal(xt, xn))}
        print(dt, json.dumps(result[dt]))
        assert np.isfinite(sdr) and sdr > 90.0 and ggap < 1e-4, (sdr, ggap)     # timing two paths that disagree is moot
        del model, head, nctx, spec, keep
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
