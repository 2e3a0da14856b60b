// Encoder stage of the forward: STFT + input normalisation, then the frequency and the time encoder side by side
// (ATHTDemucs_v2.py:197-217, 261-275; HEncLayer + DConv).
#include "forward.h"

namespace athd_fwd {
namespace {

// One encoder level's DConv (2 residual layers) on x viewed as [nb][L][C] (freq: nb = B*F rows along time), launched
// as dconv_plan (kernels.h) decides beforehand: the VALU layer, or conv3 (+stats) -> GN+GELU -> the 1x1 twice (its 2C
// outputs never touch HBM): for their GroupNorm statistics, unless the GN+GELU pass took those from the 1x1's moments,
// and again with GN -> GLU -> LayerScale -> residual in place.  A planned launcher that fails is an error.
// rw: the level's rewrite; returns whether the second layer's apply pass ran it (x then holds the first layer's output)
bool dconv(Run& r, const EncW& e, void* x, int64_t nb, int64_t L, float* hbuf, uint16_t* hbuf_b,
           const DcRewrite* rw = nullptr) {
    const int ab = r.actbf ? 1 : 0, C = e.cout, Hh = C / 8;
    const DConvW& w = e.dc;
    const DconvPlan p = dconv_plan(r.mode, C, nb, L, rw != nullptr);
    if (!p.ok) { r.check(ATHD_EHIP, "dconv: no route"); return false; }
    for (int dd = 0; dd < 2; ++dd) {
        DconvDesc d;
        d.x = x; d.x_bf16 = ab; d.h = hbuf; d.hb = hbuf_b; d.M = nb * L; d.L = L; d.C = C; d.dil = 1 << dd;
        d.st_h = r.stats(nb); d.st_y = r.stats(nb);
        d.b3 = w.c3[dd].bias; d.g1w = w.g1w[dd]; d.g1b = w.g1b[dd]; d.scale = w.scale[dd];
        if (p.valu) {   // narrow levels: HBM-bound VALU kernels (dconv_small.hip) on the natural-order f32 weights
            d.w3f = w.w3f[dd]; d.w1f = w.w1f[dd]; d.b1 = w.b1f[dd]; d.g2w = w.g2wf[dd]; d.g2b = w.g2bf[dd];
            d.gram = w.gram1[dd]; d.fast = r.actbf;
            KSite site(dd == 0 ? "dconv0" : "dconv1");
            r.check(dconv_small_launch(d, r.s), "dconv_small");
            continue;
        }
        d.w3 = (const uint16_t*)w.c3[dd].w; d.w3_kp = w.c3[dd].Kp; d.w1 = (const uint16_t*)w.c1[dd].w; d.w1_kp = w.c1[dd].Kp;
        d.b1 = w.c1[dd].bias; d.g2w = w.g2w[dd]; d.g2b = w.g2b[dd]; d.gram = w.gram1b[dd];
        if (p.conv3_mfma) {
            KSite site("dconv.conv3");
            r.check(dconv_conv3_launch(d, r.s), "dconv_conv3");
        } else {
            GemmDesc g = conv_h(w.c3[dd], x, ab, nb, L, 1, C, 3, 1, -d.dil, d.dil, L);
            out_to(g, hbuf, 0, Hh, L);
            g.stats = d.st_h;
            r.gemm(g, "dconv.conv3");
        }
        // bf16 mode: GELU(GN(h)) written once as bf16 (hbuf_b), so both 1x1 passes read half the bytes
        const bool hb = p.norm != DconvPlan::F32;
        {
            KSite site("dconv.gn_gelu");
            if (p.norm == DconvPlan::MOM) r.check(gn_gelu_mom_launch(d, r.s), "gn_gelu_mom");
            else if (hb) gn_gelu_bf16_launch(hbuf, hbuf_b, (int)nb, L * Hh, Hh, d.st_h, d.g1w, d.g1b, r.s);
            else gn_gelu_launch(hbuf, (int)nb, L * Hh, Hh, d.st_h, d.g1w, d.g1b, r.s, r.actbf);
        }
        GemmDesc g2 = conv1(w.c1[dd], hb ? (const void*)hbuf_b : (const void*)hbuf, hb ? 1 : 0, nb, L, 1, Hh);
        out_to(g2, x, ab, C, L);
        if (p.norm != DconvPlan::MOM) {
            GemmDesc g1 = g2;
            g1.stats = d.st_y; g1.store = 0;
            r.gemm(g1, "dconv.conv1x1.stats");
        }
        if (p.apply_mfma) {
            KSite site("dconv.conv1x1.apply");
            r.check(dconv_apply_launch(d, r.s, dd == 1 && p.rewrite ? rw : nullptr), "dconv_apply");
        } else {
            g2.act = ACT_GLU; g2.gn_stats = d.st_y; g2.gn_count = L * 2 * C; g2.gn_w = d.g2w; g2.gn_b = d.g2b;
            g2.res = x; g2.res_bf16 = ab; g2.res_scale = d.scale;
            r.gemm(g2, "dconv.conv1x1.apply");
        }
    }
    return p.rewrite;
}

// the rewrite 1x1 + GLU of an encoder level: y [nb][H][W][C] -> saved, its first 4 channels also to c4 (level 0)
GemmDesc rewrite_desc(const EncW& e, const void* y, int eab, int64_t nb, int64_t H, int64_t W, void* saved, void* c4) {
    GemmDesc g = conv1(e.rewrite, y, eab, nb, H, W, e.cout);
    out_to(g, saved, eab, e.cout, H);
    g.act = ACT_GLU;
    g.c4 = c4;
    return g;
}

// Frequency encoder level i on the current stream: conv (8,1)/(4,1) along freq rows, DConv, rewrite
void fenc_level(Run& r, const Dims& d, const Bufs& b, int i) {
    static const char* const kFenc[4] = {"fenc0", "fenc1", "fenc2", "fenc3"};
    KStage stage(kFenc[i]);
    athd_ctx* c = r.c;
    const EncW& e = c->fenc[i];
    const int64_t B = d.B, Ts = d.Tspec;
    const int C = e.cout, Fi = d.F[i], Fo = d.F[i + 1];
    const int eab = r.actbf ? 1 : 0;       // encoder activations in bf16 (throughput mode)
    const void* in = i == 0 ? (const void*)b.specT : (const void*)b.saved[i - 1];
    // the fused narrow level (fenc_row.hip) applies: bf16 mode, C in {48, 96}, T <= 272
    if (r.actbf && r.sw.fenc_row && fenc_row_supported(e.cin, e.cout, (int)Ts)) {
        // conv + GELU + DConv + rewrite GLU in one kernel per (b, f) row
        FencRowDesc fr;
        fr.in = in; fr.a_norm = i == 0 ? b.snorm : nullptr;
        fr.B = (int)B; fr.Fin = Fi; fr.Fout = Fo; fr.T = (int)Ts;
        fr.wc = (const uint16_t*)e.conv.w; fr.wc_ld = e.conv.Kp; fr.bc = e.conv.bias;
        for (int dd = 0; dd < 2; ++dd) {
            fr.w3[dd] = (const uint16_t*)e.dc.c3p[dd].w; fr.w3_ld = e.dc.c3p[dd].Kp; fr.b3[dd] = e.dc.c3[dd].bias;
            fr.g1w[dd] = e.dc.g1w[dd]; fr.g1b[dd] = e.dc.g1b[dd];
            fr.w1[dd] = (const uint16_t*)e.dc.c1[dd].w; fr.w1_ld = e.dc.c1[dd].Kp; fr.b1[dd] = e.dc.c1[dd].bias;
            fr.g2w[dd] = e.dc.g2w[dd]; fr.g2b[dd] = e.dc.g2b[dd]; fr.scale[dd] = e.dc.scale[dd];
            fr.gram[dd] = e.dc.gram1b[dd];
        }
        fr.wr = (const uint16_t*)e.rewrite.w; fr.wr_ld = e.rewrite.Kp; fr.br = e.rewrite.bias;
        fr.row_add = i == 0 ? c->femb : nullptr;
        fr.out = (uint16_t*)b.saved[i];
        fr.out4 = i == 0 ? (uint16_t*)b.sk4 : nullptr;
        KSite site("fenc_row");
        r.check(fenc_row_launch(fr, e.cin, C, r.s), "fenc_row");
        return;
    }
    GemmDesc g = conv_h(e.conv, in, i == 0 ? 0 : eab, B, Fi, Ts, e.cin, 8, 4, -2, 1, Fo);
    if (i == 0) {   // frame-major spectrogram: the 8 freq taps x 4 channels of a row are 128 contiguous bytes
        g.a_ld = 2048 * 4; g.a_hs = 4; g.a_bs = Ts * 2048 * 4;
        g.a_norm = b.snorm;
    }
    out_to(g, b.ybuf, eab, C, Fo);
    g.act = ACT_GELU;
    r.gemm(g, "fenc.conv");
    dconv(r, e, b.ybuf, B * Fo, Ts, b.hbuf, b.hbuf_b);
    GemmDesc gr = rewrite_desc(e, b.ybuf, eab, B, Fo, Ts, b.saved[i], i == 0 ? b.sk4 : nullptr);
    gr.row_add = i == 0 ? c->femb : nullptr;    // + freq_emb_scale * freq_emb(frs) (ATHTDemucs_v2.py:212-215)
    r.gemm(gr, "fenc.rewrite");
}

// Time encoder level i on the current stream; right zero-pad to a multiple of 4 is implicit (rows >= L read as 0)
void tenc_level(Run& r, const Dims& d, const Bufs& b, int i, const float* wav) {
    static const char* const kTenc[4] = {"tenc0", "tenc1", "tenc2", "tenc3"};
    KStage tstage(kTenc[i]);
    const EncW& et = r.c->tenc[i];
    const int64_t B = d.B, Li = d.L[i], Lo = d.L[i + 1];
    const int eab = r.actbf ? 1 : 0;
    if (i == 0) {
        KSite site("tenc.conv");
        tconv0_launch(wav, (int)B, d.T, Lo, et.conv_f32, et.conv.bias, b.tnorm_div, b.ybuf_t, eab, r.s);
    } else {
        GemmDesc gt = conv_h(et.conv, b.saved_t[i - 1], eab, B, Li, 1, et.cin, 8, 4, -2, 1, Lo);
        out_to(gt, b.ybuf_t, eab, et.cout, Lo);
        gt.act = ACT_GELU;
        r.gemm(gt, "tenc.conv");
    }
    void* const c4 = i == 0 ? b.sk4t : nullptr;
    DcRewrite rwt;
    rwt.w = (const uint16_t*)et.rewrite_perm.w; rwt.kp = et.rewrite_perm.Kp; rwt.bias = et.rewrite_perm.bias;
    rwt.out = (uint16_t*)b.saved_t[i]; rwt.c4 = (uint16_t*)c4;
    if (!dconv(r, et, b.ybuf_t, B, Lo, b.hbuf_t, b.hbuf_b_t, &rwt))
        r.gemm(rewrite_desc(et, b.ybuf_t, eab, B, Lo, 1, b.saved_t[i], c4), "tenc.rewrite");
}

}  // namespace

void encode(Run& r, const Dims& d, const Bufs& b, const float* wav) {
    athd_ctx* c = r.c;
    KSection sec_enc("encoder");
    const int64_t B = d.B, Ts = d.Tspec;
    // ---- STFT + CaC, input normalisation statistics (ATHTDemucs_v2.py:261-275) ----
    const PadPlan pp = stft_pad_plan(d.T, Ts);
    double *st_spec = r.stats(B), *st_wav = r.stats(B);
    stft_launch(wav, (int)B, d.T, pp, (int)Ts, c->tw, r.actbf ? nullptr : c->tw64, c->win, b.specT, st_spec, r.s);
    stats_launch(wav, (int)B, 2 * d.T, st_wav, r.s);
    input_norm_params_launch(st_spec, (int)B, 2048LL * Ts * 4, b.snorm, nullptr, r.s);
    input_norm_params_launch(st_wav, (int)B, 2 * d.T, b.tnorm_div, b.tnorm_std, r.s);

    // ---- encoders (ATHTDemucs_v2.py:197-217; HEncLayer + DConv) ----
    // fork: the time encoder runs on the second stream beside the frequency encoder; the branches join before the
    // transformer's up-projections.  (The waveform statistics stay before the fork: run as the time stream's first
    // kernels, beside the STFT, they measured 3 % slower per step - the time encoder's kernels then take CUs ahead
    // of the frequency encoder's level-0 rows.)
    //   main writes: ybuf, hbuf, hbuf_b, saved[], sk4 (reads specT, snorm)
    //   time writes: ybuf_t, hbuf_t, hbuf_b_t, saved_t[], sk4t (reads wav, tnorm_div)
    if (!r.ok()) return;
    r.sp.fork();
    for (int i = 0; i < 4; ++i) {
        fenc_level(r, d, b, i);
        OnBranch on(r, TIME);
        tenc_level(r, d, b, i, wav);
    }
    r.sp.join();
}

}  // namespace athd_fwd
