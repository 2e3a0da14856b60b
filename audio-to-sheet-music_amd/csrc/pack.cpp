// Weight packing for athd_finalize: the required state-dict keys, and one function per stage from the staged fp32
// host tensors (athd_ctx::host) to the context's device weights.  Layouts: pack.h (host), ctx.h up_gemm (device).
#include <cmath>

#include "attn.h"
#include "ctx.h"
#include "kernels.h"

namespace athd {

static std::vector<std::pair<std::string, std::vector<int64_t>>> make_required_keys() {
    std::vector<std::pair<std::string, std::vector<int64_t>>> r;
    auto dconv = [&](const std::string& p, int64_t c) {
        int64_t h = c / 8;
        for (int d = 0; d < 2; ++d) {
            std::string q = p + ".dconv.layers." + std::to_string(d);
            r.push_back({q + ".0.weight", {h, c, 3}});
            r.push_back({q + ".0.bias", {h}});
            r.push_back({q + ".1.weight", {h}});
            r.push_back({q + ".1.bias", {h}});
            r.push_back({q + ".3.weight", {2 * c, h, 1}});
            r.push_back({q + ".3.bias", {2 * c}});
            r.push_back({q + ".4.weight", {2 * c}});
            r.push_back({q + ".4.bias", {2 * c}});
            r.push_back({q + ".6.scale", {c}});
        }
    };
    int64_t cf = 4, ct = 2;
    for (int i = 0; i < 4; ++i) {
        int64_t c = ENC_CH[i];
        std::string p = "htdemucs.encoder." + std::to_string(i);
        r.push_back({p + ".conv.weight", {c, cf, 8, 1}});
        r.push_back({p + ".conv.bias", {c}});
        dconv(p, c);
        r.push_back({p + ".rewrite.weight", {2 * c, c, 1, 1}});
        r.push_back({p + ".rewrite.bias", {2 * c}});
        p = "htdemucs.tencoder." + std::to_string(i);
        r.push_back({p + ".conv.weight", {c, ct, 8}});
        r.push_back({p + ".conv.bias", {c}});
        dconv(p, c);
        r.push_back({p + ".rewrite.weight", {2 * c, c, 1}});
        r.push_back({p + ".rewrite.bias", {2 * c}});
        cf = ct = c;
    }
    r.push_back({"htdemucs.freq_emb.embedding.weight", {512, 48}});
    for (const char* s : {"", "_t"}) {
        std::string u = std::string("htdemucs.channel_upsampler") + s, d = std::string("htdemucs.channel_downsampler") + s;
        r.push_back({u + ".weight", {512, 384, 1}});
        r.push_back({u + ".bias", {512}});
        r.push_back({d + ".weight", {384, 512, 1}});
        r.push_back({d + ".bias", {384}});
    }
    const std::string ct_ = "htdemucs.crosstransformer";
    for (const char* s : {".norm_in", ".norm_in_t"}) {
        r.push_back({ct_ + s + ".weight", {512}});
        r.push_back({ct_ + s + ".bias", {512}});
    }
    for (int idx = 0; idx < 5; ++idx) {
        bool cross = idx % 2 == 1;
        for (const char* br : {".layers.", ".layers_t."}) {
            std::string p = ct_ + br + std::to_string(idx);
            std::string a = p + (cross ? ".cross_attn" : ".self_attn");
            r.push_back({a + ".in_proj_weight", {1536, 512}});
            r.push_back({a + ".in_proj_bias", {1536}});
            r.push_back({a + ".out_proj.weight", {512, 512}});
            r.push_back({a + ".out_proj.bias", {512}});
            r.push_back({p + ".linear1.weight", {2048, 512}});
            r.push_back({p + ".linear1.bias", {2048}});
            r.push_back({p + ".linear2.weight", {512, 2048}});
            r.push_back({p + ".linear2.bias", {512}});
            for (const char* n : {".norm1", ".norm2", ".norm3", ".norm_out"}) {
                if (!cross && std::string(n) == ".norm3") continue;
                r.push_back({p + n + ".weight", {512}});
                r.push_back({p + n + ".bias", {512}});
            }
            r.push_back({p + ".gamma_1.scale", {512}});
            r.push_back({p + ".gamma_2.scale", {512}});
        }
    }
    const std::string ta = "text_attn";
    r.push_back({ta + ".v_proj.weight", {384, 512}});
    r.push_back({ta + ".v_proj.bias", {384}});
    r.push_back({ta + ".attn.in_proj_weight", {1152, 384}});
    r.push_back({ta + ".attn.in_proj_bias", {1152}});
    r.push_back({ta + ".attn.out_proj.weight", {384, 384}});
    r.push_back({ta + ".attn.out_proj.bias", {384}});
    r.push_back({ta + ".out_mlp.0.weight", {384, 384}});
    r.push_back({ta + ".out_mlp.0.bias", {384}});
    r.push_back({ta + ".out_mlp.2.weight", {384, 384}});
    r.push_back({ta + ".out_mlp.2.bias", {384}});
    r.push_back({ta + ".norm_out.weight", {384}});
    r.push_back({ta + ".norm_out.bias", {384}});
    for (const char* name : {"freq_decoder", "time_decoder"}) {
        bool fr = std::string(name) == "freq_decoder";
        for (int i = 0; i < 4; ++i) {
            std::string p = std::string(name) + ".layers." + std::to_string(i);
            std::vector<int64_t> ws = {DEC_CH[i], DEC_CH[i + 1], 8};
            if (fr) ws.push_back(1);
            r.push_back({p + ".0.weight", ws});
            r.push_back({p + ".0.bias", {DEC_CH[i + 1]}});
            if (i < 3) {
                r.push_back({p + ".1.weight", {DEC_CH[i + 1]}});
                r.push_back({p + ".1.bias", {DEC_CH[i + 1]}});
            }
        }
    }
    r.push_back({"freq_out.weight", {2, 4, 1, 1}});
    r.push_back({"freq_out.bias", {2}});
    r.push_back({"time_out.weight", {2, 4, 1}});
    r.push_back({"time_out.bias", {2}});
    return r;
}

const std::vector<std::pair<std::string, std::vector<int64_t>>>& required_keys() {
    static const auto k = make_required_keys();
    return k;
}

void pack_encoders(athd_ctx& c) {
    int cf = 4, ct = 2;
    for (int i = 0; i < 4; ++i) {
        for (int br = 0; br < 2; ++br) {
            EncW& e = br == 0 ? c.fenc[i] : c.tenc[i];
            const int C = ENC_CH[i];
            const std::string p = std::string(br == 0 ? "htdemucs.encoder." : "htdemucs.tencoder.") + std::to_string(i);
            e.cin = br == 0 ? cf : ct;
            e.cout = C;
            e.conv = c.conv_gemm(p + ".conv.weight", p + ".conv.bias", C, e.cin, 8);
            e.rewrite = c.conv_gemm(p + ".rewrite.weight", p + ".rewrite.bias", 2 * C, C, 1, true);
            if (dconv_bf16(c.mode) && dconv_narrow(C)) {
                // the K order of the fused DConv apply (pack.h dconv_rewrite_perm)
                const auto& w = c.W(p + ".rewrite.weight").v;     // [2C][C]
                const int K2 = (C + 31) / 32 * 32;
                std::vector<float> q((size_t)2 * C * K2, 0.f);
                for (int n = 0; n < 2 * C; ++n) {
                    const int src = glu_src(n, 2 * C);
                    for (int k = 0; k < K2; ++k) {
                        const int ch = dconv_rewrite_perm(k);
                        if (ch < C) q[(size_t)n * K2 + k] = w[(size_t)src * C + ch];
                    }
                }
                e.rewrite_perm = c.up_gemm(q, 2 * C, K2, glu_order(c.W(p + ".rewrite.bias").v));
            }
            if (br == 1 && i == 0)                        // tconv0_kernel: [C][2][8] -> [C][tap * 2 + ci]
                e.conv_f32 = c.up_f32(conv_tap_major(c.W(p + ".conv.weight").v, C, 2, 8));
            for (int d = 0; d < 2; ++d) {
                const std::string q = p + ".dconv.layers." + std::to_string(d);
                e.dc.c3[d] = c.conv_gemm(q + ".0.weight", q + ".0.bias", C / 8, C, 3);
                // 1x1 conv in GLU pair order; its GroupNorm affine permuted identically (fused GN->GLU epilogue)
                e.dc.c1[d] = c.conv_gemm(q + ".3.weight", q + ".3.bias", 2 * C, C / 8, 1, true);
                e.dc.g1w[d] = c.up_key(q + ".1.weight");
                e.dc.g1b[d] = c.up_key(q + ".1.bias");
                e.dc.g2w[d] = c.up_f32(glu_order(c.W(q + ".4.weight").v));
                e.dc.g2b[d] = c.up_f32(glu_order(c.W(q + ".4.bias").v));
                e.dc.scale[d] = c.up_key(q + ".6.scale");
                if (dconv_narrow(C)) {
                    const int H = C / 8;
                    const std::vector<float> t3 = conv_tap_major(c.W(q + ".0.weight").v, H, C, 3);   // [H][tap*C + c]
                    e.dc.w3f[d] = c.up_f32(t3);
                    if (dconv_bf16(c.mode)) {
                        std::vector<float> t16((size_t)16 * 3 * C, 0.f);
                        std::copy(t3.begin(), t3.end(), t16.begin());
                        e.dc.c3p[d] = c.up_gemm(t16, 16, 3 * C, {});
                    }
                    e.dc.w1f[d] = c.up_key(q + ".3.weight");        // [2C][H][1] == [2C][H]
                    e.dc.gram1[d] = c.up_f32(conv1x1_moments(c.W(q + ".3.weight").v, c.W(q + ".3.bias").v, 2 * C, H, false));
                    if (dconv_bf16(c.mode))
                        e.dc.gram1b[d] = c.up_f32(conv1x1_moments(c.W(q + ".3.weight").v, c.W(q + ".3.bias").v, 2 * C, H, true));
                    e.dc.b1f[d] = c.up_key(q + ".3.bias");
                    e.dc.g2wf[d] = c.up_key(q + ".4.weight");
                    e.dc.g2bf[d] = c.up_key(q + ".4.bias");
                } else if (dconv_bf16(c.mode)) {      // wide levels: the 1x1's statistics from its moments (gn_gelu_mom)
                    e.dc.gram1b[d] = c.up_f32(conv1x1_moments(c.W(q + ".3.weight").v, c.W(q + ".3.bias").v, 2 * C, C / 8, true));
                }
            }
        }
        cf = ct = ENC_CH[i];
    }
    const auto& w = c.W("htdemucs.freq_emb.embedding.weight").v;
    std::vector<float> t(w.size());
    for (size_t i = 0; i < w.size(); ++i) t[i] = (w[i] * 10.0f) * 0.2f;   // ScaledEmbedding * freq_emb_scale
    c.femb = c.up_f32(t);
}

void pack_transformer(athd_ctx& c) {
    auto one = [&](const std::string& s, int N, int K) {
        const auto& w = c.W(s + ".weight").v;
        return c.up_gemm(w, N, K, c.W(s + ".bias").v);
    };
    c.up = one("htdemucs.channel_upsampler", 512, 384);
    c.down = one("htdemucs.channel_downsampler", 384, 512);
    c.up_t = one("htdemucs.channel_upsampler_t", 512, 384);
    c.down_t = one("htdemucs.channel_downsampler_t", 384, 512);
    const std::string ctp = "htdemucs.crosstransformer";
    c.nin_w = c.up_key(ctp + ".norm_in.weight");
    c.nin_b = c.up_key(ctp + ".norm_in.bias");
    c.nint_w = c.up_key(ctp + ".norm_in_t.weight");
    c.nint_b = c.up_key(ctp + ".norm_in_t.bias");
    for (int idx = 0; idx < 5; ++idx) {
        for (int br = 0; br < 2; ++br) {
            TLayerW& l = br == 0 ? c.L[idx] : c.Lt[idx];
            l.cross = idx % 2 == 1;
            const std::string p = ctp + (br == 0 ? ".layers." : ".layers_t.") + std::to_string(idx);
            const std::string a = p + (l.cross ? ".cross_attn" : ".self_attn");
            // bf16 mode: the query projection is prescaled by (1/sqrt(64)) * log2(e) so that the attention kernel's
            // scores come out in log2 units (attn.hip, attn32_kernel); f32 mode keeps the reference weights
            const float qs = c.mode == 1 ? ATTN_Q_PRESCALE : 1.f;
            if (l.cross) {
                l.q = c.lin_gemm(a + ".in_proj_weight", a + ".in_proj_bias", 0, 512, 512, qs);
                l.kv = c.lin_gemm(a + ".in_proj_weight", a + ".in_proj_bias", 512, 1024);
            } else {
                l.qkv = c.lin_gemm(a + ".in_proj_weight", a + ".in_proj_bias", 0, -1, 512, qs);
            }
            l.out = c.lin_gemm(a + ".out_proj.weight", a + ".out_proj.bias");
            l.l1 = c.lin_gemm(p + ".linear1.weight", p + ".linear1.bias");
            l.l2 = c.lin_gemm(p + ".linear2.weight", p + ".linear2.bias");
            l.n1w = c.up_key(p + ".norm1.weight");
            l.n1b = c.up_key(p + ".norm1.bias");
            l.n2w = c.up_key(p + ".norm2.weight");
            l.n2b = c.up_key(p + ".norm2.bias");
            if (l.cross) {
                l.n3w = c.up_key(p + ".norm3.weight");
                l.n3b = c.up_key(p + ".norm3.bias");
            }
            l.now = c.up_key(p + ".norm_out.weight");
            l.nob = c.up_key(p + ".norm_out.bias");
            l.g1 = c.up_key(p + ".gamma_1.scale");
            l.g2 = c.up_key(p + ".gamma_2.scale");
        }
    }
}

// Text cross-attention, closed form (single key => softmax == 1):
// v = Wv t + bv, vi = Wiv v + biv (the value third of in_proj), a = Wo vi + bo, c0 = W0 a + b0: affine in t, composed
// in double into a = Ma t + ma and c0 = Mc t + mc (384 x 512), uploaded transposed for text_vec_kernel
void pack_text_attn(athd_ctx& c) {
    const auto& wv = c.W("text_attn.v_proj.weight").v;          // [384][512]
    const auto& bv = c.W("text_attn.v_proj.bias").v;
    const auto& wi = c.W("text_attn.attn.in_proj_weight").v;     // [1152][384]: rows 768.. = value
    const auto& bi = c.W("text_attn.attn.in_proj_bias").v;
    const auto& wo = c.W("text_attn.attn.out_proj.weight").v;    // [384][384]
    const auto& bo = c.W("text_attn.attn.out_proj.bias").v;
    const auto& w0 = c.W("text_attn.out_mlp.0.weight").v;        // [384][384]
    const auto& b0 = c.W("text_attn.out_mlp.0.bias").v;
    constexpr int D = 384, TD = 512;
    std::vector<double> M0(wv.begin(), wv.end()), m0(bv.begin(), bv.end()), M1, m1, Ma, ma, Mc, mc;
    affine_compose(wi.data() + 768 * 384, bi.data() + 768, M0, m0, D, TD, M1, m1);
    affine_compose(wo.data(), bo.data(), M1, m1, D, TD, Ma, ma);
    affine_compose(w0.data(), b0.data(), Ma, ma, D, TD, Mc, mc);
    auto upT = [&](const std::vector<double>& M) {
        std::vector<float> t((size_t)TD * D);
        for (int r = 0; r < D; ++r)
            for (int k = 0; k < TD; ++k) t[(size_t)k * D + r] = (float)M[(size_t)r * TD + k];
        return c.up_f32(t);
    };
    c.ta_maT = upT(Ma);
    c.ta_mcT = upT(Mc);
    c.ta_ma = c.up_f32(std::vector<float>(ma.begin(), ma.end()));
    c.ta_mc = c.up_f32(std::vector<float>(mc.begin(), mc.end()));
    c.ta_m2b = c.up_key("text_attn.out_mlp.2.bias");
    c.mlp0 = c.lin_gemm("text_attn.out_mlp.0.weight", "text_attn.out_mlp.0.bias");
    c.mlp2 = c.lin_gemm("text_attn.out_mlp.2.weight", "text_attn.out_mlp.2.bias");
    c.ta_nw = c.up_key("text_attn.norm_out.weight");
    c.ta_nb = c.up_key("text_attn.norm_out.bias");
}

// Per level what its route reads (the table at ctx.h DecW); the last levels folded (dec_last.hip, dec_last_fold)
void pack_decoders(athd_ctx& c) {
    for (int br = 0; br < 2; ++br) {
        for (int i = 0; i < 3; ++i) {
            DecW& dw = br == 0 ? c.fdec[i] : c.tdec[i];
            const std::string p = std::string(br == 0 ? "freq_decoder" : "time_decoder") + ".layers." + std::to_string(i);
            dw.cin = DEC_CH[i];
            dw.cout = DEC_CH[i + 1];
            const auto& w = c.W(p + ".0.weight").v;
            const auto& b = c.W(p + ".0.bias").v;
            if (i == 2) {
                const PackedRows q = convt_quad(w, b, dw.cin, dw.cout);
                dw.quad = c.up_gemm(q.w, 4 * dw.cout, 3 * dw.cin, q.bias);
                if (c.mode == 1 && convt4_supported(dw.cin, dw.cout, 1, 32, 1)) {
                    const std::vector<uint16_t> q2 = convt4_rows(w, b, dw.cin, dw.cout);
                    dw.ct4w = c.dalloc<uint16_t>(q2.size());
                    c.h2d(dw.ct4w, q2.data(), q2.size() * 2);
                    dw.ct4b = c.up_f32(b);
                }
            } else if (br == 0 && i == 1) {           // [k*cout + co][ci] for the re-associated level 1
                std::vector<float> tk((size_t)8 * dw.cout * dw.cin);
                for (int k = 0; k < 8; ++k)
                    for (int co = 0; co < dw.cout; ++co)
                        for (int ci = 0; ci < dw.cin; ++ci)
                            tk[((size_t)k * dw.cout + co) * dw.cin + ci] = w[((size_t)ci * dw.cout + co) * 8 + k];
                dw.taps = c.up_gemm(tk, 8 * dw.cout, dw.cin, {});
                dw.bias = c.up_f32(b);
            } else {
                for (int pi = 0; pi < 2; ++pi) {
                    const PackedRows pk = convt_pair(w, b, dw.cin, dw.cout, pi);
                    dw.pair[pi] = c.up_gemm(pk.w, 2 * dw.cout, 2 * dw.cin, pk.bias);
                }
            }
            dw.gnw = c.up_key(p + ".1.weight");
            dw.gnb = c.up_key(p + ".1.bias");
        }
    }
    for (int br = 0; br < 2; ++br) {
        const std::string p = std::string(br == 0 ? "freq_decoder" : "time_decoder") + ".layers.3.0.";
        (br == 0 ? c.flast : c.tlast) =
            c.up_f32(dec_last_fold(c.W(p + "weight").v, c.W(p + "bias").v,
                                   c.W(br == 0 ? "freq_out.weight" : "time_out.weight").v,
                                   c.W(br == 0 ? "freq_out.bias" : "time_out.bias").v, br));
    }
}

// FFT twiddles and the periodic Hann window (torch.hann_window(4096))
void pack_tables(athd_ctx& c) {
    std::vector<float2> tw(4096);
    std::vector<double2> tw64(4096);
    std::vector<float> win(4096), win2(4096);
    for (int k = 0; k < 4096; ++k) {
        const double a = -2.0 * M_PI * (double)k / 4096.0;
        tw[k] = make_float2((float)cos(a), (float)sin(a));
        tw64[k] = make_double2(cos(a), sin(a));
        const float w = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)k / 4096.0));
        win[k] = w;
        win2[k] = w * w;
    }
    c.tw = c.dalloc<float2>(4096);
    c.h2d(c.tw, tw.data(), 4096 * sizeof(float2));
    c.tw64 = c.dalloc<double2>(4096);
    c.h2d(c.tw64, tw64.data(), 4096 * sizeof(double2));
    c.win = c.up_f32(win);
    c.win2 = c.up_f32(win2);
}

}  // namespace athd
