// Test entries for the kernel launchers (libathd_ktest.so, tests/ktest.py).  No kernels here: every kt_* wrapper copies
// a flat descriptor of int64_t / pointer fields into the launcher's own descriptor and calls the launcher that
// libathd.so ships.  Not part of the product ABI (include/athd.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "attn.h"
#include "ctx.h"
#include "forward.h"
#include "gemm.h"
#include "kernels.h"
#include "pack.h"
#include "text_tower.h"

namespace athd {   // norm.hip, dec_last.hip, fdec1f.hip: the tuning constants next to their launchers
int dec_merge_run();
int dec_merge_maxp();
int dec_last_const(int which);
int fdec1_gram_wb();
int fdec1_gram_blocks();
}  // namespace athd

using namespace athd;

extern "C" {

struct KtGemm {
    void* A; int64_t a_bf16, nb, H_in, W, C_in, a_ld, a_cs, a_bs, a_hs, ntaps, in_stride, in_off, dil, H_out;
    void* a_norm; void* a_gn_stats; int64_t a_gn_count; void* a_gn_w; void* a_gn_b;
    void* Wp; int64_t N, K, Kp; void* bias;
    void* C; int64_t c_bf16, H_out_total, o_stride, o_off, ldo, col_off, c_bs, store; void* c4;
    int64_t col_split, hi_row_off, store_mask, k_blk, act;
    void* res; int64_t res_bf16; void* res_scale; void* res_gn_stats; int64_t res_gn_count; void* res_gn_w; void* res_gn_b;
    void* row_add; void* stats; void* gn_stats; int64_t gn_count; void* gn_w; void* gn_b;
    void* pbias; int64_t pfold, res_div, res_bs;
    void* ln_w; void* ln_b; void* ln_out; void* sk_ws;
};

struct KtAttn {
    void* Q; int64_t q_bf16, q_bs, q_ld, q_off;
    void* K; int64_t k_bf16, k_bs, k_ld, k_off;
    void* V; int64_t v_bf16, v_bs, v_ld, v_off;
    void* O; int64_t o_bf16, o_bs, o_ld;
    int64_t nb, Nq, Nk, heads;
    int64_t scale_bits;      // the f32 scale's bit pattern
};

struct KtLn {
    void* x; int64_t nb, N, C; void* w; void* b; void* gn_stats; void* gn_w; void* gn_b; int64_t gn_writeback;
    void* pos; void* out; int64_t out_bf16; void* w2; void* b2; void* out2;
};

struct KtConvT4 {
    void* x; void* w; void* bias; void* out; void* stats; int64_t nb, H, W, keep;
};

struct KtConv3 {
    void* x; void* w; int64_t kp; void* bias; void* h; void* st; int64_t M, L, C, dil;
};

struct KtApply {
    void* hb; void* w; int64_t kp; void* bias; void* st; void* gn_w; void* gn_b; void* scale; void* x; int64_t M, L, C;
    int64_t rewrite; void* rw_w; int64_t rw_kp; void* rw_bias; void* rw_out; void* rw_c4;
};

struct KtDcSmall {
    void* x; int64_t x_bf16; void* h; int64_t nb, L, C, dil; void* w3; void* b3; void* g1w; void* g1b; void* w1; void* b1;
    void* gram1; void* g2w; void* g2b; void* scale; void* st_h; void* st_y; int64_t fast;
};

struct KtGnMom {
    void* h; void* out; int64_t nb, L, H; void* stats; void* w; void* b; void* gram; void* st_y;
};

struct KtFencRow {
    void* in; void* a_norm; int64_t B, Fin, Fout, T; void* wc; int64_t wc_ld; void* bc;
    void* w3[2]; int64_t w3_ld; void* b3[2]; void* g1w[2]; void* g1b[2]; void* w1[2]; int64_t w1_ld; void* b1[2];
    void* g2w[2]; void* g2b[2]; void* gram[2]; void* scale[2]; void* wr; int64_t wr_ld; void* br; void* row_add;
    void* out; void* out4; int64_t cin, c;
};

int64_t kt_sizeof_conv3() { return (int64_t)sizeof(KtConv3); }
int64_t kt_sizeof_apply() { return (int64_t)sizeof(KtApply); }
int64_t kt_sizeof_dcsmall() { return (int64_t)sizeof(KtDcSmall); }
int64_t kt_sizeof_gnmom() { return (int64_t)sizeof(KtGnMom); }
int64_t kt_sizeof_fencrow() { return (int64_t)sizeof(KtFencRow); }
int64_t kt_sizeof_gemm() { return (int64_t)sizeof(KtGemm); }
int64_t kt_sizeof_attn() { return (int64_t)sizeof(KtAttn); }
int64_t kt_sizeof_ln() { return (int64_t)sizeof(KtLn); }
int64_t kt_sizeof_convt4() { return (int64_t)sizeof(KtConvT4); }

static GemmDesc to_desc(const KtGemm* k) {
    GemmDesc g;
    g.A = k->A; g.a_bf16 = (int)k->a_bf16; g.nb = (int)k->nb; g.H_in = (int)k->H_in; g.W = (int)k->W;
    g.C_in = (int)k->C_in; g.a_ld = (int)k->a_ld; g.a_cs = k->a_cs; g.a_bs = k->a_bs; g.a_hs = k->a_hs;
    g.ntaps = (int)k->ntaps; g.in_stride = (int)k->in_stride; g.in_off = (int)k->in_off; g.dil = (int)k->dil;
    g.H_out = (int)k->H_out;
    g.a_norm = (const float*)k->a_norm; g.a_gn_stats = (const double*)k->a_gn_stats; g.a_gn_count = k->a_gn_count;
    g.a_gn_w = (const float*)k->a_gn_w; g.a_gn_b = (const float*)k->a_gn_b;
    g.Wp = k->Wp; g.N = (int)k->N; g.K = (int)k->K; g.Kp = (int)k->Kp; g.bias = (const float*)k->bias;
    g.C = k->C; g.c_bf16 = (int)k->c_bf16; g.H_out_total = (int)k->H_out_total; g.o_stride = (int)k->o_stride;
    g.o_off = (int)k->o_off; g.ldo = (int)k->ldo; g.col_off = (int)k->col_off; g.c_bs = k->c_bs;
    g.store = (int)k->store; g.c4 = k->c4;
    g.col_split = (int)k->col_split; g.hi_row_off = (int)k->hi_row_off; g.store_mask = (int)k->store_mask;
    g.k_blk = (int)k->k_blk; g.act = (int)k->act;
    g.res = k->res; g.res_bf16 = (int)k->res_bf16; g.res_scale = (const float*)k->res_scale;
    g.res_gn_stats = (const double*)k->res_gn_stats; g.res_gn_count = k->res_gn_count;
    g.res_gn_w = (const float*)k->res_gn_w; g.res_gn_b = (const float*)k->res_gn_b;
    g.row_add = (const float*)k->row_add; g.stats = (double*)k->stats; g.gn_stats = (const double*)k->gn_stats;
    g.gn_count = k->gn_count; g.gn_w = (const float*)k->gn_w; g.gn_b = (const float*)k->gn_b;
    g.pbias = (const float*)k->pbias; g.pfold = (int)k->pfold; g.res_div = (int)k->res_div; g.res_bs = k->res_bs;
    g.ln_w = (const float*)k->ln_w; g.ln_b = (const float*)k->ln_b; g.ln_out = k->ln_out; g.sk_ws = (float*)k->sk_ws;
    return g;
}

int kt_gemm(const KtGemm* k, int mode, void* stream) { return gemm_launch(to_desc(k), mode, (hipStream_t)stream); }
int kt_gemm_route(const KtGemm* k, int mode) { return gemm_route(to_desc(k), mode); }
int64_t kt_sk_bytes() { return (int64_t)SK_WS_BYTES; }
int64_t kt_sk_resident(const KtGemm* k) { return gemm5_sk_resident(to_desc(k)); }
// out = {full, tail, S} of the launch gemm_launch would make for k (no split when the route is not gemm5's)
void kt_sk_plan(const KtGemm* k, int64_t* out) {
    const GemmDesc g = to_desc(k);
    SkPlan p = gemm5_sk_plan(g, gemm_route(g, 1) == ROUTE_GEMM5 ? gemm5_sk_resident(g) : 0);
    out[0] = p.full; out[1] = p.tail; out[2] = p.S;
}

static AttnDesc to_attn_desc(const KtAttn* k) {
    AttnDesc a;
    a.Q = k->Q; a.q_bf16 = (int)k->q_bf16; a.q_bs = k->q_bs; a.q_ld = (int)k->q_ld; a.q_off = (int)k->q_off;
    a.K = k->K; a.k_bf16 = (int)k->k_bf16; a.k_bs = k->k_bs; a.k_ld = (int)k->k_ld; a.k_off = (int)k->k_off;
    a.V = k->V; a.v_bf16 = (int)k->v_bf16; a.v_bs = k->v_bs; a.v_ld = (int)k->v_ld; a.v_off = (int)k->v_off;
    a.O = k->O; a.o_bf16 = (int)k->o_bf16; a.o_bs = k->o_bs; a.o_ld = (int)k->o_ld;
    a.nb = (int)k->nb; a.Nq = (int)k->Nq; a.Nk = (int)k->Nk; a.heads = (int)k->heads;
    const uint32_t bits = (uint32_t)k->scale_bits;
    memcpy(&a.scale, &bits, 4);
    return a;
}

int kt_attn(const KtAttn* k, int mode, void* stream) { return attn_launch(to_attn_desc(k), mode, (hipStream_t)stream); }
// the ping-pong form attn_pp_kernel<prio> (attn_pp.hip, linked into this library only)
int kt_attn_pp(const KtAttn* k, int prio, void* stream) { return attn_pp_launch(to_attn_desc(k), prio, (hipStream_t)stream); }

int kt_layernorm(const KtLn* k, void* stream) {
    LnDesc l;
    l.x = (float*)k->x; l.nb = (int)k->nb; l.N = k->N; l.C = (int)k->C; l.w = (const float*)k->w; l.b = (const float*)k->b;
    l.gn_stats = (const double*)k->gn_stats; l.gn_w = (const float*)k->gn_w; l.gn_b = (const float*)k->gn_b;
    l.gn_writeback = (int)k->gn_writeback; l.pos = (const float*)k->pos; l.out = k->out; l.out_bf16 = (int)k->out_bf16;
    l.w2 = (const float*)k->w2; l.b2 = (const float*)k->b2; l.out2 = k->out2;
    layernorm_launch(l, (hipStream_t)stream);
    return (int)hipGetLastError();
}

int kt_convt4(const KtConvT4* k, void* stream) {
    ConvT4Desc c;
    c.x = (const uint16_t*)k->x; c.w = (const uint16_t*)k->w; c.bias = (const float*)k->bias; c.out = (uint16_t*)k->out;
    c.stats = (double*)k->stats; c.nb = (int)k->nb; c.H = (int)k->H; c.W = (int)k->W; c.keep = (int)k->keep;
    return convt4_launch(c, (hipStream_t)stream);
}

int kt_to_bf16(const float* x, uint16_t* y, int64_t n, void* stream) {
    to_bf16_launch(x, y, n, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int kt_stats(const float* x, int64_t nb, int64_t n, double* stats, void* stream) {
    stats_launch(x, (int)nb, n, stats, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int kt_input_norm_params(const double* stats, int64_t nb, int64_t n, float* mean_inv, float* mean_std, void* stream) {
    input_norm_params_launch(stats, (int)nb, n, mean_inv, mean_std, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int kt_gn_gelu(float* h, int64_t nb, int64_t per_batch, int64_t H, const double* stats, const float* w, const float* b,
               int64_t fast, void* stream) {
    gn_gelu_launch(h, (int)nb, per_batch, (int)H, stats, w, b, (hipStream_t)stream, fast != 0);
    return (int)hipGetLastError();
}
int kt_gn_gelu_bf16(const float* h, uint16_t* out, int64_t nb, int64_t per_batch, int64_t H, const double* stats,
                    const float* w, const float* b, void* stream) {
    gn_gelu_bf16_launch(h, out, (int)nb, per_batch, (int)H, stats, w, b, (hipStream_t)stream);
    return (int)hipGetLastError();
}
// ---- the DConv kernels and the fused encoder rows ----
int kt_dconv_conv3(const KtConv3* k, void* stream) {
    DconvDesc d;
    d.x = k->x; d.w3 = (const uint16_t*)k->w; d.w3_kp = (int)k->kp; d.b3 = (const float*)k->bias; d.h = (float*)k->h;
    d.st_h = (double*)k->st; d.M = k->M; d.L = k->L; d.C = (int)k->C; d.dil = (int)k->dil;
    return dconv_conv3_launch(d, (hipStream_t)stream);
}
int kt_dconv_apply(const KtApply* k, void* stream) {
    DcRewrite rw;
    rw.w = (const uint16_t*)k->rw_w; rw.kp = (int)k->rw_kp; rw.bias = (const float*)k->rw_bias;
    rw.out = (uint16_t*)k->rw_out; rw.c4 = (uint16_t*)k->rw_c4;
    DconvDesc d;
    d.hb = (uint16_t*)k->hb; d.w1 = (const uint16_t*)k->w; d.w1_kp = (int)k->kp; d.b1 = (const float*)k->bias;
    d.st_y = (double*)k->st; d.g2w = (const float*)k->gn_w; d.g2b = (const float*)k->gn_b; d.scale = (const float*)k->scale;
    d.x = k->x; d.M = k->M; d.L = k->L; d.C = (int)k->C;
    return dconv_apply_launch(d, (hipStream_t)stream, k->rewrite ? &rw : nullptr);
}
int kt_dconv_small(const KtDcSmall* k, void* stream) {
    DconvDesc d;
    d.x = k->x; d.x_bf16 = (int)k->x_bf16; d.h = (float*)k->h; d.M = k->nb * k->L; d.L = k->L; d.C = (int)k->C;
    d.dil = (int)k->dil; d.w3f = (const float*)k->w3; d.b3 = (const float*)k->b3; d.g1w = (const float*)k->g1w;
    d.g1b = (const float*)k->g1b; d.w1f = (const float*)k->w1; d.b1 = (const float*)k->b1; d.gram = (const float*)k->gram1;
    d.g2w = (const float*)k->g2w; d.g2b = (const float*)k->g2b; d.scale = (const float*)k->scale;
    d.st_h = (double*)k->st_h; d.st_y = (double*)k->st_y; d.fast = k->fast != 0;
    return dconv_small_launch(d, (hipStream_t)stream);
}
int kt_gn_gelu_mom(const KtGnMom* k, void* stream) {
    DconvDesc d;
    d.h = (float*)k->h; d.hb = (uint16_t*)k->out; d.M = k->nb * k->L; d.L = k->L; d.C = 8 * (int)k->H;
    d.st_h = (double*)k->stats; d.g1w = (const float*)k->w; d.g1b = (const float*)k->b; d.gram = (const float*)k->gram;
    d.st_y = (double*)k->st_y;
    return gn_gelu_mom_launch(d, (hipStream_t)stream);
}
int kt_gn_gelu_bf16in(const uint16_t* h, uint16_t* out, int64_t nb, int64_t per_batch, int64_t H, const double* stats,
                      const float* w, const float* b, void* stream) {
    gn_gelu_bf16in_launch(h, out, (int)nb, per_batch, (int)H, stats, w, b, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int kt_fenc_row(const KtFencRow* k, void* stream) {
    FencRowDesc d;
    d.in = k->in; d.a_norm = (const float*)k->a_norm; d.B = (int)k->B; d.Fin = (int)k->Fin; d.Fout = (int)k->Fout;
    d.T = (int)k->T; d.wc = (const uint16_t*)k->wc; d.wc_ld = (int)k->wc_ld; d.bc = (const float*)k->bc;
    d.w3_ld = (int)k->w3_ld; d.w1_ld = (int)k->w1_ld;
    for (int i = 0; i < 2; ++i) {
        d.w3[i] = (const uint16_t*)k->w3[i]; d.b3[i] = (const float*)k->b3[i];
        d.g1w[i] = (const float*)k->g1w[i]; d.g1b[i] = (const float*)k->g1b[i];
        d.w1[i] = (const uint16_t*)k->w1[i]; d.b1[i] = (const float*)k->b1[i];
        d.g2w[i] = (const float*)k->g2w[i]; d.g2b[i] = (const float*)k->g2b[i];
        d.gram[i] = (const float*)k->gram[i]; d.scale[i] = (const float*)k->scale[i];
    }
    d.wr = (const uint16_t*)k->wr; d.wr_ld = (int)k->wr_ld; d.br = (const float*)k->br;
    d.row_add = (const float*)k->row_add; d.out = (uint16_t*)k->out; d.out4 = (uint16_t*)k->out4;
    return fenc_row_launch(d, (int)k->cin, (int)k->c, (hipStream_t)stream);
}
int kt_fenc_row_supported(int64_t cin, int64_t c, int64_t T) { return fenc_row_supported((int)cin, (int)c, (int)T); }
int kt_dconv_conv3_supported(int64_t C, int64_t H, int64_t kp, int64_t L) {
    return dconv_conv3_supported((int)C, (int)H, (int)kp, L);
}
int kt_dconv_apply_supported(int64_t C, int64_t H, int64_t kp, int64_t M) {
    return dconv_apply_supported((int)C, (int)H, (int)kp, M);
}
int kt_gn_gelu_mom_supported(int64_t H, int64_t L) { return gn_gelu_mom_supported((int)H, L); }
// out = {ok, valu, conv3_mfma, norm, apply_mfma, rewrite}
void kt_dconv_plan(int64_t mode, int64_t C, int64_t nb, int64_t L, int64_t rewrite_fusable, int64_t* out) {
    const DconvPlan p = dconv_plan((int)mode, (int)C, nb, L, rewrite_fusable != 0);
    out[0] = p.ok; out[1] = p.valu; out[2] = p.conv3_mfma; out[3] = p.norm; out[4] = p.apply_mfma; out[5] = p.rewrite;
}

// ---- the host-side packers of pack.h (no GPU) ----
int64_t kt_glu_src(int64_t pr, int64_t n) { return glu_src((int)pr, (int)n); }
int64_t kt_rewrite_perm(int64_t k) { return dconv_rewrite_perm((int)k); }
int64_t kt_host_f2bf(int64_t f32_bits) {
    const uint32_t u = (uint32_t)f32_bits;
    float f;
    memcpy(&f, &u, 4);
    return host_f2bf(f);
}
// out: H * H + 2 H + 2 floats
void kt_conv1x1_moments(const float* w, const float* b, int64_t N, int64_t H, int64_t round_bf16, float* out) {
    const std::vector<float> g = conv1x1_moments(std::vector<float>(w, w + N * H), std::vector<float>(b, b + N),
                                                 (int)N, (int)H, round_bf16 != 0);
    memcpy(out, g.data(), g.size() * sizeof(float));
}

// ---- the decoder kernels and the folded last level ----
struct KtMerge {
    void* src; int64_t src_bf16, H_src, kept, C; void* stats; int64_t gn_count; void* gn_w; void* gn_b;
    void* skip; int64_t skip_bf16, H_skip, C_skip, P; void* out; int64_t out_bf16, H_out, W, NI;
    void* proj_w; void* proj_b; int64_t fast_gelu;
};
struct KtLowRank {
    void* steps; void* Z; void* Zs; int64_t z_bf16, z_taps, Hs, Hk, Hd, W, Co, P, NI; void* bias; void* stats;
    void* gn_w; void* gn_b; int64_t fast_gelu; void* skip; int64_t skip_bf16, H_skip, C_skip; void* out; int64_t out_bf16;
    void* S; void* Wt; int64_t w_ld, Ci; void* z4; void* gram; void* gq;
};
struct KtDecLast {
    void* in; int64_t in_bf16, NI, P, H, W, T; void* fold; void* skip; int64_t skip_bf16, H_skip, C_skip; void* out;
    void* g; int64_t g_bf16, Hg; void* stats; int64_t gn_count; void* gn_w; void* gn_b; int64_t fast_gelu;
    void* skip2; int64_t skip2_bf16, H_skip2, C_skip2;
};
int64_t kt_sizeof_merge() { return (int64_t)sizeof(KtMerge); }
int64_t kt_sizeof_lowrank() { return (int64_t)sizeof(KtLowRank); }
int64_t kt_sizeof_declast() { return (int64_t)sizeof(KtDecLast); }
int64_t kt_sizeof_lrstep() { return (int64_t)sizeof(LrStep); }

int kt_dec_merge(const KtMerge* k, void* stream) {
    MergeDesc d;
    d.src = k->src; d.src_bf16 = (int)k->src_bf16; d.H_src = (int)k->H_src; d.kept = (int)k->kept; d.C = (int)k->C;
    d.stats = (const double*)k->stats; d.gn_count = k->gn_count; d.gn_w = (const float*)k->gn_w;
    d.gn_b = (const float*)k->gn_b; d.skip = k->skip; d.skip_bf16 = (int)k->skip_bf16; d.H_skip = (int)k->H_skip;
    d.C_skip = (int)k->C_skip; d.P = (int)k->P; d.out = k->out; d.out_bf16 = (int)k->out_bf16; d.H_out = (int)k->H_out;
    d.W = (int)k->W; d.NI = (int)k->NI; d.proj_w = (const float*)k->proj_w; d.proj_b = (const float*)k->proj_b;
    d.fast_gelu = (int)k->fast_gelu;
    return dec_merge_launch(d, (hipStream_t)stream);
}
static LowRankDesc to_lr(const KtLowRank* k) {
    LowRankDesc d;
    d.steps = (const LrStep*)k->steps; d.Z = k->Z; d.Zs = k->Zs; d.z_bf16 = (int)k->z_bf16; d.z_taps = (int)k->z_taps;
    d.Hs = (int)k->Hs; d.Hk = (int)k->Hk; d.Hd = (int)k->Hd; d.W = (int)k->W; d.Co = (int)k->Co; d.P = (int)k->P;
    d.NI = (int)k->NI; d.bias = (const float*)k->bias; d.stats = (double*)k->stats; d.gn_w = (const float*)k->gn_w;
    d.gn_b = (const float*)k->gn_b; d.fast_gelu = (int)k->fast_gelu; d.skip = k->skip; d.skip_bf16 = (int)k->skip_bf16;
    d.H_skip = (int)k->H_skip; d.C_skip = (int)k->C_skip; d.out = k->out; d.out_bf16 = (int)k->out_bf16;
    d.S = k->S; d.Wt = k->Wt; d.w_ld = (int)k->w_ld; d.Ci = (int)k->Ci; d.z4 = k->z4;
    return d;
}
int kt_fdec_lr_stats(const KtLowRank* k, void* stream) { return fdec_lr_stats_launch(to_lr(k), (hipStream_t)stream); }
int kt_fdec_lr_merge(const KtLowRank* k, void* stream) { return fdec_lr_merge_launch(to_lr(k), (hipStream_t)stream); }
int kt_fdec1_gram(const KtLowRank* k, void* stream) {
    return fdec1_gram_launch(to_lr(k), (float*)k->gram, (double*)k->gq, (hipStream_t)stream);
}
int kt_fdec1_gram_supported(const KtLowRank* k) { return fdec1_gram_supported(to_lr(k)); }
int kt_fdec_lr_steps(void* steps, int64_t Hd, int64_t Hs, int64_t Hk, int64_t H_skip, void* stream) {
    return fdec_lr_steps_launch((LrStep*)steps, (int)Hd, (int)Hs, (int)Hk, (int)H_skip, (hipStream_t)stream);
}
int64_t kt_fdec1_gram_floats(int64_t NI, int64_t W) { return fdec1_gram_floats(NI, (int)W); }
int64_t kt_fdec1_gram_q_doubles() { return fdec1_gram_q_doubles(); }
static DecLastDesc to_dl(const KtDecLast* k) {
    DecLastDesc d;
    d.in = k->in; d.in_bf16 = (int)k->in_bf16; d.NI = (int)k->NI; d.P = (int)k->P; d.H = (int)k->H; d.W = (int)k->W;
    d.T = k->T; d.fold = (const float*)k->fold; d.skip = k->skip; d.skip_bf16 = (int)k->skip_bf16;
    d.H_skip = (int)k->H_skip; d.C_skip = (int)k->C_skip; d.out = (float*)k->out; d.g = k->g; d.g_bf16 = (int)k->g_bf16;
    d.Hg = (int)k->Hg; d.stats = (const double*)k->stats; d.gn_count = k->gn_count; d.gn_w = (const float*)k->gn_w;
    d.gn_b = (const float*)k->gn_b; d.fast_gelu = (int)k->fast_gelu; d.skip2 = k->skip2; d.skip2_bf16 = (int)k->skip2_bf16;
    d.H_skip2 = (int)k->H_skip2; d.C_skip2 = (int)k->C_skip2;
    return d;
}
int kt_fdec_last(const KtDecLast* k, void* stream) { return fdec_last_launch(to_dl(k), (hipStream_t)stream); }
int kt_tdec_last(const KtDecLast* k, void* stream) { return tdec_last_launch(to_dl(k), (hipStream_t)stream); }
int kt_fdec_tail(const KtDecLast* k, void* stream) { return fdec_tail_launch(to_dl(k), (hipStream_t)stream); }
int kt_tdec_tail(const KtDecLast* k, void* stream) { return tdec_tail_launch(to_dl(k), (hipStream_t)stream); }
int kt_tdec_tail_supported(const KtDecLast* k) { return tdec_tail_supported(to_dl(k)); }
// the constants the tests' shape lists depend on
int64_t kt_fl_dc() { return dec_last_const(0); }
int64_t kt_ft_dc() { return dec_last_const(1); }
int64_t kt_tl_in() { return dec_last_const(2); }
int64_t kt_tt_rows() { return dec_last_const(3); }
int64_t kt_dm_run() { return dec_merge_run(); }
int64_t kt_merge_maxp() { return dec_merge_maxp(); }
int64_t kt_g_wb() { return fdec1_gram_wb(); }
int64_t kt_fdec1_gram_blocks() { return fdec1_gram_blocks(); }      // (queries the current device's CU count)
// pack.h dec_last_fold (host): w [48][4][8], b [4], P [2][4], pb [2] -> out (br 0: 298 floats, br 1: 780)
int64_t kt_dec_last_fold(const float* w, const float* b, const float* P, const float* pb, int64_t br, float* out) {
    const std::vector<float> f = dec_last_fold(std::vector<float>(w, w + 48 * 4 * 8), std::vector<float>(b, b + 4),
                                               std::vector<float>(P, P + 8), std::vector<float>(pb, pb + 2), (int)br);
    if (out) memcpy(out, f.data(), f.size() * sizeof(float));
    return (int64_t)f.size();
}
// pack.h ConvT residue rows (host) of w [cin][cout][8], b [cout].  form 0: convt_pair(pi) -> rows f32 [2 cout][2 cin],
// bias [2 cout]; 1: convt_quad -> rows f32 [4 cout][3 cin], bias [4 cout]; 2: convt4_rows -> rows bf16 [4 cout][2 cin],
// no bias.  Returns the number of row elements written.
int64_t kt_convt_rows(const float* w, const float* b, int64_t cin, int64_t cout, int64_t form, int64_t pi, void* rows,
                      float* bias) {
    const std::vector<float> wv(w, w + cin * cout * 8), bv(b, b + cout);
    if (form == 2) {
        const std::vector<uint16_t> q = convt4_rows(wv, bv, (int)cin, (int)cout);
        memcpy(rows, q.data(), q.size() * sizeof(uint16_t));
        return (int64_t)q.size();
    }
    const PackedRows p = form == 0 ? convt_pair(wv, bv, (int)cin, (int)cout, (int)pi) : convt_quad(wv, bv, (int)cin, (int)cout);
    memcpy(rows, p.w.data(), p.w.size() * sizeof(float));
    memcpy(bias, p.bias.data(), p.bias.size() * sizeof(float));
    return (int64_t)p.w.size();
}

int kt_gn_apply(float* x, int64_t nb, int64_t N, int64_t C, const double* stats, const float* w, const float* b,
                void* stream) {
    gn_apply_launch(x, (int)nb, N, (int)C, stats, w, b, (hipStream_t)stream);
    return (int)hipGetLastError();
}

// ---- the CLAP text tower's kernels (text_tower.hip; tests/ktest_text.py) ----
struct KtTtGemm {
    void* W; int64_t bf16; void* X; int64_t ldx, M, N, K; void* bias; void* res; int64_t ldr, act; void* part; void* out;
    int64_t ldo;
};
struct KtTtAttn { void* part; int64_t S; void* bias; void* mask; int64_t P, L; void* out; };
int64_t kt_sizeof_tt_gemm() { return (int64_t)sizeof(KtTtGemm); }
int64_t kt_sizeof_tt_attn() { return (int64_t)sizeof(KtTtAttn); }
// {S, W, KW} of the (N, K) shape's plan; 0 if the shape has none
int64_t kt_tt_gemm_plan(int64_t N, int64_t K, int64_t* out3) {
    const TtGemmPlan* p = tt_gemm_plan((int)N, (int)K);
    if (!p) return 0;
    out3[0] = p->S; out3[1] = p->W; out3[2] = p->KW;
    return 1;
}
// the skinny GEMM with its slice reduction: out = act(X W^T + bias (+ res)); part: S * M * N floats
int kt_tt_gemm(const KtTtGemm* d, void* stream) {
    const TtGemmPlan* p = tt_gemm_plan((int)d->N, (int)d->K);
    if (!p) return -1;
    int rc = tt_gemm_launch(d->bf16 != 0, d->W, (const float*)d->X, d->ldx, (int)d->M, *p, (float*)d->part,
                            (hipStream_t)stream);
    if (rc != 0) return rc;
    return tt_reduce_launch((const float*)d->part, p->S, (int)d->M, p->N, (const float*)d->bias, (const float*)d->res,
                            d->ldr, (int)d->act, (float*)d->out, d->ldo, (hipStream_t)stream);
}
int kt_tt_attn(const KtTtAttn* d, void* stream) {
    int rc = tt_init();
    if (rc != 0) return rc;
    return tt_attn_launch((const float*)d->part, (int)d->S, (const float*)d->bias, (const int32_t*)d->mask, (int)d->P,
                          (int)d->L, (float*)d->out, (hipStream_t)stream);
}

// ---- the spectral front and back end, the time encoder's first conv, the prompt vectors, the position tables ----
struct KtStft {
    void* wav; int64_t nb, T, Tspec; void* tw; void* tw64; void* win; void* specT; void* stats;
    int64_t pp_L, pp_left, pp_ext_left, pp_Lx;       // the explicit PadPlan (kt_stft_pad_plan gives the product's)
};
struct KtIstft {
    void* fo; int64_t NI, Tspec, P, T; void* spec; void* tw; void* tw64; void* win; void* win2; void* xt2; void* tnorm;
    void* out; void* part;
};
struct KtTconv0 { void* wav; int64_t nb, T, Lo; void* w; void* bias; void* tnorm; void* out; int64_t out_bf16; };
struct KtTextVec {
    void* text; int64_t NI, P, per_item; void* maT; void* ma; void* mcT; void* mc; void* b2; void* a; void* c0; void* c2;
};
int64_t kt_sizeof_stft() { return (int64_t)sizeof(KtStft); }
int64_t kt_sizeof_istft() { return (int64_t)sizeof(KtIstft); }
int64_t kt_sizeof_tconv0() { return (int64_t)sizeof(KtTconv0); }
int64_t kt_sizeof_textvec() { return (int64_t)sizeof(KtTextVec); }

int kt_stft(const KtStft* k, void* stream) {
    PadPlan pp;
    pp.L = k->pp_L; pp.left = k->pp_left; pp.ext_left = k->pp_ext_left; pp.Lx = k->pp_Lx;
    stft_launch((const float*)k->wav, (int)k->nb, k->T, pp, (int)k->Tspec, (const float2*)k->tw, (const double2*)k->tw64,
                (const float*)k->win, (float*)k->specT, (double*)k->stats, (hipStream_t)stream);
    return (int)hipGetLastError();
}
void kt_stft_pad_plan(int64_t T, int64_t Tspec, int64_t* out4) {
    const PadPlan pp = stft_pad_plan(T, Tspec);
    out4[0] = pp.L; out4[1] = pp.left; out4[2] = pp.ext_left; out4[3] = pp.Lx;
}
int kt_istft_ola(const KtIstft* k, void* stream) {
    istft_ola_launch((const float*)k->fo, (int)k->NI, (int)k->Tspec, (int)k->P, k->T, (const float*)k->spec,
                     (const float2*)k->tw, (const double2*)k->tw64, (const float*)k->win, (const float*)k->win2,
                     (const float*)k->xt2, (const float*)k->tnorm, (float*)k->out, (float*)k->part, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int64_t kt_istft_nwg(int64_t Tspec) { return istft_ola_nwg((int)Tspec); }
int64_t kt_istft_frames(int64_t Tspec) { return istft_ola_frames((int)Tspec); }
int64_t kt_istft_part_floats(int64_t NI, int64_t Tspec) { return istft_ola_part_floats(NI, (int)Tspec); }
int kt_tconv0(const KtTconv0* k, void* stream) {
    tconv0_launch((const float*)k->wav, (int)k->nb, k->T, k->Lo, (const float*)k->w, (const float*)k->bias,
                  (const float*)k->tnorm, k->out, (int)k->out_bf16, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int kt_text_vec(const KtTextVec* k, void* stream) {
    text_vec_launch((const float*)k->text, (int)k->NI, (int)k->P, (int)k->per_item, (const float*)k->maT,
                    (const float*)k->ma, (const float*)k->mcT, (const float*)k->mc, (const float*)k->b2, (float*)k->a,
                    (float*)k->c0, (float*)k->c2, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int kt_pos2d(float* out, int64_t Fr, int64_t T1, int64_t C, void* stream) {
    pos2d_launch(out, (int)Fr, (int)T1, (int)C, (hipStream_t)stream);
    return (int)hipGetLastError();
}
int kt_pos1d(float* out, int64_t T2, int64_t C, void* stream) {
    pos1d_launch(out, (int)T2, (int)C, (hipStream_t)stream);
    return (int)hipGetLastError();
}

// ---- the feature export of athd_encode (export.hip; tests/ktest_head.py) ----
struct KtExportCf { void* src; int64_t src_bf16, nb, rows, C, Cs; void* out; };
struct KtExportSpec { void* specT; int64_t B, Tspec; void* z; };
int64_t kt_sizeof_export_cf() { return (int64_t)sizeof(KtExportCf); }
int64_t kt_sizeof_export_spec() { return (int64_t)sizeof(KtExportSpec); }
int kt_export_cf(const KtExportCf* k, void* stream) {
    return export_cf_launch(k->src, (int)k->src_bf16, k->nb, k->rows, (int)k->C, (int)k->Cs, (float*)k->out,
                            (hipStream_t)stream);
}
int kt_export_spec(const KtExportSpec* k, void* stream) {
    return export_spec_launch((const float*)k->specT, k->B, k->Tspec, (float*)k->z, (hipStream_t)stream);
}

// ---- head training's output stage (head_grad.hip; tests/test_gpu_head_output.py) ----
// the device tables of a finalized context {tw, tw64, win, win2}, so that kt_istft_ola can run on the very tables
// athd_head_output uses
int kt_ctx_tables(const athd_ctx* c, void** out) {
    if (!c || !c->finalized || !out) return -1;
    out[0] = c->tw; out[1] = c->tw64; out[2] = c->win; out[3] = c->win2;
    return 0;
}

// ---- the forward's workspace layout (forward_plan.cpp; tests/test_workspace_refs.py, tests/test_gpu_workspace.py) ----
// unused bytes after every arena buffer of this context's forwards (Arena::gap)
int kt_set_arena_gap(athd_ctx* c, int64_t bytes) {
    if (!c || bytes < 0 || bytes % 256) return -1;
    c->arena_gap = (size_t)bytes;
    return 0;
}

// (offset, bytes) of every buffer of plan(), in plan()'s order (tests/ktest.py LAYOUT_NAMES), then the total at
// out[2 * count]; returns the count, also when cap is too small (nothing is written then).  bytes is the rounded size
// (next offset - this offset - gap); a slot that plan() leaves null has bytes == 0.  No context and no device: the
// arena's base is an address that is only ever subtracted again, so the null slots are plan()'s own.
int64_t kt_forward_layout(int bf16, int64_t decode_items, int64_t B, int64_t T, int P, int64_t gap, int64_t* out,
                          int64_t cap) {
    using namespace athd_fwd;
    if (B <= 0 || T <= 0 || P <= 0 || gap < 0 || decode_items <= 0) return -1;
    athd_ctx c;
    c.decode_items = decode_items;
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 40);
    Arena ar{base, 0, (size_t)gap};
    Bufs b{};
    const size_t total = plan(ar, make_dims(&c, B, T, P), b, bf16 != 0);
    const void* const slots[] = {
        b.stats, b.specT, b.snorm, b.tnorm_div, b.tnorm_std,
        b.saved[0], b.saved_t[0], b.saved[1], b.saved_t[1], b.saved[2], b.saved_t[2], b.saved[3], b.saved_t[3],
        b.sk4, b.sk4t, b.ybuf_t, b.hbuf_t, b.hbuf_b_t, b.ybuf, b.hbuf, b.hbuf_b, b.X, b.XT,
        b.H[0], b.H[1], b.H[2], b.H[3], b.QKV, b.O, b.F1, b.QKVt, b.Ot, b.F1t, b.pos2d, b.pos1d,
        b.x_enc, b.xt_enc, b.x_enc_b, b.xt_enc_b, b.avec, b.tc0, b.tc2, b.Hm, b.Yb, b.Hmt, b.Ybt, b.x_cond, b.xt_cond,
        b.G, b.D, b.Gt, b.Dt, b.S, b.Z, b.Zs, b.FO, b.FO2, b.ola_part, b.lrsteps, b.gram, b.gramq, b.skw[0], b.skw[1]};
    const int64_t n = (int64_t)(sizeof(slots) / sizeof(slots[0]));
    if (!out || cap < 2 * n + 1) return n;
    int64_t next = (int64_t)total;
    for (int64_t i = n - 1; i >= 0; --i) {
        if (slots[i]) {
            const int64_t off = (const char*)slots[i] - base;
            out[2 * i] = off;
            out[2 * i + 1] = next - off - gap;
            next = off;
        } else {
            out[2 * i] = next;
            out[2 * i + 1] = 0;
        }
    }
    out[2 * n] = (int64_t)total;
    return n;
}

}  // extern "C"
