// Decoder stage of the forward, per decode chunk: text cross-attention, the frequency and the time decoder side by
// side, then mask + iSTFT + branch sum (ATHTDemucs_v2.py:38-58, 82-139, 293-324).
#include "forward.h"

namespace athd_fwd {
namespace {

// ConvTranspose (k8, s4, p2) along H as two GEMMs, one per residue pair: output rows 4u+{0,1} read input rows
// u-1, u; rows 4u+{2,3} read u, u+1.  Each GEMM has N = 2*cout (columns >= cout belong to the odd residue).
// keep < 0: store all rows (4*H_in rows).  keep > 0: store only rows 4u+1, 4u+2 as slots 2u, 2u+1 (the only
// rows the following exact /4 bilinear resize reads); statistics (if st) still cover all four residues.
void conv_t(Run& r, const DecW& w, const void* A, int a_bf16, int nb, int H_in, int W, void* out, int out_bf16,
            double* st, int keep, const char* stage) {
    KStage kst(stage);
    if (w.ct4w && a_bf16 && out_bf16 && convt4_supported(w.cin, w.cout, nb, H_in, W)) {
        // dedicated pass (convt4.hip): weights resident in LDS, barrier-free waves over 32-row units
        ConvT4Desc q;
        q.x = (const uint16_t*)A; q.w = w.ct4w; q.bias = w.ct4b; q.out = (uint16_t*)out; q.stats = st;
        q.nb = nb; q.H = H_in; q.W = W; q.keep = keep < 0 ? 0 : 1;
        r.check(convt4_launch(q, r.s), "convt4");
        return;
    }
    // residues as column groups of cout columns, group g to output row o_stride * u + o_off + g * hi_row_off
    auto residues = [&](const GemmW& gw, int ntaps, int in_off) {
        GemmDesc g = conv_h(gw, A, a_bf16, nb, H_in, W, w.cin, ntaps, 1, in_off, 1, H_in);
        out_to(g, out, out_bf16, w.cout, (keep < 0 ? 4 : 2) * H_in);
        g.o_stride = keep < 0 ? 4 : 2;
        g.stats = st; g.col_split = w.cout;
        return g;
    };
    if (w.quad.w) {
        // all four residues in one GEMM (N = 4 cout, K = rows u-1 | u | u+1): the input is read once
        GemmDesc g = residues(w.quad, 3, -1);
        if (w.cin % 32 == 0) g.k_blk = w.cin;       // skip the zero third of K per residue pair (gemm3)
        if (keep < 0) { g.o_off = 0; g.store_mask = 15; }
        else { g.o_off = -1; g.store_mask = 6; }    // residues 1, 2 -> slots 2u, 2u+1; 0 and 3 feed the statistics
        r.gemm(g, "convt.quad");
        return;
    }
    // the pair GEMMs store all rows, and only the levels routed here have pair weights (ctx.h DecW)
    if (!w.pair[0].w || !w.pair[1].w || keep >= 0) { r.check(-2, "convt: no packed route"); return; }
    for (int pi = 0; pi < 2; ++pi) {
        GemmDesc g = residues(w.pair[pi], 2, pi == 0 ? -1 : 0);
        g.o_off = 2 * pi; g.store_mask = 3;
        r.gemm(g, pi == 0 ? "convt.pair01" : "convt.pair23");
    }
}

// one decode chunk: the state its stages share
struct Chunk {
    Run& r;
    const Dims& d;
    const Bufs& b;
    athd_ctx* c;
    int64_t s0, Bc;      // first segment and segment count
    int P, NI, ab;       // prompts, (segment, prompt) items = Bc * P, activations in bf16
    void text_attn(const float* enc, const uint16_t* enc_b, int64_t ntok, float* cond, void* Hm, float* Yb) const;
    // the last level's fields of a DecLastDesc: the folded weights and the level-3 skip = saved[0][:, :4], the
    // compact copy the encoder wrote (4 channels per row)
    void last_level(DecLastDesc& dl, const float* fold, const void* skip, int64_t H_skip) const {
        dl.NI = NI; dl.P = P;
        dl.fold = fold; dl.skip = skip; dl.skip_bf16 = ab; dl.H_skip = (int)H_skip; dl.C_skip = 4;
    }
    void freq_decoder(float* FO) const;
    float* time_decoder() const;
};

// ---- text cross-attention, closed form (ATHTDemucs_v2.py:38-58) ----
// The prompt enters only through the row vector a = attn_out (one key: softmax == 1), so with u = x + a
// (ATHTDemucs_v2.py:46-48):  h = GELU(W0 u + b0) = GELU(W0 x + c0),  y = u + W2 h + b2 = x + W2 h + c2  (c0, c2 per
// prompt, text_vec_kernel).  text.mlp0 multiplies the SEGMENT's x once and its epilogue writes the P prompts' h
// (F_PB, pfold = P); text.mlp2 adds the segment's x as the residual (res_div = P) and the prompt's c2.
void Chunk::text_attn(const float* enc, const uint16_t* enc_b, int64_t ntok, float* cond, void* Hm, float* Yb) const {
    KStage kst(ntok == d.Nf ? "text_attn.freq" : "text_attn.time");
    GemmDesc g = lin(c->mlp0, enc_b ? (const void*)enc_b : enc, enc_b ? 1 : 0, Bc, ntok, 384, Hm, ab);
    g.bias = nullptr; g.pbias = b.tc0; g.pfold = P; g.act = ACT_GELU;
    r.gemm(g, "text.mlp0");
    GemmDesc g2 = lin(c->mlp2, Hm, ab, NI, ntok, 384, Yb, 0);
    g2.bias = nullptr; g2.pbias = b.tc2; g2.res = enc; g2.res_div = P; g2.res_bs = ntok * 384;
    if (r.actbf) {
        // bf16 mode: norm_out in the GEMM's epilogue (gemm3 row-LayerNorm variant: 128 x 384 tiles hold whole
        // rows), x_cond written directly; Yb is not used
        g2.C = cond; g2.c_bf16 = 1; g2.ln_w = c->ta_nw; g2.ln_b = c->ta_nb;
        r.gemm(g2, "text.mlp2.ln");
        return;
    }
    r.gemm(g2, "text.mlp2");
    LnDesc l;
    l.x = Yb; l.nb = NI; l.N = ntok; l.C = 384; l.w = c->ta_nw; l.b = c->ta_nb; l.out = cond; l.out_bf16 = ab;
    layernorm_launch(l, r.s);
}

// ---- frequency decoder (ATHTDemucs_v2.py:82-104, 293-297): x_cond -> FO ----
void Chunk::freq_decoder(float* FO) const {
    const int64_t Ts = d.Tspec;
    const int ea = b.ea;
    void* const sv[4] = {eoff(b.saved[0], s0 * 512 * Ts * 48, ea), eoff(b.saved[1], s0 * 128 * Ts * 96, ea),
                         eoff(b.saved[2], s0 * 32 * Ts * 192, ea), eoff(b.saved[3], s0 * 8 * Ts * 384, ea)};
    // level 0: 8 -> 32 rows, GN+GELU (in place, fp32: every source row feeds ~Ts/32 output rows), resize to
    // Tspec rows, + 0.1 * resize(saved[3][:, :192])
    double* st = r.stats(NI);
    // (bf16 mode: the ConvT output G as bf16, its GroupNorm statistics taken by the GEMM epilogue before rounding)
    conv_t(r, c->fdec[0], b.x_cond, ab, NI, 8, (int)Ts, b.G, ab, st, -1, "fdec0");
    KStage kst("fdec0");
    // S = GELU(GN(ConvT0)): in place (fp32 mode) or as a bf16 copy, the A operand of the level-1 tap GEMM
    if (r.actbf)
        gn_gelu_bf16in_launch((const uint16_t*)b.G, (uint16_t*)b.S, NI, 32 * Ts * 192, 192, st, c->fdec[0].gnw,
                              c->fdec[0].gnb, r.s);
    else gn_gelu_launch(b.G, NI, 32 * Ts * 192, 192, st, c->fdec[0].gnw, c->fdec[0].gnb, r.s, false);
    // level 1 from the 32-row S = GELU(GN(ConvT0)) without materialising the resized 259-row input
    // (fdec_lr.hip): Z = S @ [W_0 .. W_7], Zs = skip3[:, :192] @ [W_0 .. W_7], then stats + merge passes
    KStage kst1("fdec1");
    const DecW& w1 = c->fdec[1];
    GemmDesc gz = conv1(w1.taps, r.actbf ? b.S : (const void*)b.G, ab, NI, 32, Ts, w1.cin);
    out_to(gz, b.Z, ab, w1.taps.N, 32);
    LowRankDesc lr;
    lr.steps = b.lrsteps;
    lr.Z = b.Z; lr.Zs = b.Zs; lr.z_bf16 = ab; lr.Hs = 32; lr.Hk = 8; lr.Hd = (int)Ts; lr.W = (int)Ts;
    lr.Co = w1.cout; lr.P = P; lr.NI = NI; lr.bias = w1.bias; lr.stats = r.stats(NI);
    lr.gn_w = w1.gnw; lr.gn_b = w1.gnb; lr.fast_gelu = ab;
    lr.skip = sv[2]; lr.skip_bf16 = ab; lr.H_skip = 32; lr.C_skip = 192;
    lr.out = b.D; lr.out_bf16 = ab;
    lr.S = gz.A; lr.Wt = w1.taps.w; lr.w_ld = w1.taps.Kp; lr.Ci = w1.cin;
    // bf16 mode: the statistics from Gram matrices of Z tiles computed in LDS (fdec1f.hip), which also stores
    // the merge pass's taps 0, 3, 4, 7 of Z (no Z GEMM)
    const bool gram = r.sw.fdec1_fused && b.gram && fdec1_gram_supported(lr);
    if (gram) { lr.z_taps = 4; lr.z4 = b.Z; }   // (z4: written by fdec1_gram_kernel)
    else r.gemm(gz, "fdec1.z");
    GemmDesc gs = conv1(w1.taps, sv[3], ab, Bc, 8, Ts, w1.cin);   // the skip's first 192 of its 384 channels
    gs.a_ld = 384;
    out_to(gs, b.Zs, ab, w1.taps.N, 8);
    r.gemm(gs, "fdec1.zs");
    r.check(fdec_lr_steps_launch(b.lrsteps, (int)Ts, 32, 8, 32, r.s), "fdec_lr_steps");
    if (gram) r.check(fdec1_gram_launch(lr, b.gram, b.gramq, r.s), "fdec1_gram");
    else r.check(fdec_lr_stats_launch(lr, r.s), "fdec_lr_stats");
    r.check(fdec_lr_merge_launch(lr, r.s), "fdec_lr_merge");
    // levels 2, 3: Tspec -> 4 Tspec rows; the /4 bilinear resize reads only rows 4d+1, 4d+2.
    // level 2 ConvT (only rows 4d+1, 4d+2 stored; statistics over all four residues), then its merge (GN +
    // GELU + resize + skip) fused with level 3 + resize + skip + freq_out 1x1 (4 -> 2) in one pass over the
    // stored ConvT rows (dec_last.hip::fdec_tail_kernel)
    const DecW& w = c->fdec[2];
    double* sti = r.stats(NI);
    conv_t(r, w, b.D, ab, NI, (int)Ts, (int)Ts, b.G, ab, sti, 1, "fdec2");
    KStage kst3("fdec3");
    DecLastDesc dl;
    dl.g = b.G; dl.g_bf16 = ab; dl.stats = sti; dl.gn_count = 4 * Ts * Ts * w.cout; dl.gn_w = w.gnw; dl.gn_b = w.gnb;
    dl.fast_gelu = ab; dl.skip2 = sv[1]; dl.skip2_bf16 = ab; dl.H_skip2 = 128; dl.C_skip2 = 96;
    dl.H = (int)Ts; dl.W = (int)Ts;
    last_level(dl, c->flast, eoff(b.sk4, s0 * 512 * Ts * 4, ea), 512);
    dl.out = FO;
    r.check(fdec_tail_launch(dl, r.s), "fdec_tail");
}

// ---- time decoder (ATHTDemucs_v2.py:125-139, 313-321): xt_cond -> time_out [NI][T][2], returned ----
float* Chunk::time_decoder() const {
    const void* svt[4] = {eoff(b.saved_t[0], s0 * d.L[1] * 48, b.ea), eoff(b.saved_t[1], s0 * d.L[2] * 96, b.ea),
                          eoff(b.saved_t[2], s0 * d.L[3] * 192, b.ea), eoff(b.saved_t[3], s0 * d.L[4] * 384, b.ea)};
    const void* const sk4t = eoff(b.sk4t, s0 * d.L[1] * 4, b.ea);
    const void* A = b.xt_cond;
    int64_t Lin = d.Nt;
    static const char* const kT[3] = {"tdec0", "tdec1", "tdec2"};
    for (int i = 0; i < 3; ++i) {
        const DecW& w = c->tdec[i];
        double* st = r.stats(NI);
        conv_t(r, w, A, ab, NI, (int)Lin, 1, b.Gt, ab, st, -1, kT[i]);
        KStage kst(kT[i]);
        const int64_t target = d.L[3 - i];       // lengths_t reversed
        MergeDesc m;
        m.src = b.Gt; m.src_bf16 = ab; m.H_src = (int)(4 * Lin); m.kept = 0; m.C = w.cout; m.fast_gelu = ab;
        m.stats = st; m.gn_count = 4 * Lin * w.cout; m.gn_w = w.gnw; m.gn_b = w.gnb;
        m.skip = svt[3 - i]; m.skip_bf16 = ab; m.H_skip = (int)d.L[4 - i]; m.C_skip = ENC_CH[3 - i]; m.P = P;
        m.out = b.Dt; m.out_bf16 = ab; m.H_out = (int)target; m.W = 1; m.NI = NI;
        if (i == 2) {
            // level 2's merge fused with level 3 + resize + skip + time_out 1x1 (4 -> 2) when 4 L1 == T
            // (dec_last.hip::tdec_tail_kernel): one pass over the ConvT output, xt2 -> Dt
            DecLastDesc dl;
            dl.g = b.Gt; dl.g_bf16 = ab; dl.Hg = (int)(4 * Lin); dl.stats = st; dl.gn_count = m.gn_count;
            dl.gn_w = w.gnw; dl.gn_b = w.gnb; dl.fast_gelu = ab;
            dl.skip2 = svt[1]; dl.skip2_bf16 = ab; dl.H_skip2 = (int)d.L[2]; dl.C_skip2 = ENC_CH[1];
            dl.H = (int)target; dl.T = d.T;
            last_level(dl, c->tlast, sk4t, d.L[1]);
            dl.out = b.Dt;
            if (tdec_tail_supported(dl)) {
                KStage kst3("tdec3");
                r.check(tdec_tail_launch(dl, r.s), "tdec_tail");
                return b.Dt;
            }
        }
        r.check(dec_merge_launch(m, r.s), "dec_merge");
        A = b.Dt;
        Lin = target;
    }
    // ragged T: level 3 + resize + skip + time_out 1x1 (4 -> 2) over the merged 48-channel input (dec_last.hip)
    KStage kst("tdec3");
    DecLastDesc dl;
    dl.in = b.Dt; dl.in_bf16 = ab; dl.H = (int)Lin; dl.T = d.T;
    last_level(dl, c->tlast, sk4t, d.L[1]);
    dl.out = b.Gt;
    r.check(tdec_last_launch(dl, r.s), "tdec_last");
    return b.Gt;
}

}  // namespace

void decode_chunk(Run& r, const Dims& d, const Bufs& b, int64_t s0, int64_t Bc, const float* text, bool text_per_item,
                  float* out, float* FO) {
    athd_ctx* c = r.c;
    KSection sec_dec("decoder");
    const int P = d.P;
    const int64_t Ts = d.Tspec;
    const Chunk k{r, d, b, c, s0, Bc, P, (int)(Bc * P), r.actbf ? 1 : 0};
    // Chunk ordering: the previous chunk's time branch (second stream) recorded ev_t after its text cross-attention,
    // i.e. after it read tc0 / tc2 / avec, and - in stream order - after the iSTFT of the chunk before it, the last
    // reader of the FO buffer this chunk's fdec_tail rewrites (FO[c & 1] == FO[(c - 2) & 1]).  Waiting on it here
    // orders both write-after-read pairs; at chunk 0 ev_t is the encoder's join, already waited on.
    if (s0 > 0) r.sp.chunk_wait_time();
    text_vec_launch(text_per_item ? text + s0 * 512 : text, k.NI, P, text_per_item ? 1 : 0, c->ta_maT, c->ta_ma, c->ta_mcT,
                    c->ta_mc, c->ta_m2b, b.avec, b.tc0, b.tc2, r.s);
    // fork after the prompt vectors: the time branch (its text cross-attention with its own Hmt / Ybt scratch, then
    // the time decoder with its own Gt / Dt buffers) runs on the second stream beside the frequency branch and the
    // iSTFT; the branches join before istft_ola_kernel, which reads both
    //   main writes: Hm, Yb, x_cond, G, D, S, Z, Zs, lrsteps, gram, gramq, FO / FO2 (reads avec, tc0, tc2, x_enc)
    //   time writes: Hmt, Ybt, xt_cond, Gt, Dt, then (after the join) ola_part and out (reads avec, tc0, tc2, xt_enc)
    if (!r.ok()) return;
    r.sp.fork();
    k.text_attn(b.x_enc + s0 * d.Nf * 384, b.x_enc_b ? b.x_enc_b + s0 * d.Nf * 384 : nullptr, d.Nf, b.x_cond, b.Hm, b.Yb);
    k.freq_decoder(FO);

    OnBranch on(r, TIME);
    k.text_attn(b.xt_enc + s0 * d.Nt * 384, b.xt_enc_b ? b.xt_enc_b + s0 * d.Nt * 384 : nullptr, d.Nt, b.xt_cond, b.Hmt, b.Ybt);
    r.sp.chunk_record_time();                     // tc0 / tc2 read: the next chunk may rewrite them
    r.xt2 = k.time_decoder();
    // join on the SECOND stream: the iSTFT runs there after both branches, so the next chunk's decoder (main stream)
    // overlaps it; its time branch follows it on the second stream in stream order (xt2 is the time decoder's buffer),
    // and forward_impl joins the second stream back into the caller's after the last chunk
    r.sp.main_into_time();
    // ---- mask + iSTFT + overlap-add + denorm + branch sum (ATHTDemucs_v2.py:297-324), one fused pass ----
    KStage kst("istft");
    istft_ola_launch(FO, k.NI, (int)Ts, P, d.T, b.specT + s0 * 2048 * Ts * 4, c->tw, r.actbf ? nullptr : c->tw64,
                     c->win, c->win2, r.xt2, b.tnorm_std + 2 * s0, out + s0 * P * 2 * d.T, b.ola_part, r.s);
}

}  // namespace athd_fwd
