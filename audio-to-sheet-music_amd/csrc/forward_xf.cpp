// Cross-transformer stage of the forward (ATHTDemucs_v2.py:219-234): channel up-projection, 5 layers on the
// frequency and the time branch (self, cross, self, cross, self), channel down-projection.
#include "forward.h"

namespace athd_fwd {
namespace {

// a GroupNorm(1) (norm_out of a layer) whose statistics exist but which has not been applied to the rows yet
struct Pending { const double* st = nullptr; const float* w = nullptr; const float* b = nullptr; };

// one branch's state across the layers
struct BranchX {
    float* X;            // the residual stream [B][N][512]
    int64_t N;
    void *QKV, *O, *F1;  // the branch's scratch
    Pending pend;        // norm_out of the last layer, applied by the next LayerNorm pass over X
    // bf16 mode: the LayerNorm pass that consumes a pending GroupNorm applies it in registers only, without writing
    // X / XT back; the branch's next out_proj applies the same GroupNorm to its residual read (GemmDesc::res_gn_*), the
    // only other reader of those raw rows (the cross layers' second norm of the same rows runs inside the same pass).
    // Saves the 271 MB (freq) / 136 MB (time) write-back per layer.  f32 mode keeps the write-back.
    Pending resgn;       // consumed by the last LayerNorm, due on the next out_proj residual
};

struct Xf {
    Run& r;
    const Dims& d;
    const Bufs& b;
    const int ab;        // activations in bf16

    // LayerNorm of x's rows to out (and, with w2, a second affine of the same rows to out2), applying x's pending
    // GroupNorm first
    void ln(BranchX& x, const float* w, const float* bb, bool pending, void* out, const float* w2 = nullptr,
            const float* b2 = nullptr, void* out2 = nullptr) {
        LnDesc l;
        l.x = x.X; l.nb = (int)d.B; l.N = x.N; l.C = 512; l.w = w; l.b = bb; l.out = out; l.out_bf16 = ab;
        if (pending && x.pend.st) {
            l.gn_stats = x.pend.st; l.gn_w = x.pend.w; l.gn_b = x.pend.b;
            // (the residual epilogue takes it when a 256-row tile spans at most two batches: N >= 256 tokens; the
            // LayerNorm pass has the register-only form only where ln_lazy_gn_ok holds)
            l.out2 = out2;
            if (r.actbf && x.N >= 256 && ln_lazy_gn_ok(l)) { l.gn_writeback = 0; x.resgn = x.pend; }
            x.pend = Pending();
        }
        l.w2 = w2; l.b2 = b2; l.out2 = out2;
        layernorm_launch(l, r.s);
    }
    // attention + FFN of one branch given LN'ed query rows Hq and key/value source (projected inside)
    void block(const TLayerW& L, BranchX& x, void* Hq, void* Hkv, int64_t Nk) {
        const int64_t B = d.B, N = x.N;
        AttnDesc a;
        a.nb = (int)B; a.Nq = (int)N; a.Nk = (int)Nk; a.heads = 8;
        a.scale = r.actbf ? ATTN_SCALE_PRESCALED : 0.125f;     // bf16: queries prescaled at pack time (attn.h)
        if (!L.cross) {
            r.gemm(lin(L.qkv, Hq, ab, B, N, 512, x.QKV, ab), "qkv");
            a.Q = x.QKV; a.q_bf16 = ab; a.q_bs = N * 1536; a.q_ld = 1536; a.q_off = 0;
            a.K = x.QKV; a.k_bf16 = ab; a.k_bs = N * 1536; a.k_ld = 1536; a.k_off = 512;
            a.V = x.QKV; a.v_bf16 = ab; a.v_bs = N * 1536; a.v_ld = 1536; a.v_off = 1024;
        } else {
            char* Qb = (char*)x.QKV;
            char* KVb = Qb + (size_t)B * d.Nmax * 512 * (ab ? 2 : 4);
            r.gemm(lin(L.q, Hq, ab, B, N, 512, Qb, ab), "q");
            r.gemm(lin(L.kv, Hkv, ab, B, Nk, 512, KVb, ab), "kv");
            a.Q = Qb; a.q_bf16 = ab; a.q_bs = N * 512; a.q_ld = 512; a.q_off = 0;
            a.K = KVb; a.k_bf16 = ab; a.k_bs = Nk * 1024; a.k_ld = 1024; a.k_off = 0;
            a.V = KVb; a.v_bf16 = ab; a.v_bs = Nk * 1024; a.v_ld = 1024; a.v_off = 512;
        }
        a.O = x.O; a.o_bf16 = ab; a.o_bs = N * 512; a.o_ld = 512;
        r.check(attn_launch(a, r.mode, r.s), "attention");
        GemmDesc go = lin(L.out, x.O, ab, B, N, 512, x.X, 0);
        go.res = x.X; go.res_scale = L.g1;
        if (x.resgn.st) {
            go.res_gn_stats = x.resgn.st; go.res_gn_count = N * 512; go.res_gn_w = x.resgn.w; go.res_gn_b = x.resgn.b;
            x.resgn = Pending();
        }
        const float *n2w = L.cross ? L.n3w : L.n2w, *n2b = L.cross ? L.n3b : L.n2b;
        go.ln_w = n2w; go.ln_b = n2b; go.ln_out = Hq;
        if (r.actbf && r.sw.rowln && rowln_supported(go)) {
            // bf16 mode: out_proj with the FFN's LayerNorm in its epilogue (rowln.hip: whole 512-column rows per
            // workgroup; the LayerNorm pass and its second read of X are gone)
            r.gemm(go, "out_proj.ln");
        } else {
            go.ln_w = go.ln_b = nullptr; go.ln_out = nullptr;
            r.gemm(go, "out_proj");
            ln(x, n2w, n2b, false, Hq);
        }
        GemmDesc g1 = lin(L.l1, Hq, ab, B, N, 512, x.F1, ab);
        g1.act = ACT_GELU;
        r.gemm(g1, "linear1");
        double* st = r.stats(B);
        GemmDesc g2 = lin(L.l2, x.F1, ab, B, N, 2048, x.X, 0);
        g2.res = x.X; g2.res_scale = L.g2; g2.stats = st;
        // K = 2048: the last partial round of tiles split along K (gemm5), with the current branch's scratch
        g2.sk_ws = r.sw.sk ? b.skw[r.sk] : nullptr;
        r.gemm(g2, "linear2");
        x.pend.st = st; x.pend.w = L.now; x.pend.b = L.nob;
    }
    void down(const GemmW& w, BranchX& x, float* enc, uint16_t* enc_b, const char* site) {   // channel down-projection
        GemmDesc g = lin(w, x.X, 0, d.B, x.N, 512, enc, 0);
        if (r.actbf) { g.a_gn_stats = x.pend.st; g.a_gn_count = x.N * 512; g.a_gn_w = x.pend.w; g.a_gn_b = x.pend.b; }
        r.gemm(g, site);
        if (enc_b) to_bf16_launch(enc, enc_b, d.B * x.N * 384, r.s);
    }
};

}  // namespace

void transformer(Run& r, const Dims& d, const Bufs& b) {
    athd_ctx* c = r.c;
    KStage xstage("transformer");
    KSection sec_x("transformer");
    const int64_t B = d.B;
    Xf xf{r, d, b, r.actbf ? 1 : 0};
    BranchX f{b.X, d.Nf, b.QKV, b.O, b.F1}, t{b.XT, d.Nt, b.QKVt, b.Ot, b.F1t};
    r.gemm(lin(c->up, b.saved[3], xf.ab, B, d.Nf, 384, b.X, 0), "upsampler");
    r.gemm(lin(c->up_t, b.saved_t[3], xf.ab, B, d.Nt, 384, b.XT, 0), "upsampler_t");
    pos2d_launch(b.pos2d, 8, d.Tspec, 512, r.s);
    pos1d_launch(b.pos1d, (int)d.Nt, 512, r.s);
    LnDesc l;
    l.x = b.X; l.nb = (int)B; l.N = d.Nf; l.C = 512; l.w = c->nin_w; l.b = c->nin_b; l.pos = b.pos2d; l.out = b.X;
    layernorm_launch(l, r.s);
    LnDesc lt;
    lt.x = b.XT; lt.nb = (int)B; lt.N = d.Nt; lt.C = 512; lt.w = c->nint_w; lt.b = c->nint_b; lt.pos = b.pos1d; lt.out = b.XT;
    layernorm_launch(lt, r.s);
    // Two streams: the frequency branch on the caller's stream, the time branch on ctx.s_time.  Self-attention
    // layers are independent per branch; a cross layer joins both streams (each waits for the other's previous
    // layer: the key/value norms below overwrite buffers the other branch read), computes its four norms, joins
    // again (each block reads the other branch's kv norm) and runs both blocks side by side.  Buffers: H[0] / H[1]
    // written only on the freq stream, H[2] / H[3] only on the time stream; separate QKV / O / F1 scratch.
    //   main writes: X, H[0], H[1], QKV, O, F1, skw[0], x_enc, x_enc_b (a cross layer reads H[3])
    //   time writes: XT, H[2], H[3], QKVt, Ot, F1t, skw[1], xt_enc, xt_enc_b (a cross layer reads H[1])
    if (!r.ok()) return;
    r.sp.fork();                                 // the time stream starts after everything issued so far
    for (int idx = 0; idx < 5; ++idx) {
        const TLayerW& Lf = c->L[idx];
        const TLayerW& Lt = c->Lt[idx];
        if (!Lf.cross) {
            xf.ln(f, Lf.n1w, Lf.n1b, true, b.H[0]);
            xf.block(Lf, f, b.H[0], nullptr, d.Nf);
            OnBranch on(r, TIME);
            xf.ln(t, Lt.n1w, Lt.n1b, true, b.H[2]);
            xf.block(Lt, t, b.H[2], nullptr, d.Nt);
        } else {
            r.sp.cross_join();
            // all four norms read the pre-layer X / XT (time branch attends to old_x, demucs transformer.py)
            // (bf16 mode: each pair is one pass over X / XT with two affines, layernorm_launch's out2)
            // pending GN applied to X; norm1(x) and the time branch's kv = norm2_t(old_x)
            xf.ln(f, Lf.n1w, Lf.n1b, true, b.H[0], Lt.n2w, Lt.n2b, b.H[1]);
            {
                OnBranch on(r, TIME);            // norm1_t(xt) and the freq branch's kv = norm2(xt)
                xf.ln(t, Lt.n1w, Lt.n1b, true, b.H[2], Lf.n2w, Lf.n2b, b.H[3]);
            }
            r.sp.cross_join();
            xf.block(Lf, f, b.H[0], b.H[3], d.Nt);
            OnBranch on(r, TIME);
            xf.block(Lt, t, b.H[2], b.H[1], d.Nf);
        }
    }
    // the last layer's pending GroupNorm: in the bf16 mode applied by the downsamplers' A load (gemm2 a_gn; X / XT
    // have no other reader), in the f32 mode written back first
    if (!r.actbf) gn_apply_launch(b.X, (int)B, d.Nf, 512, f.pend.st, f.pend.w, f.pend.b, r.s);
    {
        OnBranch on(r, TIME);                    // the time branch's channel downsampler on its own stream
        if (!r.actbf) gn_apply_launch(b.XT, (int)B, d.Nt, 512, t.pend.st, t.pend.w, t.pend.b, r.s);
        xf.down(c->down_t, t, b.xt_enc, b.xt_enc_b, "downsampler_t");
    }
    xf.down(c->down, f, b.x_enc, b.x_enc_b, "downsampler");
    r.sp.join();                                 // the caller's stream continues after the time branch
}

}  // namespace athd_fwd
