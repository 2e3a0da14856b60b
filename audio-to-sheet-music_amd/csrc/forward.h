// Internal to the forward orchestration (forward*.cpp): shapes and workspace (Dims, Bufs), the run state (Run), the
// stream plan, the runtime switches, the GemmDesc builders and the stage prototypes.  The tensors' layout in HBM:
// DESIGN.md §2.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/athd.h"
#include "attn.h"
#include "ctx.h"
#include "gemm.h"
#include "kernels.h"
#include "prof.h"

namespace athd_fwd {

struct Dims {
    int64_t B = 0, T = 0;
    int P = 1, Tspec = 0;
    int F[5] = {2048, 512, 128, 32, 8};
    int64_t L[5] = {0, 0, 0, 0, 0};   // L[0] = T, L[i+1] = ceil(L[i]/4)
    int64_t Nf = 0, Nt = 0, Nmax = 0;
    int64_t Bc = 0, chunks = 0;       // samples per decode chunk, decode chunks
};

struct Bufs {
    float* specT;
    double* stats;
    int64_t nstats;     // number of double pairs
    float *snorm, *tnorm_div, *tnorm_std;
    // encoder activations: f32 in parity mode, bf16 in throughput mode (Bufs::ea bytes per element)
    void *saved[4], *saved_t[4];
    void *sk4, *sk4t;                 // channels 0..3 of saved[0] / saved_t[0] ([rows][4]): the decoders' level-3 skip
    void *ybuf, *ybuf_t;              // level buffers; *_t: the time encoder's (it runs on the second stream)
    float *hbuf, *hbuf_t;
    uint16_t *hbuf_b, *hbuf_b_t;      // bf16 mode: GELU(GN(hbuf)) as bf16, the A operand of the wide DConv 1x1 GEMMs
    int ea = 4;
    float *X, *XT;
    void *H[4], *QKV, *O, *F1;
    void *QKVt, *Ot, *F1t;            // the time branch's scratch (it runs on its own stream beside the freq branch)
    float *Gt, *Dt;                   // the time decoder's ConvT / merge buffers (second stream too)
    float *pos2d, *pos1d, *x_enc, *xt_enc;
    uint16_t *x_enc_b, *xt_enc_b;     // bf16 copies (throughput mode): the A operand of text.mlp0
    // decode (per chunk)
    float *avec, *tc0, *tc2;         // per-prompt attention vector and out_mlp row biases (text_vec_kernel)
    float *Yb, *x_cond, *xt_cond;
    void* Hm;
    float* Ybt;         // Ybt, Hmt: the time branch's text cross-attention scratch (it runs on the second stream)
    void* Hmt;
    float *G, *D, *FO;
    float* FO2 = nullptr;             // second freq-output buffer (chunks > 1): chunk c's iSTFT reads FO[c & 1] while
                                      // chunk c + 1's decoder writes the other one
    float* ola_part;    // boundary partial sums of the fused iSTFT (spectral.hip)
    LrStep* lrsteps;    // level-1 low-rank decoder step table (fdec_lr.hip)
    float* gram;        // level-1 statistics Gram blocks / quadratic forms (fdec1f.hip, bf16 mode)
    double* gramq;
    void *S, *Z, *Zs;   // freq level 1 re-associated (fdec_lr.hip): per-tap products of the 32 / 8 source rows
    float* skw[2] = {nullptr, nullptr};   // split-K tail scratch of the main / time branch (gemm5, GemmDesc::sk_ws)
};

// element offset into an encoder activation buffer (f32 or bf16 storage)
inline void* eoff(void* p, int64_t n, int ea) { return (char*)p + n * ea; }

// Runtime switches of the forward, read once per forward (forward_impl).  The A/B switches are off only when the
// value starts with '0'; ATHD_SERIAL is on for any non-empty value not starting with '0'.
//   ATHD_SERIAL=1       both branches on the caller's stream (profiling runs whose per-kernel times should be the
//                       kernel's own; also the behaviour while an athd_profile window is open)
//   ATHD_SK=0           no split-K tail of linear2 (gemm5)
//   ATHD_ROWLN=0        out_proj and the FFN's LayerNorm as two launches instead of rowln.hip
//   ATHD_FDEC1_FUSED=0  the unfused level-1 frequency decoder (Z by a GEMM, fdec_lr.hip's two passes), not fdec1f.hip
//   ATHD_FENC_ROW=0     the unfused implicit-GEMM + DConv path instead of fenc_row.hip
struct Switches {
    static bool env(const char* name, bool dflt) {
        const char* e = std::getenv(name);
        return dflt ? !(e && *e == '0') : (e && *e && *e != '0');
    }
    bool serial = env("ATHD_SERIAL", false), sk = env("ATHD_SK", true), rowln = env("ATHD_ROWLN", true),
         fdec1_fused = env("ATHD_FDEC1_FUSED", true), fenc_row = env("ATHD_FENC_ROW", true);
};

// first error of a forward: launch return codes and the stream plan's HIP calls end here
struct Status {
    int err = 0;
    std::string what;
    void check(int rc, const char* w) { if (rc != 0 && err == 0) { err = rc; what = w; } }
};

// The forward's stream plan: which stream a branch launches on and every event that orders the two branches.
// main = the caller's stream (frequency branch, and everything that is not forked); time = the context's second
// stream (time branch), or the caller's stream again in serial mode (ATHD_SERIAL, or a kernel profile is open: the
// per-kernel event times are then the kernel's own and not shared with a concurrent one).  The stream and the two
// events are created by athd_finalize: a forward creates no HIP objects, so it can be graph-captured from the first
// call.  fork / join / cross_join / main_into_time are issued in serial mode too (one stream: no effect); the three
// per-chunk operations are skipped there.
enum Branch { MAIN = 0, TIME = 1 };
struct StreamPlan {
    hipStream_t main, time;
    hipEvent_t ev_f, ev_t;      // recorded on main / on time
    bool serial;
    Status* st;

    StreamPlan(athd_ctx* c, hipStream_t caller, bool serial_, Status* st_)
        : main(caller), time(serial_ ? caller : c->s_time), ev_f(c->ev_f), ev_t(c->ev_t), serial(serial_), st(st_) {
        if (!c->s_time || !c->ev_f || !c->ev_t) st->check((int)hipErrorInvalidResourceHandle, "second stream");
    }
    void record(hipEvent_t ev, hipStream_t s) { st->check((int)hipEventRecord(ev, s), "event record"); }
    void wait(hipStream_t s, hipEvent_t ev) { st->check((int)hipStreamWaitEvent(s, ev, 0), "event wait"); }
    void fork() { record(ev_f, main); wait(time, ev_f); }   // the time branch starts after main's work so far
    void join() { record(ev_t, time); wait(main, ev_t); }   // main continues after the time branch
    void cross_join() {                                     // each branch continues after the other (transformer)
        record(ev_f, main); record(ev_t, time);
        wait(time, ev_f); wait(main, ev_t);
    }
    void main_into_time() { record(ev_f, main); wait(time, ev_f); }   // the decoder's join before the iSTFT
    // per decode chunk, two streams only: ev_t after the time branch's text cross-attention, which the next chunk's
    // main stream waits on (forward_dec.cpp decode_chunk); the last chunk's iSTFT back into the caller's stream
    void chunk_record_time() { if (!serial) record(ev_t, time); }
    void chunk_wait_time() { if (!serial) wait(main, ev_t); }
    void final_join() { if (!serial) join(); }
};

struct Run : Status {
    athd_ctx* c;
    const Switches sw;
    StreamPlan sp;
    hipStream_t s;          // the stream launches go to: main, or what an OnBranch guard selects
    int sk = 0;             // that branch's split-K scratch (Bufs::skw): one per stream, so 0 for both in serial mode
    int mode;
    bool actbf;
    double* st_next;
    float* xt2 = nullptr;   // time_out(time decoder) of the last decode chunk: Dt (fused tail) or Gt (ragged T)

    Run(athd_ctx* c_, hipStream_t caller, double* stats_pool)
        : c(c_), sp(c_, caller, sw.serial || c_->prof != nullptr, this), s(caller), mode(c_->mode),
          actbf(c_->mode == 1), st_next(stats_pool) {}
    // checked where a stage forks: false ends the stage (a context without its second stream, or an earlier error)
    bool ok() const { return err == 0; }
    double* stats(int64_t pairs) { double* p = st_next; st_next += 2 * pairs; return p; }
    void gemm(const GemmDesc& g, const char* w) {
        KSite site(w);
        check(gemm_launch(g, mode, s), w);
    }
};

// Scoped branch selection (as KStage / KSite): launches inside the scope go to the branch's stream and use its
// split-K scratch; the previous selection comes back at the end of the scope.
struct OnBranch {
    Run& r;
    const hipStream_t saved_s;
    const int saved_sk;
    OnBranch(Run& r_, Branch b) : r(r_), saved_s(r_.s), saved_sk(r_.sk) {
        r.s = b == TIME ? r.sp.time : r.sp.main;
        r.sk = b == TIME && !r.sp.serial ? 1 : 0;
    }
    ~OnBranch() { r.s = saved_s; r.sk = saved_sk; }
};

// ---- GemmDesc builders: call sites add only what is special to them (epilogue, statistics, residual, ...) ----
// Conv of `ntaps` taps along H of a channels-last A [nb][H_in][W][C_in] with the packed weights w:
// row ho reads input rows ho * in_stride + in_off + tap * dil
inline GemmDesc conv_h(const GemmW& w, const void* A, int a_bf16, int64_t nb, int64_t H_in, int64_t W, int C_in,
                       int ntaps, int in_stride, int in_off, int dil, int64_t H_out) {
    GemmDesc g;
    g.A = A; g.a_bf16 = a_bf16; g.nb = (int)nb; g.H_in = (int)H_in; g.W = (int)W; g.C_in = C_in; g.a_ld = C_in;
    g.ntaps = ntaps; g.in_stride = in_stride; g.in_off = in_off; g.dil = dil; g.H_out = (int)H_out;
    g.Wp = w.w; g.N = w.N; g.K = w.K; g.Kp = w.Kp; g.bias = w.bias;
    return g;
}
// 1x1 conv: the same rows out as in
inline GemmDesc conv1(const GemmW& w, const void* A, int a_bf16, int64_t nb, int64_t H, int64_t W, int C_in) {
    return conv_h(w, A, a_bf16, nb, H, W, C_in, 1, 1, 0, 1, H);
}
// output to C: ldo elements between positions, H_out_total rows per batch
inline void out_to(GemmDesc& g, void* C, int c_bf16, int ldo, int64_t H_out_total) {
    g.C = C; g.c_bf16 = c_bf16; g.ldo = ldo; g.H_out_total = (int)H_out_total;
}
// Linear layer on token rows: C[nb][ntok][n] = A[nb][ntok][:] @ W^T (+ epilogue)
inline GemmDesc lin(const GemmW& w, const void* A, int a_bf16, int64_t nb, int64_t ntok, int ldA, void* C, int c_bf16) {
    GemmDesc g = conv1(w, A, a_bf16, nb, ntok, 1, w.K);
    g.a_ld = ldA;
    out_to(g, C, c_bf16, w.N, ntok);
    return g;
}

// ---- stages ----
Dims make_dims(const athd_ctx* c, int64_t B, int64_t T, int P);                  // forward_plan.cpp
size_t plan(Arena& ar, const Dims& d, Bufs& b, bool actbf);
void dump_all(const Dims& d, const Bufs& b, const float* xt2, size_t gap, hipStream_t s);
void encode(Run& r, const Dims& d, const Bufs& b, const float* wav);             // forward_enc.cpp
void transformer(Run& r, const Dims& d, const Bufs& b);                          // forward_xf.cpp
// one decode chunk of Bc segments from segment s0 (sets r.xt2)                  // forward_dec.cpp
void decode_chunk(Run& r, const Dims& d, const Bufs& b, int64_t s0, int64_t Bc, const float* text, bool text_per_item,
                  float* out, float* FO);

}  // namespace athd_fwd
