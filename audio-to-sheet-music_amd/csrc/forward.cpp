// athd forward orchestration: AudioTextHTDemucs.forward (ATHTDemucs_v2.py:250-326) as a sequence of HIP kernels on
// the caller's stream and the context's second stream (forward.h: the stages and the stream plan).
#include "forward.h"

namespace athd_fwd {

int forward_impl(athd_ctx* c, const float* wav, int64_t B, int64_t T, const float* text, bool per_item, int P,
                 float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    if (!c->finalized) return c->fail(ATHD_ESTATE, "athd_forward before athd_finalize");
    if (!wav || !text || !out || B <= 0 || T <= 0 || P <= 0) return c->fail(ATHD_EINVAL, "bad forward arguments");
    if (P > 256) return c->fail(ATHD_EINVAL, "at most 256 prompts per athd_forward_prompts call");
    if (T > (int64_t)1 << 26) return c->fail(ATHD_EINVAL, "segment too long");
    const Dims d = make_dims(c, B, T, P);
    Bufs b;
    Arena sz{nullptr, 0, c->arena_gap};
    const size_t need = plan(sz, d, b, c->mode == 1);
    if (!ws || ws_bytes < need) return c->fail(ATHD_EWORKSPACE, "workspace too small: need " + std::to_string(need));
    Arena ar{(char*)ws, 0, c->arena_gap};
    plan(ar, d, b, c->mode == 1);
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    Run r(c, (hipStream_t)stream, b.stats);   // reads the runtime switches and sets up the stream plan
    if (hipMemsetAsync(b.stats, 0, (size_t)b.nstats * 2 * sizeof(double), r.s) != hipSuccess)
        return c->fail(ATHD_EHIP, "memset failed");
    struct ProfBind {   // route this call's launches into the context's profile window (prof.h)
        KProf* saved;
        explicit ProfBind(KProf* p) : saved(t_kprof) { t_kprof = p; }
        ~ProfBind() { t_kprof = saved; }
    } prof_bind(c->prof);
    encode(r, d, b, wav);
    if (r.ok()) transformer(r, d, b);
    for (int64_t ch = 0; ch < d.chunks && r.err == 0; ++ch) {
        const int64_t s0 = ch * d.Bc;
        const int64_t bc = std::min(d.Bc, B - s0);
        decode_chunk(r, d, b, s0, bc, text, per_item, out, (ch & 1) && b.FO2 ? b.FO2 : b.FO);
    }
    if (r.ok()) r.sp.final_join();   // the last chunk's iSTFT (second stream) joins the caller's stream
    if (d.chunks == 1) dump_all(d, b, r.xt2, c->arena_gap, r.s);
    if (r.err) return c->fail(ATHD_EHIP, "launch failed in " + r.what + " (code " + std::to_string(r.err) + ")");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return c->fail(ATHD_EHIP, std::string("HIP error: ") + hipGetErrorString(e));
    return ATHD_OK;
}

}  // namespace athd_fwd

using namespace athd_fwd;

extern "C" {

size_t athd_workspace_bytes(athd_ctx* c, int64_t B, int64_t T, int P) {
    if (!c || B <= 0 || T <= 0 || P <= 0) return 0;
    Bufs b;
    Arena a{nullptr, 0, c->arena_gap};
    return plan(a, make_dims(c, B, T, P), b, c->mode == 1);
}

int athd_forward(athd_ctx* c, const float* wav, int64_t B, int64_t T, const float* text_emb, float* out, void* ws,
                 size_t ws_bytes, void* stream) {
    return forward_impl(c, wav, B, T, text_emb, true, 1, out, ws, ws_bytes, stream);
}

int athd_forward_prompts(athd_ctx* c, const float* wav, int64_t B, int64_t T, const float* text_table, int P,
                         float* out, void* ws, size_t ws_bytes, void* stream) {
    return forward_impl(c, wav, B, T, text_table, false, P, out, ws, ws_bytes, stream);
}

}  // extern "C"
