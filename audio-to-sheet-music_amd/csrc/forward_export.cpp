// athd_encode: the frozen half of the forward (encode + transformer stages, forward.h) followed by the feature export
// (export.hip) into caller-owned tensors, for a torch head that trains on them (athd/head.py).
#include "forward.h"

namespace athd_fwd {
namespace {

constexpr int SKIP_CH[4] = {DEC_CH[4], DEC_CH[3], DEC_CH[2], DEC_CH[1]};   // channels the decoders read of level i

bool features_complete(const athd_features* f) {
    if (!f || !f->x_enc || !f->xt_enc || !f->z || !f->meant || !f->stdt) return false;
    for (int i = 0; i < 4; ++i)
        if (!f->skip_f[i] || !f->skip_t[i]) return false;
    return true;
}

// Every source buffer is complete in the order of the caller's stream here: transformer() ends with StreamPlan::join(),
// after the time branch's last writer (downsampler_t; saved_t[], sk4t and xt_enc are written before it on that stream),
// so all launches go to the caller's stream and the exported tensors are ordered with whatever the caller enqueues next.
void export_features(Run& r, const Dims& d, const Bufs& b, const athd_features& f) {
    KStage stage("export");
    KSection sec("export");
    const int64_t B = d.B, Ts = d.Tspec;
    const int eab = r.actbf ? 1 : 0;
    r.check(export_cf_launch(b.x_enc, 0, B, d.Nf, 384, 384, f.x_enc, r.s), "export x_enc");
    r.check(export_cf_launch(b.xt_enc, 0, B, d.Nt, 384, 384, f.xt_enc, r.s), "export xt_enc");
    for (int i = 0; i < 4; ++i) {
        // level 0: the 4-channel copies the decoders read themselves (sk4 / sk4t), contiguous rows of 4
        const void* sf = i == 0 ? b.sk4 : b.saved[i];
        const void* st = i == 0 ? b.sk4t : b.saved_t[i];
        const int C = i == 0 ? 4 : ENC_CH[i];
        r.check(export_cf_launch(sf, eab, B, (int64_t)d.F[i + 1] * Ts, C, SKIP_CH[i], f.skip_f[i], r.s), "export skip_f");
        r.check(export_cf_launch(st, eab, B, d.L[i + 1], C, SKIP_CH[i], f.skip_t[i], r.s), "export skip_t");
    }
    r.check(export_spec_launch(b.specT, B, Ts, f.z, r.s), "export z");
    r.check(export_norm_launch(b.tnorm_std, B, f.meant, f.stdt, r.s), "export meant/stdt");
}

}  // namespace

// The checks, the workspace plan and the run set-up are forward_impl's, restated here so that athd_forward* keep their
// code path untouched; P = 1 gives the forward's own workspace layout (the decode buffers stay unused).
int encode_impl(athd_ctx* c, const float* wav, int64_t B, int64_t T, const athd_features* out, void* ws,
                size_t ws_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    if (!c->finalized) return c->fail(ATHD_ESTATE, "athd_encode before athd_finalize");
    if (!wav || B <= 0 || T <= 0) return c->fail(ATHD_EINVAL, "bad encode arguments");
    if (!features_complete(out)) return c->fail(ATHD_EINVAL, "athd_encode: a null member in athd_features");
    if (T > (int64_t)1 << 26) return c->fail(ATHD_EINVAL, "segment too long");
    const Dims d = make_dims(c, B, T, 1);
    Bufs b;
    Arena sz{nullptr, 0, c->arena_gap};
    const size_t need = plan(sz, d, b, c->mode == 1);
    if (!ws || ws_bytes < need) return c->fail(ATHD_EWORKSPACE, "workspace too small: need " + std::to_string(need));
    Arena ar{(char*)ws, 0, c->arena_gap};
    plan(ar, d, b, c->mode == 1);
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    Run r(c, (hipStream_t)stream, b.stats);
    if (hipMemsetAsync(b.stats, 0, (size_t)b.nstats * 2 * sizeof(double), r.s) != hipSuccess)
        return c->fail(ATHD_EHIP, "memset failed");
    struct ProfBind {
        KProf* saved;
        explicit ProfBind(KProf* p) : saved(t_kprof) { t_kprof = p; }
        ~ProfBind() { t_kprof = saved; }
    } prof_bind(c->prof);
    encode(r, d, b, wav);
    if (r.ok()) transformer(r, d, b);
    if (r.ok()) export_features(r, d, b, *out);
    if (r.err) return c->fail(ATHD_EHIP, "launch failed in " + r.what + " (code " + std::to_string(r.err) + ")");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return c->fail(ATHD_EHIP, std::string("HIP error: ") + hipGetErrorString(e));
    return ATHD_OK;
}

}  // namespace athd_fwd

extern "C" {

size_t athd_encode_workspace_bytes(athd_ctx* c, int64_t B, int64_t T) { return athd_workspace_bytes(c, B, T, 1); }

int athd_encode(athd_ctx* c, const float* wav, int64_t B, int64_t T, const athd_features* out, void* ws, size_t ws_bytes,
                void* stream) {
    return athd_fwd::encode_impl(c, wav, B, T, out, ws, ws_bytes, stream);
}

}  // extern "C"
