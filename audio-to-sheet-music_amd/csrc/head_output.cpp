// Head training's output stage behind the C ABI (include/athd.h): the packed spectrogram, the forward (the inference
// path's fused mask + iSTFT, spectral.hip, with P = 1) and its adjoint with respect to the logits (head_grad.hip).
// Each entry checks its arguments, enqueues on the caller's stream and returns: no host synchronisation, no HIP object.
#include <string>

#include "../../include/athd.h"
#include "ctx.h"
#include "kernels.h"

namespace {

constexpr int64_t HOP = 1024, MAX_TS = 2048, MAX_B = 65535;

// shared by the three entries: the context's state, then the shape
int check(athd_ctx* c, const char* what, bool ptrs_ok, int64_t B) {
    if (!c->finalized) return c->fail(ATHD_ESTATE, std::string(what) + " before athd_finalize");
    if (!ptrs_ok) return c->fail(ATHD_EINVAL, std::string(what) + ": a null pointer");
    if (B <= 0 || B > MAX_B) return c->fail(ATHD_EINVAL, std::string(what) + ": B must be in [1, 65535]");
    return ATHD_OK;
}

int check_T(athd_ctx* c, const char* what, int64_t T) {
    if (T <= 0) return c->fail(ATHD_EINVAL, std::string(what) + ": T must be positive");
    if ((T + HOP - 1) / HOP > MAX_TS)
        return c->fail(ATHD_EINVAL, std::string(what) + ": more than 2048 frames (T > 2097152): the logits' resize to "
                                                        "2048 bins would be a downsample, which the adjoint does not cover");
    return ATHD_OK;
}

int finish(athd_ctx* c, const char* what, int rc) {
    if (rc == -1) return c->fail(ATHD_EINVAL, std::string(what) + ": bad shape");
    if (rc != 0) return c->fail(ATHD_EHIP, std::string(what) + ": launch failed (code " + std::to_string(rc) + ")");
    return ATHD_OK;
}

}  // namespace

extern "C" {

int athd_pack_spectrum(athd_ctx* c, const float* z, int64_t B, int64_t Ts, float* spec, void* stream) {
    if (!c) return ATHD_EINVAL;
    if (int rc = check(c, "athd_pack_spectrum", z && spec, B)) return rc;
    if (Ts <= 0 || Ts > MAX_TS) return c->fail(ATHD_EINVAL, "athd_pack_spectrum: Ts must be in [1, 2048]");
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    return finish(c, "athd_pack_spectrum", pack_spec_launch(z, B, Ts, spec, (hipStream_t)stream));
}

size_t athd_head_output_workspace_bytes(int64_t B, int64_t T) {
    if (B <= 0 || B > MAX_B || T <= 0 || (T + HOP - 1) / HOP > MAX_TS) return 0;
    return (size_t)istft_ola_part_floats(B, (int)((T + HOP - 1) / HOP)) * sizeof(float);
}

int athd_head_output(athd_ctx* c, const float* logits, const float* spec, const float* xt, const float* tnorm, int64_t B,
                     int64_t T, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    if (int rc = check(c, "athd_head_output", logits && spec && xt && tnorm && out, B)) return rc;
    if (int rc = check_T(c, "athd_head_output", T)) return rc;
    const size_t need = athd_head_output_workspace_bytes(B, T);
    if (!ws || ws_bytes < need)
        return c->fail(ATHD_EWORKSPACE, "athd_head_output: workspace too small: need " + std::to_string(need));
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    // the inference path's launch (forward_dec.cpp) with one prompt per segment: f32 context = the double FFT with the
    // exact mask arithmetic, bf16 context = the fast variant
    istft_ola_launch(logits, (int)B, (int)((T + HOP - 1) / HOP), 1, T, spec, c->tw, c->mode == 1 ? nullptr : c->tw64,
                     c->win, c->win2, xt, tnorm, out, (float*)ws, (hipStream_t)stream);
    return finish(c, "athd_head_output", (int)hipGetLastError());
}

int athd_head_output_backward(athd_ctx* c, const float* grad_out, const float* logits, const float* spec, int64_t B,
                              int64_t T, float* grad_logits, void* stream) {
    if (!c) return ATHD_EINVAL;
    if (int rc = check(c, "athd_head_output_backward", grad_out && logits && spec && grad_logits, B)) return rc;
    if (int rc = check_T(c, "athd_head_output_backward", T)) return rc;
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    return finish(c, "athd_head_output_backward",
                  head_grad_launch(grad_out, logits, spec, B, (int)((T + HOP - 1) / HOP), T, c->tw, c->win, c->win2,
                                   grad_logits, (hipStream_t)stream));
}

}  // extern "C"
