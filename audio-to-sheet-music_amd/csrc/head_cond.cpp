// Head training's text-conditioning stage behind the C ABI (include/athd.h): the forward and its backward with respect
// to the six weight tensors and the per-item attention vector (head_cond.hip).  Each entry checks its arguments,
// enqueues on the caller's stream and returns: no host synchronisation, no HIP object.
#include <string>

#include "../../include/athd.h"
#include "ctx.h"
#include "kernels.h"
#include "prof.h"

namespace {

// the context's state, then the pointers, then the shape
int check(athd_ctx* c, const char* what, bool ptrs_ok, int64_t B, int64_t N) {
    if (!c->finalized) return c->fail(ATHD_ESTATE, std::string(what) + " before athd_finalize");
    if (!ptrs_ok) return c->fail(ATHD_EINVAL, std::string(what) + ": a null pointer");
    if (B <= 0 || B > 65535) return c->fail(ATHD_EINVAL, std::string(what) + ": B must be in [1, 65535]");
    if (N <= 0 || N > athd::HEAD_COND_MAX_N)
        return c->fail(ATHD_EINVAL, std::string(what) + ": N must be in [1, 1048576]");
    return ATHD_OK;
}

// routes the call's launches into the context's profile window (prof.h); nothing while no window is open
struct ProfBind {
    athd::KProf* saved;
    explicit ProfBind(athd::KProf* p) : saved(athd::t_kprof) { athd::t_kprof = p; }
    ~ProfBind() { athd::t_kprof = saved; }
};

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int finish(athd_ctx* c, const char* what, int rc) {
    if (rc == -1) return c->fail(ATHD_EINVAL, std::string(what) + ": bad shape");
    if (rc != 0) return c->fail(ATHD_EHIP, std::string(what) + ": launch failed (code " + std::to_string(rc) + ")");
    return ATHD_OK;
}

}  // namespace

extern "C" {

size_t athd_head_cond_workspace_bytes(int64_t B, int64_t N) {
    return (size_t)athd::head_cond_ws_floats(B, N) * sizeof(float);
}

int athd_head_cond(athd_ctx* c, const float* x, const float* a, const float* w0, const float* b0, const float* w2,
                   const float* b2, const float* gamma, const float* beta, int64_t B, int64_t N, float* y, void* ws,
                   size_t ws_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    const char* what = "athd_head_cond";
    if (int rc = check(c, what, x && a && w0 && b0 && w2 && b2 && gamma && beta && y, B, N)) return rc;
    if (!aligned16(w0) || !aligned16(w2)) return c->fail(ATHD_EINVAL, std::string(what) + ": w0 / w2 not 16-byte aligned");
    (void)ws;                                              // the forward needs no workspace
    (void)ws_bytes;
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    ProfBind prof_bind(c->prof);
    return finish(c, what, athd::head_cond_fwd_launch(x, a, w0, b0, w2, b2, gamma, beta, B, N, y, (hipStream_t)stream));
}

int athd_head_cond_backward(athd_ctx* c, const float* grad_y, const float* x, const float* a, const float* w0,
                            const float* b0, const float* w2, const float* b2, const float* gamma, int64_t B, int64_t N,
                            float* grad_w0, float* grad_b0, float* grad_w2, float* grad_b2, float* grad_gamma,
                            float* grad_beta, float* grad_a, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    const char* what = "athd_head_cond_backward";
    if (int rc = check(c, what,
                       grad_y && x && a && w0 && b0 && w2 && b2 && gamma && grad_w0 && grad_b0 && grad_w2 && grad_b2 &&
                           grad_gamma && grad_beta && grad_a,
                       B, N))
        return rc;
    if (!aligned16(w0) || !aligned16(w2) || !aligned16(grad_w0) || !aligned16(grad_w2))
        return c->fail(ATHD_EINVAL, std::string(what) + ": w0 / w2 / grad_w0 / grad_w2 not 16-byte aligned");
    const size_t need = athd_head_cond_workspace_bytes(B, N);
    if (!ws || ws_bytes < need)
        return c->fail(ATHD_EWORKSPACE, std::string(what) + ": workspace too small: need " + std::to_string(need));
    if (!aligned16(ws)) return c->fail(ATHD_EINVAL, std::string(what) + ": workspace not 16-byte aligned");
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    ProfBind prof_bind(c->prof);
    return finish(c, what,
                  athd::head_cond_bwd_launch(grad_y, x, a, w0, b0, w2, b2, gamma, B, N, grad_w0, grad_b0, grad_w2,
                                             grad_b2, grad_gamma, grad_beta, grad_a, (float*)ws, (hipStream_t)stream));
}

}  // extern "C"
