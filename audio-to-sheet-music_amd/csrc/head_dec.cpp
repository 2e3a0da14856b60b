// Head training's decoder level behind the C ABI (include/athd.h): the forward and its backward with respect to the
// level's input and its parameters (head_dec.hip).  Each entry checks its arguments, enqueues on the caller's stream and
// returns: no host synchronisation, no HIP object.
#include <string>

#include "../../include/athd.h"
#include "ctx.h"
#include "kernels.h"
#include "prof.h"

namespace {

// the context's state, then the pointers, then the level and the shape
int check(athd_ctx* c, const char* what, bool ptrs_ok, bool norm_ptrs_ok, int level, int64_t B, int64_t M, int64_t inner,
          int64_t Lt) {
    if (!c->finalized) return c->fail(ATHD_ESTATE, std::string(what) + " before athd_finalize");
    if (!ptrs_ok || (level >= 0 && level < 3 && !norm_ptrs_ok))
        return c->fail(ATHD_EINVAL, std::string(what) + ": a null pointer");
    if (level < 0 || level > 3) return c->fail(ATHD_EINVAL, std::string(what) + ": level must be in [0, 3]");
    if (B <= 0 || B > 65535) return c->fail(ATHD_EINVAL, std::string(what) + ": B must be in [1, 65535]");
    if (M <= 0 || M > athd::HEAD_DEC_MAX_M || inner <= 0 || inner > athd::HEAD_DEC_MAX_INNER || Lt <= 0 ||
        Lt > athd::HEAD_DEC_MAX_LT || M * inner > athd::HEAD_DEC_MAX_TOKENS || Lt * inner > 4 * athd::HEAD_DEC_MAX_TOKENS)
        return c->fail(ATHD_EINVAL, std::string(what) + ": M in [1, 1048576], inner in [1, 4096], Lt in [1, 4194304], "
                                                        "M inner <= 67108864 and Lt inner <= 268435456");
    return ATHD_OK;
}

// routes the call's launches into the context's profile window (prof.h); nothing while no window is open
struct ProfBind {
    athd::KProf* saved;
    explicit ProfBind(athd::KProf* p) : saved(athd::t_kprof) { athd::t_kprof = p; }
    ~ProfBind() { athd::t_kprof = saved; }
};

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the weight's alignment, then the workspace: present and large enough, then aligned
int check_ws(athd_ctx* c, const char* what, const float* w, const float* gw, int level, int64_t B, int64_t M,
             int64_t inner, int64_t Lt, const void* ws, size_t ws_bytes) {
    if (!aligned16(w) || !aligned16(gw))
        return c->fail(ATHD_EINVAL, std::string(what) + ": weight (or its gradient) not 16-byte aligned");
    if (ws && !aligned16(ws)) return c->fail(ATHD_EINVAL, std::string(what) + ": workspace not 16-byte aligned");
    const size_t need = athd_head_dec_workspace_bytes(level, B, M, inner, Lt);
    if (!ws || ws_bytes < need)
        return c->fail(ATHD_EWORKSPACE, std::string(what) + ": workspace too small: need " + std::to_string(need));
    return ATHD_OK;
}

int finish(athd_ctx* c, const char* what, int rc) {
    if (rc == -1) return c->fail(ATHD_EINVAL, std::string(what) + ": bad shape");
    if (rc != 0) return c->fail(ATHD_EHIP, std::string(what) + ": launch failed (code " + std::to_string(rc) + ")");
    return ATHD_OK;
}

}  // namespace

extern "C" {

size_t athd_head_dec_workspace_bytes(int level, int64_t B, int64_t M, int64_t inner, int64_t Lt) {
    return (size_t)athd::head_dec_ws_floats(level, B, M, inner, Lt) * sizeof(float);
}

int athd_head_dec_level(athd_ctx* c, int level, const float* x, const float* w, const float* bias, const float* gamma,
                        const float* beta, const float* skip, int64_t B, int64_t M, int64_t inner, int64_t S, int64_t Lt,
                        float* y, float* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    const char* what = "athd_head_dec_level";
    if (int rc = check(c, what, x && w && bias && y, gamma && beta && stats, level, B, M, inner, Lt)) return rc;
    if ((skip == nullptr) != (S == 0) || S < 0 || S > athd::HEAD_DEC_MAX_LT || S * inner > 4 * athd::HEAD_DEC_MAX_TOKENS)
        return c->fail(ATHD_EINVAL, std::string(what) + ": skip and S go together (NULL with 0), S in [0, 4194304] and "
                                                        "S inner <= 268435456");
    if (int rc = check_ws(c, what, w, nullptr, level, B, M, inner, Lt, ws, ws_bytes)) return rc;
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    ProfBind prof_bind(c->prof);
    return finish(c, what,
                  athd::head_dec_fwd_launch(level, x, w, bias, gamma, beta, skip, B, M, inner, S, Lt, y, stats,
                                            (float*)ws, (hipStream_t)stream));
}

int athd_head_dec_level_backward(athd_ctx* c, int level, const float* grad_y, const float* x, const float* w,
                                 const float* bias, const float* gamma, const float* beta, const float* stats, int64_t B,
                                 int64_t M, int64_t inner, int64_t Lt, float* grad_x, float* grad_w, float* grad_bias,
                                 float* grad_gamma, float* grad_beta, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    const char* what = "athd_head_dec_level_backward";
    if (int rc = check(c, what, grad_y && x && w && bias && grad_x && grad_w && grad_bias,
                       gamma && beta && stats && grad_gamma && grad_beta, level, B, M, inner, Lt))
        return rc;
    if (int rc = check_ws(c, what, w, grad_w, level, B, M, inner, Lt, ws, ws_bytes)) return rc;
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    ProfBind prof_bind(c->prof);
    return finish(c, what,
                  athd::head_dec_bwd_launch(level, grad_y, x, w, bias, gamma, beta, stats, B, M, inner, Lt, grad_x,
                                            grad_w, grad_bias, grad_gamma, grad_beta, (float*)ws, (hipStream_t)stream));
}

}  // extern "C"
