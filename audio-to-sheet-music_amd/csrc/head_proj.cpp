// Head training's output projections and attention vector behind the C ABI (include/athd.h): freq_out / time_out in the
// output stage's layouts with their backward, and out_proj(in_proj_v(v_proj(text))) with its backward (head_proj.hip).
// Each entry checks its arguments, enqueues on the caller's stream and returns: no host synchronisation, no HIP object.
#include <string>

#include "../../include/athd.h"
#include "ctx.h"
#include "kernels.h"
#include "prof.h"

namespace {

// routes the call's launches into the context's profile window (prof.h); nothing while no window is open
struct ProfBind {
    athd::KProf* saved;
    explicit ProfBind(athd::KProf* p) : saved(athd::t_kprof) { athd::t_kprof = p; }
    ~ProfBind() { athd::t_kprof = saved; }
};

bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// the context's state, then the pointers, then the shape, then the alignment
int check_proj(athd_ctx* c, const char* what, bool ptrs_ok, bool big_aligned, bool small_aligned, int64_t B, int64_t R,
               int64_t S) {
    if (!c->finalized) return c->fail(ATHD_ESTATE, std::string(what) + " before athd_finalize");
    if (!ptrs_ok) return c->fail(ATHD_EINVAL, std::string(what) + ": a null pointer");
    if (B <= 0 || B > 65535) return c->fail(ATHD_EINVAL, std::string(what) + ": B must be in [1, 65535]");
    if (R <= 0 || R > athd::HEAD_PROJ_MAX_R) return c->fail(ATHD_EINVAL, std::string(what) + ": R must be in [1, 4096]");
    if (S <= 0 || S > athd::HEAD_PROJ_MAX_S)
        return c->fail(ATHD_EINVAL, std::string(what) + ": S must be in [1, 4194304]");
    if (R * S > athd::HEAD_PROJ_MAX_RS) return c->fail(ATHD_EINVAL, std::string(what) + ": R S must be at most 4194304");
    if (!big_aligned) return c->fail(ATHD_EINVAL, std::string(what) + ": x, y, grad_y or grad_x not 16-byte aligned");
    if (!small_aligned) return c->fail(ATHD_EINVAL, std::string(what) + ": a parameter pointer not 4-byte aligned");
    return ATHD_OK;
}

int check_attn(athd_ctx* c, const char* what, bool ptrs_ok, bool ptrs_aligned, int64_t B, int64_t max_b) {
    if (!c->finalized) return c->fail(ATHD_ESTATE, std::string(what) + " before athd_finalize");
    if (!ptrs_ok) return c->fail(ATHD_EINVAL, std::string(what) + ": a null pointer");
    if (B <= 0 || B > max_b)
        return c->fail(ATHD_EINVAL, std::string(what) + ": B must be in [1, " + std::to_string(max_b) + "]");
    if (!ptrs_aligned) return c->fail(ATHD_EINVAL, std::string(what) + ": a pointer not 4-byte aligned");
    return ATHD_OK;
}

int finish(athd_ctx* c, const char* what, int rc) {
    if (rc == -1) return c->fail(ATHD_EINVAL, std::string(what) + ": bad shape");
    if (rc != 0) return c->fail(ATHD_EHIP, std::string(what) + ": launch failed (code " + std::to_string(rc) + ")");
    return ATHD_OK;
}

}  // namespace

extern "C" {

size_t athd_head_proj_workspace_bytes(int64_t B, int64_t R, int64_t S) {
    return (size_t)athd::head_proj_ws_doubles(B, R, S) * sizeof(double);
}

int athd_head_proj(athd_ctx* c, const float* x, const float* w, const float* bias, int64_t B, int64_t R, int64_t S,
                   float* y, void* stream) {
    if (!c) return ATHD_EINVAL;
    const char* what = "athd_head_proj";
    if (int rc = check_proj(c, what, x && w && bias && y, aligned(x, 16) && aligned(y, 16),
                            aligned(w, 4) && aligned(bias, 4), B, R, S))
        return rc;
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    ProfBind prof_bind(c->prof);
    return finish(c, what, athd::head_proj_fwd_launch(x, w, bias, B, R, S, y, (hipStream_t)stream));
}

int athd_head_proj_backward(athd_ctx* c, const float* grad_y, int grad_channel_first, const float* scale,
                            const float* x, const float* w, int64_t B, int64_t R, int64_t S, float* grad_x,
                            float* grad_w, float* grad_b, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    const char* what = "athd_head_proj_backward";
    if (int rc = check_proj(c, what, grad_y && x && w && grad_x && grad_w && grad_b,
                            aligned(grad_y, 16) && aligned(x, 16) && aligned(grad_x, 16),
                            aligned(scale, 4) && aligned(w, 4) && aligned(grad_w, 4) && aligned(grad_b, 4), B, R, S))
        return rc;
    const size_t need = athd_head_proj_workspace_bytes(B, R, S);
    if (!ws || ws_bytes < need)
        return c->fail(ATHD_EWORKSPACE, std::string(what) + ": workspace too small: need " + std::to_string(need));
    if (!aligned(ws, 16)) return c->fail(ATHD_EINVAL, std::string(what) + ": workspace not 16-byte aligned");
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    ProfBind prof_bind(c->prof);
    return finish(c, what,
                  athd::head_proj_bwd_launch(grad_y, grad_channel_first != 0, scale, x, w, B, R, S, grad_x, grad_w, grad_b,
                                             (double*)ws, (hipStream_t)stream));
}

int athd_head_attn_vec(athd_ctx* c, const float* text, const float* wv, const float* bv, const float* w_in,
                       const float* b_in, const float* wo, const float* bo, int64_t B, float* a, float* keep,
                       void* stream) {
    if (!c) return ATHD_EINVAL;
    const char* what = "athd_head_attn_vec";
    if (int rc = check_attn(c, what, text && wv && bv && w_in && b_in && wo && bo && a && keep,
                            aligned(text, 4) && aligned(wv, 4) && aligned(bv, 4) && aligned(w_in, 4) && aligned(b_in, 4) &&
                                aligned(wo, 4) && aligned(bo, 4) && aligned(a, 4) && aligned(keep, 4),
                            B, 65535))
        return rc;
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    ProfBind prof_bind(c->prof);
    return finish(c, what,
                  athd::head_attn_vec_fwd_launch(text, wv, bv, w_in, b_in, wo, bo, B, a, keep, (hipStream_t)stream));
}

int athd_head_attn_vec_backward(athd_ctx* c, const float* grad_a, const float* text, const float* keep,
                                const float* w_in, const float* wo, int64_t B, float* grad_wv, float* grad_bv,
                                float* grad_w_in, float* grad_b_in, float* grad_wo, float* grad_bo, void* stream) {
    if (!c) return ATHD_EINVAL;
    const char* what = "athd_head_attn_vec_backward";
    if (int rc = check_attn(c, what,
                            grad_a && text && keep && w_in && wo && grad_wv && grad_bv && grad_w_in && grad_b_in &&
                                grad_wo && grad_bo,
                            aligned(grad_a, 4) && aligned(text, 4) && aligned(keep, 4) && aligned(w_in, 4) &&
                                aligned(wo, 4) && aligned(grad_wv, 4) && aligned(grad_bv, 4) && aligned(grad_w_in, 4) &&
                                aligned(grad_b_in, 4) && aligned(grad_wo, 4) && aligned(grad_bo, 4),
                            B, athd::HEAD_ATTN_MAX_B))
        return rc;
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    ProfBind prof_bind(c->prof);
    return finish(c, what,
                  athd::head_attn_vec_bwd_launch(grad_a, text, keep, w_in, wo, B, grad_wv, grad_bv, grad_w_in, grad_b_in,
                                                 grad_wo, grad_bo, (hipStream_t)stream));
}

}  // extern "C"
