// Head training's update step behind the C ABI (include/athd.h): the fused clip + AdamW launches of head_step.hip.
// There is no context: the entry checks its arguments, enqueues on the caller's stream and returns; no host
// synchronisation, no allocation, no HIP object.
#include "../../include/athd.h"
#include "kernels.h"

extern "C" {

size_t athd_head_step_workspace_bytes(const athd_step_tensor* t, int n_tensors) {
    return (size_t)athd::head_step_chunks(t, n_tensors) * sizeof(double);
}

int athd_head_step(const athd_step_tensor* t, int n_tensors, const athd_step_hparams* hp, const float* grad_scale,
                   const float* found_inf, int32_t* step, float* stats, void* workspace, size_t workspace_bytes,
                   void* stream) {
    if (!t || !hp) return ATHD_EINVAL;
    const size_t need = athd_head_step_workspace_bytes(t, n_tensors);
    if (need == 0) return ATHD_EINVAL;                     // n_tensors outside 1..64, an n < 1, or too many chunks
    if (!workspace || workspace_bytes < need) return ATHD_EWORKSPACE;
    const int rc = athd::head_step_launch(t, n_tensors, *hp, grad_scale, found_inf, step, stats, (double*)workspace,
                                          (hipStream_t)stream);
    return rc == 0 ? ATHD_OK : rc == -1 ? ATHD_EINVAL : ATHD_EHIP;
}

}  // extern "C"
