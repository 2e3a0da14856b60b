// Head training's update step (include/athd.h `athd_head_step`): the global gradient norm, clip_grad_norm_'s coefficient,
// the AMP scaler's unscale and skip, and torch.optim.AdamW's update for up to 64 tensors, in three launches.
//
// A pure streaming pass: 4 bytes per element read by the norm launch, 16 read and 12 written by the update launch.  A
// tensor is cut into chunks of HEAD_STEP_CHUNK = 4096 elements (the last one shorter) and one workgroup of 256 threads
// takes one chunk, so a chunk never straddles two tensors.  The tensor table (64 x 40 bytes) and the per-tensor
// chunk-count prefix (65 ints) travel by value in the kernel arguments: nothing is uploaded, and the pointers may change
// from call to call.  Thread t of a chunk takes the groups of four elements t, t + 256, t + 512, t + 768; a whole group
// is one 16-byte access when the tensor's four pointers are 16-byte aligned and four 4-byte ones otherwise, a group cut
// by the tensor's end goes element by element.  The element -> thread map does not depend on the alignment, so neither do
// the sums.
//
//   1. head_step_norm_kernel    part[chunk] = sum g^2 in fp64: per thread in ascending element order, the wave by
//                               shuffles, the four waves in ascending order (as loss.hip's block_store)
//   2. head_step_update_kernel  every workgroup stages the partials in LDS and its thread 0 adds them in index order
//                               (sum_partials: the same code, hence the same bits, in every workgroup and in the
//                               tail), derives norm, coef, the skip flag and the step's scalars in fp64 and hands them
//                               over in LDS while the chunk's loads are in flight; then per element, in fp64, rounded
//                               once per stored value
//   3. head_step_tail_kernel    one workgroup, one writing thread: the same scalars again, then stats and the counter.
//                               No workgroup of launch 2 reads a word that launch 2 writes: the counter is only read
//                               there.
// No atomics anywhere: the same bits on every run and under graph replay.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace athd {

constexpr int HS_THREADS = 256;
constexpr int HS_GROUPS = HEAD_STEP_CHUNK / 4 / HS_THREADS;      // groups of four elements per thread and chunk

struct StepTable {
    athd_step_tensor t[ATHD_STEP_MAX_TENSORS];
};
struct StepChunks {
    int first[ATHD_STEP_MAX_TENSORS + 1];      // first[i] = chunks of the tensors before i; first[n_tensors] = all
};

// the tensor that owns chunk `c` (wave-uniform: the prefix sits in the kernel arguments)
ATHD_DEV int chunk_tensor(const StepChunks& ch, int n_tensors, int c) {
    int ti = 0;
    while (ti + 1 < n_tensors && ch.first[ti + 1] <= c) ++ti;
    return ti;
}

ATHD_DEV bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// one thread's elements of a chunk of `len` elements from `p`: whole groups by load4, a cut group per element
ATHD_DEV void load_chunk(const float* __restrict__ p, int64_t len, bool vec, float (&x)[HS_GROUPS][4]) {
#pragma unroll
    for (int j = 0; j < HS_GROUPS; ++j) {
        const int64_t e0 = 4 * ((int64_t)threadIdx.x + HS_THREADS * j);
        if (e0 + 4 <= len) {
            if (vec) {
                const float4 q = *reinterpret_cast<const float4*>(p + e0);
                x[j][0] = q.x; x[j][1] = q.y; x[j][2] = q.z; x[j][3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) x[j][k] = p[e0 + k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) x[j][k] = e0 + k < len ? p[e0 + k] : 0.f;
        }
    }
}

ATHD_DEV void store_chunk(float* __restrict__ p, int64_t len, bool vec, const float (&x)[HS_GROUPS][4]) {
#pragma unroll
    for (int j = 0; j < HS_GROUPS; ++j) {
        const int64_t e0 = 4 * ((int64_t)threadIdx.x + HS_THREADS * j);
        if (e0 + 4 <= len) {
            if (vec) {
                *reinterpret_cast<float4*>(p + e0) = make_float4(x[j][0], x[j][1], x[j][2], x[j][3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) p[e0 + k] = x[j][k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < len) p[e0 + k] = x[j][k];
        }
    }
}

// grid: one workgroup per chunk.  Elements past the tensor's end are read as 0 and add nothing.
__global__ __launch_bounds__(HS_THREADS) void head_step_norm_kernel(StepTable tab, StepChunks ch, int n_tensors,
                                                                    double* __restrict__ part) {
    const int c = (int)blockIdx.x;
    const int ti = chunk_tensor(ch, n_tensors, c);
    const int64_t base = (int64_t)(c - ch.first[ti]) * HEAD_STEP_CHUNK;
    const int64_t n = tab.t[ti].n;
    const float* g = tab.t[ti].grad;
    const bool vec = aligned16(tab.t[ti].param) && aligned16(g) && aligned16(tab.t[ti].exp_avg) &&
                     aligned16(tab.t[ti].exp_avg_sq);
    const int64_t len = n - base < HEAD_STEP_CHUNK ? n - base : HEAD_STEP_CHUNK;
    float x[HS_GROUPS][4];
    load_chunk(g + base, len, vec, x);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < HS_GROUPS; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)x[j][k] * (double)x[j][k];
    __shared__ double sh[HS_THREADS / 64];
    const double w = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) part[c] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// What one step needs besides the elements, from the partial sums, the hyper-parameters and the counter.
struct StepScalars {
    double norm, coef;      // the unscaled gradients' global norm; clip_grad_norm_'s clamped coefficient
    double inv;             // 1 / *grad_scale
    double decay;           // 1 - lr wd
    double omb1, omb2;      // 1 - beta1, 1 - beta2
    double step_size;       // lr / (1 - beta1^t)
    double rsqrt_bc2;       // 1 / sqrt(1 - beta2^t)
    int skipped, t;         // t = the counter after this call
};

// The sum of the partials, in index order, valid in thread 0.  The whole workgroup copies them into LDS with coalesced
// loads (n_chunks <= HEAD_STEP_MAX_CHUNKS doubles, 32 KiB), then thread 0 adds them one after the other: the order, and
// with it the bits, are those of a plain loop over the array, in every workgroup and in the tail, but the chain of
// additions waits on LDS reads that pipeline, not on one global load per term.
ATHD_DEV double sum_partials(const double* __restrict__ part, int n_chunks, double* sp) {
    for (int i = threadIdx.x; i < n_chunks; i += blockDim.x) sp[i] = part[i];
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < n_chunks; ++i) total += sp[i];
    return total;
}

// One thread's work, from the sum of the partials.
ATHD_DEV StepScalars step_scalars(const athd_step_hparams& hp, const float* grad_scale, const float* found_inf,
                                  const int32_t* step, double total) {
    StepScalars s;
    s.inv = grad_scale ? 1.0 / (double)*grad_scale : 1.0;
    s.norm = sqrt(total) * s.inv;
    s.coef = hp.max_norm > 0.0 ? fmin(1.0, hp.max_norm / (s.norm + 1e-6)) : 1.0;
    s.skipped = (found_inf && *found_inf != 0.f) || !isfinite(s.norm);
    const int t0 = *step;
    s.t = s.skipped ? t0 : t0 + 1;
    s.decay = 1.0 - hp.lr * hp.weight_decay;
    s.omb1 = 1.0 - hp.beta1;
    s.omb2 = 1.0 - hp.beta2;
    s.step_size = hp.lr / (1.0 - pow(hp.beta1, (double)s.t));
    s.rsqrt_bc2 = 1.0 / sqrt(1.0 - pow(hp.beta2, (double)s.t));
    return s;
}

// grid: one workgroup per chunk.  torch.optim.AdamW's order: decay, moments, bias-corrected update.
__global__ __launch_bounds__(HS_THREADS) void head_step_update_kernel(StepTable tab, StepChunks ch, int n_tensors,
                                                                      athd_step_hparams hp,
                                                                      const float* __restrict__ grad_scale,
                                                                      const float* __restrict__ found_inf,
                                                                      const int32_t* __restrict__ step,
                                                                      const double* __restrict__ part) {
    const int c = (int)blockIdx.x;
    const int ti = chunk_tensor(ch, n_tensors, c);
    const int64_t base = (int64_t)(c - ch.first[ti]) * HEAD_STEP_CHUNK;
    const int64_t n = tab.t[ti].n;
    float* p = tab.t[ti].param + base;
    const float* g = tab.t[ti].grad + base;
    float* m = tab.t[ti].exp_avg + base;
    float* v = tab.t[ti].exp_avg_sq + base;
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);      // base keeps the alignment
    const int64_t len = n - base < HEAD_STEP_CHUNK ? n - base : HEAD_STEP_CHUNK;
    float pv[HS_GROUPS][4], gv[HS_GROUPS][4], mv[HS_GROUPS][4], vv[HS_GROUPS][4];
    load_chunk(p, len, vec, pv);
    load_chunk(g, len, vec, gv);
    load_chunk(m, len, vec, mv);
    load_chunk(v, len, vec, vv);
    __shared__ StepScalars sh;
    __shared__ double sp[HEAD_STEP_MAX_CHUNKS];
    const double total = sum_partials(part, ch.first[n_tensors], sp);
    if (threadIdx.x == 0) sh = step_scalars(hp, grad_scale, found_inf, step, total);
    __syncthreads();
    const StepScalars s = sh;
    if (s.skipped) return;                                   // nothing is written to any parameter or moment
#pragma unroll
    for (int j = 0; j < HS_GROUPS; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double gr = ((double)gv[j][k] * s.inv) * s.coef;
            const double pd = (double)pv[j][k] * s.decay;
            const double md = hp.beta1 * (double)mv[j][k] + s.omb1 * gr;
            const double vd = hp.beta2 * (double)vv[j][k] + s.omb2 * (gr * gr);
            pv[j][k] = (float)(pd - s.step_size * md / (sqrt(vd) * s.rsqrt_bc2 + hp.eps));
            mv[j][k] = (float)md;
            vv[j][k] = (float)vd;
        }
    store_chunk(p, len, vec, pv);
    store_chunk(m, len, vec, mv);
    store_chunk(v, len, vec, vv);
}

// one workgroup, one writing thread: stats = {norm, coef, skipped, the counter after this call} and the counter itself
__global__ __launch_bounds__(HS_THREADS) void head_step_tail_kernel(athd_step_hparams hp, const float* __restrict__ grad_scale,
                                                            const float* __restrict__ found_inf, int32_t* step,
                                                            const double* __restrict__ part, int n_chunks,
                                                            float* __restrict__ stats) {
    __shared__ double sp[HEAD_STEP_MAX_CHUNKS];
    const double total = sum_partials(part, n_chunks, sp);
    if (threadIdx.x != 0) return;
    const StepScalars s = step_scalars(hp, grad_scale, found_inf, step, total);
    stats[0] = (float)s.norm;
    stats[1] = (float)s.coef;
    stats[2] = s.skipped ? 1.f : 0.f;
    stats[3] = (float)s.t;
    *step = s.t;
}

int64_t head_step_chunks(const athd_step_tensor* t, int n_tensors) {
    if (!t || n_tensors < 1 || n_tensors > ATHD_STEP_MAX_TENSORS) return 0;
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (t[i].n < 1 || t[i].n > HEAD_STEP_MAX_CHUNKS * HEAD_STEP_CHUNK) return 0;
        chunks += (t[i].n + HEAD_STEP_CHUNK - 1) / HEAD_STEP_CHUNK;
    }
    return chunks <= HEAD_STEP_MAX_CHUNKS ? chunks : 0;
}

int head_step_launch(const athd_step_tensor* t, int n_tensors, const athd_step_hparams& hp, const float* grad_scale,
                     const float* found_inf, int32_t* step, float* stats, double* part, hipStream_t s) {
    const int64_t chunks = head_step_chunks(t, n_tensors);
    if (chunks == 0 || !step || !stats || !part) return -1;
    if (((uintptr_t)grad_scale & 3) || ((uintptr_t)found_inf & 3) || ((uintptr_t)step & 3) || ((uintptr_t)stats & 3) ||
        ((uintptr_t)part & 7))
        return -1;
    StepTable tab = {};
    StepChunks ch = {};
    for (int i = 0; i < n_tensors; ++i) {
        const athd_step_tensor& e = t[i];
        if (!e.param || !e.grad || !e.exp_avg || !e.exp_avg_sq) return -1;
        if (((uintptr_t)e.param & 3) || ((uintptr_t)e.grad & 3) || ((uintptr_t)e.exp_avg & 3) ||
            ((uintptr_t)e.exp_avg_sq & 3))
            return -1;
        tab.t[i] = e;
        ch.first[i + 1] = ch.first[i] + (int)((e.n + HEAD_STEP_CHUNK - 1) / HEAD_STEP_CHUNK);
    }
    for (int i = n_tensors; i < ATHD_STEP_MAX_TENSORS; ++i) ch.first[i + 1] = ch.first[n_tensors];
    hipLaunchKernelGGL(head_step_norm_kernel, dim3((unsigned)chunks), dim3(HS_THREADS), 0, s, tab, ch, n_tensors, part);
    hipLaunchKernelGGL(head_step_update_kernel, dim3((unsigned)chunks), dim3(HS_THREADS), 0, s, tab, ch, n_tensors, hp,
                       grad_scale, found_inf, (const int32_t*)step, (const double*)part);
    hipLaunchKernelGGL(head_step_tail_kernel, dim3(1), dim3(HS_THREADS), 0, s, hp, grad_scale, found_inf, step,
                       (const double*)part, (int)chunks, stats);
    return (int)hipGetLastError();
}

}  // namespace athd
