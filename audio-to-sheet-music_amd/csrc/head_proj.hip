// Head training's output projections and attention vector (include/athd.h `athd_head_proj*`, `athd_head_attn_vec*`), all
// f32 storage.
//
// The projection is `freq_out` / `time_out`: a 1x1 convolution from 4 to 2 channels between the last decoder level's
// channel-first x (B, 4, R, S) and the output stage's position-major y (B, S, R, 2).  It is a pure streaming pass (24
// bytes per position forward, 40 backward), so the only question is the layout:
//   * R == 1 (the time branch), and every backward whose gradient is channel-first: position p of item b is element p of
//     each channel row, nothing is transposed.  A workgroup of 256 threads takes a chunk of HEAD_PROJ_CHUNK = 4096
//     positions; thread t takes the groups of four positions t, t + 256, t + 512, t + 768, each one 16-byte access per
//     row when R S is a multiple of 4 and four 4-byte ones otherwise (the element -> thread map is the same, so are the
//     sums).
//   * R > 1 with y's layout: a 32 x 32 tile of (r, s) goes through LDS with pitch 33 (export_spec_kernel's pattern), so
//     that the reads and writes along s (x, grad_x) and along (r, o) (y, grad_y) are both coalesced.
// The backward's ten sums (grad_w, grad_b): per thread in double in ascending position order, the wave by shuffles, the
// four waves in ascending order, one partial of ten doubles per workgroup; proj_tail_kernel (one workgroup) adds the
// partials in index order and rounds once.  No atomics anywhere: the same bits on every run and under graph replay.
//
// The attention vector is three matrix-vector products per item and their gradients, a few MFLOP: every output element
// belongs to one wave (forward) or one thread (backward), which sums in double in ascending index order.
#include "common.h"
#include "kernels.h"

namespace athd {

constexpr int PJ_THREADS = 256;
constexpr int PJ_GROUPS = HEAD_PROJ_CHUNK / 4 / PJ_THREADS;
constexpr int PJ_T = 32;                                   // tile edge

struct ProjW {
    float w[2][4];
    float b[2];
};

ATHD_DEV ProjW load_w(const float* __restrict__ w, const float* __restrict__ bias) {
    ProjW p;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
#pragma unroll
        for (int c = 0; c < 4; ++c) p.w[o][c] = w[o * 4 + c];
        p.b[o] = bias ? bias[o] : 0.f;
    }
    return p;
}

ATHD_DEV float proj_y(const ProjW& p, int o, const float (&x)[4]) {
    return fmaf(p.w[o][3], x[3], fmaf(p.w[o][2], x[2], fmaf(p.w[o][1], x[1], fmaf(p.w[o][0], x[0], p.b[o]))));
}

// four consecutive elements from p + e, `len` of them valid (the rest read as 0)
ATHD_DEV void load4(const float* __restrict__ p, int64_t len, bool vec, float (&v)[4]) {
    if (len >= 4 && vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < len ? p[k] : 0.f;
    }
}

ATHD_DEV void store4(float* __restrict__ p, int64_t len, bool vec, const float (&v)[4]) {
    if (len >= 4 && vec) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < len) p[k] = v[k];
    }
}

// the workgroup's ten sums -> part[10 wg ..]
ATHD_DEV void block_partials(const double (&acc)[10], double* __restrict__ part, int64_t wg) {
    __shared__ double sh[PJ_THREADS / 64][10];
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const double w = wave_sum_d(acc[j]);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][j] = w;
    }
    __syncthreads();
    if (threadIdx.x < 10) part[wg * 10 + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) +
                                                         sh[3][threadIdx.x];
}

// ------------------------------------------------------------------------------------------------------- forward
// One kernel for both branches.  R == 1: grid (chunks, B), the straight stream; R > 1: grid (ceil(S / 32), ceil(R / 32),
// B), the transpose through LDS.
__global__ __launch_bounds__(PJ_THREADS) void head_proj_fwd_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ w,
                                                                   const float* __restrict__ bias, int64_t R, int64_t S,
                                                                   float* __restrict__ y) {
    const ProjW p = load_w(w, bias);
    if (R == 1) {
        const int64_t b = blockIdx.y;
        const bool vec = (S & 3) == 0;
        const float* xb = x + b * 4 * S;
        float* yb = y + b * S * 2;
#pragma unroll
        for (int j = 0; j < PJ_GROUPS; ++j) {
            const int64_t e = (int64_t)blockIdx.x * HEAD_PROJ_CHUNK + 4 * ((int64_t)threadIdx.x + PJ_THREADS * j);
            const int64_t len = S - e;
            if (len <= 0) continue;
            float xv[4][4], y0[4], y1[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) load4(xb + c * S + e, len, vec, xv[c]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xs[4] = {xv[0][k], xv[1][k], xv[2][k], xv[3][k]};
                const float a0 = proj_y(p, 0, xs), a1 = proj_y(p, 1, xs);
                // positions k = 0, 1 fill y0, positions 2, 3 fill y1: (o interleaved)
                if (k < 2) { y0[2 * k] = a0; y0[2 * k + 1] = a1; } else { y1[2 * k - 4] = a0; y1[2 * k - 3] = a1; }
            }
            store4(yb + 2 * e, 2 * len, vec, y0);
            store4(yb + 2 * e + 4, 2 * len - 4, vec, y1);
        }
        return;
    }
    __shared__ float2 tile[PJ_T][PJ_T + 1];                      // [s][r]
    const int64_t b = blockIdx.z;
    const int64_t s0 = (int64_t)blockIdx.x * PJ_T, r0 = (int64_t)blockIdx.y * PJ_T;
    for (int i = threadIdx.x; i < PJ_T * PJ_T; i += PJ_THREADS) {
        const int s = i & (PJ_T - 1), r = i >> 5;
        if (s0 + s < S && r0 + r < R) {
            float xs[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) xs[c] = x[((b * 4 + c) * R + r0 + r) * S + s0 + s];
            tile[s][r] = make_float2(proj_y(p, 0, xs), proj_y(p, 1, xs));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PJ_T * PJ_T; i += PJ_THREADS) {
        const int r = i & (PJ_T - 1), s = i >> 5;
        if (s0 + s < S && r0 + r < R)
            *reinterpret_cast<float2*>(y + ((b * S + s0 + s) * R + r0 + r) * 2) = tile[s][r];
    }
}

// ------------------------------------------------------------------------------------------------------ backward
ATHD_DEV void proj_accumulate(double (&acc)[10], float g0, float g1, const float (&xs)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        acc[c] += (double)g0 * (double)xs[c];
        acc[4 + c] += (double)g1 * (double)xs[c];
    }
    acc[8] += (double)g0;
    acc[9] += (double)g1;
}

// The stream: n = R S positions per item, x and grad_x (B, 4, n); grad_y planar (B, 2, n) or interleaved (B, n, 2).
// grid (chunks, B).
template <bool PLANAR>
__global__ __launch_bounds__(PJ_THREADS) void head_proj_bwd_stream_kernel(const float* __restrict__ gy,
                                                                          const float* __restrict__ scale,
                                                                          const float* __restrict__ x,
                                                                          const float* __restrict__ w, int64_t n,
                                                                          float* __restrict__ gx,
                                                                          double* __restrict__ part) {
    const ProjW p = load_w(w, nullptr);
    const int64_t b = blockIdx.y;
    const bool vec = (n & 3) == 0;
    const float sc = scale ? scale[b] : 1.f;
    const float* xb = x + b * 4 * n;
    const float* gb = gy + b * 2 * n;
    float* gxb = gx + b * 4 * n;
    double acc[10] = {};
#pragma unroll
    for (int j = 0; j < PJ_GROUPS; ++j) {
        const int64_t e = (int64_t)blockIdx.x * HEAD_PROJ_CHUNK + 4 * ((int64_t)threadIdx.x + PJ_THREADS * j);
        const int64_t len = n - e;
        if (len <= 0) continue;
        float xv[4][4], g0[4], g1[4], out[4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) load4(xb + c * n + e, len, vec, xv[c]);
        if (PLANAR) {
            load4(gb + e, len, vec, g0);
            load4(gb + n + e, len, vec, g1);
        } else {
            float a[4], c2[4];
            load4(gb + 2 * e, 2 * len, vec, a);
            load4(gb + 2 * e + 4, 2 * len - 4, vec, c2);
            g0[0] = a[0]; g1[0] = a[1]; g0[1] = a[2]; g1[1] = a[3];
            g0[2] = c2[0]; g1[2] = c2[1]; g0[3] = c2[2]; g1[3] = c2[3];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float h0 = scale ? g0[k] * sc : g0[k], h1 = scale ? g1[k] * sc : g1[k];
            const float xs[4] = {xv[0][k], xv[1][k], xv[2][k], xv[3][k]};
            proj_accumulate(acc, h0, h1, xs);
#pragma unroll
            for (int c = 0; c < 4; ++c) out[c][k] = fmaf(p.w[1][c], h1, p.w[0][c] * h0);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) store4(gxb + c * n + e, len, vec, out[c]);
    }
    block_partials(acc, part, (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// R > 1 with grad_y in y's layout (B, S, R, 2): grid (ceil(S / 32), ceil(R / 32), B)
__global__ __launch_bounds__(PJ_THREADS) void head_proj_bwd_tile_kernel(const float* __restrict__ gy,
                                                                        const float* __restrict__ scale,
                                                                        const float* __restrict__ x,
                                                                        const float* __restrict__ w, int64_t R, int64_t S,
                                                                        float* __restrict__ gx,
                                                                        double* __restrict__ part) {
    __shared__ float2 tile[PJ_T][PJ_T + 1];                      // [s][r]
    const ProjW p = load_w(w, nullptr);
    const int64_t b = blockIdx.z;
    const int64_t s0 = (int64_t)blockIdx.x * PJ_T, r0 = (int64_t)blockIdx.y * PJ_T;
    const float sc = scale ? scale[b] : 1.f;
    for (int i = threadIdx.x; i < PJ_T * PJ_T; i += PJ_THREADS) {
        const int r = i & (PJ_T - 1), s = i >> 5;
        if (s0 + s < S && r0 + r < R) {
            float2 g = *reinterpret_cast<const float2*>(gy + ((b * S + s0 + s) * R + r0 + r) * 2);
            if (scale) { g.x *= sc; g.y *= sc; }
            tile[s][r] = g;
        }
    }
    __syncthreads();
    double acc[10] = {};
    for (int i = threadIdx.x; i < PJ_T * PJ_T; i += PJ_THREADS) {
        const int s = i & (PJ_T - 1), r = i >> 5;
        if (s0 + s < S && r0 + r < R) {
            const float2 g = tile[s][r];
            float xs[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) xs[c] = x[((b * 4 + c) * R + r0 + r) * S + s0 + s];
            proj_accumulate(acc, g.x, g.y, xs);
#pragma unroll
            for (int c = 0; c < 4; ++c) gx[((b * 4 + c) * R + r0 + r) * S + s0 + s] = fmaf(p.w[1][c], g.y, p.w[0][c] * g.x);
        }
    }
    block_partials(acc, part, ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

// one workgroup: the partials in index order, 256 workgroups' worth staged in LDS at a time (the order, and with it the
// bits, of a plain loop over the array); thread j < 10 owns sum j
__global__ __launch_bounds__(PJ_THREADS) void head_proj_tail_kernel(const double* __restrict__ part, int64_t nwg,
                                                                    float* __restrict__ gw, float* __restrict__ gb) {
    __shared__ double sp[PJ_THREADS * 10];
    double total = 0.0;
    for (int64_t base = 0; base < nwg; base += PJ_THREADS) {
        const int cnt = (int)(nwg - base < PJ_THREADS ? nwg - base : PJ_THREADS);
        for (int i = threadIdx.x; i < cnt * 10; i += PJ_THREADS) sp[i] = part[base * 10 + i];
        __syncthreads();
        if (threadIdx.x < 10)
            for (int i = 0; i < cnt; ++i) total += sp[i * 10 + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < 8) gw[threadIdx.x] = (float)total;
    else if (threadIdx.x < 10) gb[threadIdx.x - 8] = (float)total;
}

static bool proj_shape_ok(int64_t B, int64_t R, int64_t S) {
    return B >= 1 && B <= 65535 && R >= 1 && R <= HEAD_PROJ_MAX_R && S >= 1 && S <= HEAD_PROJ_MAX_S &&
           R * S <= HEAD_PROJ_MAX_RS;
}
static int64_t proj_chunks(int64_t n) { return (n + HEAD_PROJ_CHUNK - 1) / HEAD_PROJ_CHUNK; }
static int64_t proj_tiles(int64_t R, int64_t S) { return ((R + PJ_T - 1) / PJ_T) * ((S + PJ_T - 1) / PJ_T); }

int64_t head_proj_ws_doubles(int64_t B, int64_t R, int64_t S) {
    if (!proj_shape_ok(B, R, S)) return 0;
    const int64_t a = proj_chunks(R * S), t = R > 1 ? proj_tiles(R, S) : 0;      // (R == 1 never takes the tiles)
    return 10 * B * (a > t ? a : t);
}

int head_proj_fwd_launch(const float* x, const float* w, const float* bias, int64_t B, int64_t R, int64_t S, float* y,
                         hipStream_t s) {
    if (!x || !w || !bias || !y || !proj_shape_ok(B, R, S)) return -1;
    const dim3 grid = R == 1 ? dim3((unsigned)proj_chunks(S), (unsigned)B)
                             : dim3((unsigned)((S + PJ_T - 1) / PJ_T), (unsigned)((R + PJ_T - 1) / PJ_T), (unsigned)B);
    hipLaunchKernelGGL(head_proj_fwd_kernel, grid, dim3(PJ_THREADS), 0, s, x, w, bias, R, S, y);
    return (int)hipGetLastError();
}

int head_proj_bwd_launch(const float* gy, int channel_first, const float* scale, const float* x, const float* w,
                         int64_t B, int64_t R, int64_t S, float* gx, float* gw, float* gb, double* part, hipStream_t s) {
    if (!gy || !x || !w || !gx || !gw || !gb || !part || !proj_shape_ok(B, R, S)) return -1;
    int64_t nwg;
    if (channel_first || R == 1) {
        const int64_t n = R * S;
        const dim3 grid((unsigned)proj_chunks(n), (unsigned)B);
        nwg = proj_chunks(n) * B;
        if (channel_first)
            hipLaunchKernelGGL(head_proj_bwd_stream_kernel<true>, grid, dim3(PJ_THREADS), 0, s, gy, scale, x, w, n, gx,
                               part);
        else
            hipLaunchKernelGGL(head_proj_bwd_stream_kernel<false>, grid, dim3(PJ_THREADS), 0, s, gy, scale, x, w, n, gx,
                               part);
    } else {
        const dim3 grid((unsigned)((S + PJ_T - 1) / PJ_T), (unsigned)((R + PJ_T - 1) / PJ_T), (unsigned)B);
        nwg = proj_tiles(R, S) * B;
        hipLaunchKernelGGL(head_proj_bwd_tile_kernel, grid, dim3(PJ_THREADS), 0, s, gy, scale, x, w, R, S, gx, part);
    }
    hipLaunchKernelGGL(head_proj_tail_kernel, dim3(1), dim3(PJ_THREADS), 0, s, (const double*)part, nwg, gw, gb);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------- the attention vector
constexpr int AV_D = HEAD_ATTN_D, AV_TEXT = HEAD_ATTN_TEXT;

// out[b][n] = bias[n] + sum_k W[n][k] in[b][k]: one wave per output element, lane l takes k = l, l + 64, ... in
// ascending order, then the shuffle tree.  grid ceil(B N / 4) workgroups of 4 waves.
__global__ __launch_bounds__(256) void attn_vec_matvec_kernel(const float* __restrict__ in, int64_t in_stride,
                                                              const float* __restrict__ W,
                                                              const float* __restrict__ bias, int64_t B, int N, int K,
                                                              float* __restrict__ out, int64_t out_stride) {
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= B * N) return;
    const int64_t b = e / N;
    const int n = (int)(e % N), lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int k = lane; k < K; k += 64) acc += (double)W[(int64_t)n * K + k] * (double)in[b * in_stride + k];
    acc = wave_sum_d(acc);
    if (lane == 0) out[b * out_stride + n] = (float)(acc + (double)bias[n]);
}

// One linear layer's backward, y = W u + bias with W (N, K): g (B, N) = dL/dy, u (B, K) its input.
//   workgroups 0 .. N-1:      gW[n][k] = sum_b g[b][n] u[b][k] (thread per k, b ascending), gbias[n] = sum_b g[b][n]
//   workgroups N .. N+B-1:    gu[b][k] = sum_n W[n][k] g[b][n] (thread per k, n ascending); skipped when gu == nullptr
// g and u have row strides gs and us (keep's two intermediates are interleaved per item).
__global__ __launch_bounds__(256) void attn_vec_linear_bwd_kernel(const float* __restrict__ g, int64_t gs,
                                                                  const float* __restrict__ u, int64_t us,
                                                                  const float* __restrict__ W, int64_t B, int N, int K,
                                                                  float* __restrict__ gW, float* __restrict__ gbias,
                                                                  float* __restrict__ gu) {
    if ((int)blockIdx.x < N) {
        const int n = blockIdx.x;
        for (int k = threadIdx.x; k < K; k += 256) {
            double acc = 0.0;
            for (int64_t b = 0; b < B; ++b) acc += (double)g[b * gs + n] * (double)u[b * us + k];
            gW[(int64_t)n * K + k] = (float)acc;
        }
        if (threadIdx.x == 0) {
            double acc = 0.0;
            for (int64_t b = 0; b < B; ++b) acc += (double)g[b * gs + n];
            gbias[n] = (float)acc;
        }
    } else {
        const int64_t b = (int64_t)blockIdx.x - N;
        for (int k = threadIdx.x; k < K; k += 256) {
            double acc = 0.0;
            for (int n = 0; n < N; ++n) acc += (double)W[(int64_t)n * K + k] * (double)g[b * gs + n];
            gu[b * K + k] = (float)acc;
        }
    }
}

__global__ void attn_vec_zero_kernel(float* __restrict__ a, int64_t na, float* __restrict__ b, int64_t nb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) a[i] = 0.f;
    if (i < nb) b[i] = 0.f;
}

int head_attn_vec_fwd_launch(const float* text, const float* wv, const float* bv, const float* w_in, const float* b_in,
                             const float* wo, const float* bo, int64_t B, float* a, float* keep, hipStream_t s) {
    if (!text || !wv || !bv || !w_in || !b_in || !wo || !bo || !a || !keep || B < 1 || B > 65535) return -1;
    const dim3 grid((unsigned)((B * AV_D + 3) / 4));
    hipLaunchKernelGGL(attn_vec_matvec_kernel, grid, dim3(256), 0, s, text, (int64_t)AV_TEXT, wv, bv, B, AV_D, AV_TEXT,
                       keep, (int64_t)2 * AV_D);
    hipLaunchKernelGGL(attn_vec_matvec_kernel, grid, dim3(256), 0, s, (const float*)keep, (int64_t)2 * AV_D,
                       w_in + (int64_t)2 * AV_D * AV_D, b_in + 2 * AV_D, B, AV_D, AV_D, keep + AV_D, (int64_t)2 * AV_D);
    hipLaunchKernelGGL(attn_vec_matvec_kernel, grid, dim3(256), 0, s, (const float*)keep + AV_D, (int64_t)2 * AV_D, wo,
                       bo, B, AV_D, AV_D, a, (int64_t)AV_D);
    return (int)hipGetLastError();
}

int head_attn_vec_bwd_launch(const float* ga, const float* text, const float* keep, const float* w_in, const float* wo,
                             int64_t B, float* gwv, float* gbv, float* gw_in, float* gb_in, float* gwo, float* gbo,
                             hipStream_t s) {
    if (!ga || !text || !keep || !w_in || !wo || !gwv || !gbv || !gw_in || !gb_in || !gwo || !gbo || B < 1 ||
        B > HEAD_ATTN_MAX_B)
        return -1;
    // dL/dv2 and dL/dv1 (B, 384 each) live in the dead two thirds of grad_w_in until the last launch zeroes them:
    // 2 B 384 <= 768 x 384 floats for B <= HEAD_ATTN_MAX_B
    float* gv2 = gw_in;
    float* gv1 = gw_in + B * AV_D;
    const int64_t live = (int64_t)2 * AV_D * AV_D;
    const dim3 grid((unsigned)(AV_D + B));
    hipLaunchKernelGGL(attn_vec_linear_bwd_kernel, grid, dim3(256), 0, s, ga, (int64_t)AV_D, keep + AV_D,
                       (int64_t)2 * AV_D, wo, B, AV_D, AV_D, gwo, gbo, gv2);
    hipLaunchKernelGGL(attn_vec_linear_bwd_kernel, grid, dim3(256), 0, s, (const float*)gv2, (int64_t)AV_D, keep,
                       (int64_t)2 * AV_D, w_in + live, B, AV_D, AV_D, gw_in + live, gb_in + 2 * AV_D, gv1);
    hipLaunchKernelGGL(attn_vec_linear_bwd_kernel, dim3(AV_D), dim3(256), 0, s, (const float*)gv1, (int64_t)AV_D, text,
                       (int64_t)AV_TEXT, (const float*)nullptr, B, AV_D, AV_TEXT, gwv, gbv, (float*)nullptr);
    hipLaunchKernelGGL(attn_vec_zero_kernel, dim3((unsigned)((live + 255) / 256)), dim3(256), 0, s, gw_in, live, gb_in,
                       (int64_t)2 * AV_D);
    return (int)hipGetLastError();
}

}  // namespace athd
