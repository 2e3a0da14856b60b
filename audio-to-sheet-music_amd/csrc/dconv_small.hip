// DConv (demucs residual dilated-conv branch) for the narrow levels (C = 48, 96; hidden
// H = C/8 = 6, 12).  These layers are HBM-bound with K or N far below an MFMA tile, so they run as VALU kernels.
// x is [nb][L][C] in f32 (parity mode) or bf16 (throughput mode); h is [nb][L][H] f32.  One layer = 3 passes
// (each GroupNorm needs complete statistics before it can be applied):
//   c3:     h = b + W3 * x[t - dil], x[t], x[t + dil]          + GroupNorm statistics of h per group
//   c1stat: y = b1 + W1 * GELU(GN(h))   (2C outputs, never stored)  -> GroupNorm statistics of y per group
//   c1app:  x += scale * GLU(GN(y))     (y recomputed: K = H is tiny)
// A "group" is the GroupNorm(1) sample: one nb row of L positions (freq rows (b,f) along time, or time samples).
// Access pattern: c3 stages its x tile (+ dilation halo) in LDS with 16-B coalesced loads; the 1x1 passes map a
// lane to one position.  Every weight is read at a wave-uniform address (scalar loads, SGPR operands of the FMAs:
// no LDS traffic for weights).  Per-group GroupNorm parameters are finalised once per block into LDS.
#include <algorithm>

#include "common.h"
#include "prof.h"
#include "kernels.h"

namespace athd {

template <typename TS> struct XS;
template <> struct XS<float> {
    static ATHD_DEV float ld(const float* p, int64_t i) { return p[i]; }
};
template <> struct XS<bf16_t> {
    static ATHD_DEV float ld(const bf16_t* p, int64_t i) { return bf2f(p[i]); }
};

// 16 B of x -> EPC floats
template <typename TS>
ATHD_DEV void unpack16(const uint4 q, float* v) {
    if constexpr (sizeof(TS) == 2) {
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
        }
    } else {
        v[0] = __uint_as_float(q.x); v[1] = __uint_as_float(q.y); v[2] = __uint_as_float(q.z); v[3] = __uint_as_float(q.w);
    }
}

// Block-level {sum, sumsq} per group.  Blocks cover <= 256 consecutive positions, so with L >= 256 a block spans
// at most two groups (g0 and g0 + 1).  Shorter rows fall back to per-thread atomics.
ATHD_DEV void group_stats_add(double* __restrict__ st, int64_t p0, int64_t p, bool valid, int64_t L, float s1, float s2,
                              double* sh) {
    if (L < 256) {
        if (valid) {
            atomicAdd(&st[2 * (p / L)], (double)s1);
            atomicAdd(&st[2 * (p / L) + 1], (double)s2);
        }
        return;
    }
    const int64_t g0 = p0 / L;
    const bool second = valid && (p / L) != g0;
    double a0 = (valid && !second) ? s1 : 0.0, b0 = (valid && !second) ? s2 : 0.0;
    double a1 = second ? s1 : 0.0, b1 = second ? s2 : 0.0;
    a0 = wave_sum_d(a0); b0 = wave_sum_d(b0); a1 = wave_sum_d(a1); b1 = wave_sum_d(b1);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[4 * w] = a0; sh[4 * w + 1] = b0; sh[4 * w + 2] = a1; sh[4 * w + 3] = b1; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double v = 0.0;
        for (int i = 0; i < 4; ++i) v += sh[4 * i + threadIdx.x];
        const int64_t g = g0 + (threadIdx.x >= 2 ? 1 : 0);
        if (v != 0.0) atomicAdd(&st[2 * g + (threadIdx.x & 1)], v);
    }
}

ATHD_DEV void gn_mr(const double* st, int64_t g, double cnt, float& mean, float& rstd) {
    const double mm = st[2 * g] / cnt;
    double var = st[2 * g + 1] / cnt - mm * mm;
    if (var < 0) var = 0;
    mean = (float)mm;
    rstd = (float)(1.0 / sqrt(var + 1e-5));
}

// ---- c3: TILE positions per block, TPP = 256 / TILE threads per position, each computing H / TPP outputs
template <int C, typename TS>
__global__ __launch_bounds__(256) void dconv_c3_kernel(const TS* __restrict__ x, int64_t nb, int64_t L, int dil,
                                                       const float* __restrict__ W, const float* __restrict__ bias,
                                                       float* __restrict__ h, double* __restrict__ st) {
    constexpr int H = C / 8, K = 3 * C, HALO = 2;
    constexpr int TILE = sizeof(TS) == 2 ? 256 : 128;
    constexpr int TPP = 256 / TILE, HJ = H / TPP;
    constexpr int ROWS = TILE + 2 * HALO;
    constexpr int EPC = 16 / sizeof(TS);                    // elements per 16-B chunk
    constexpr int CPR = C / EPC;                             // chunks per row
    __shared__ __attribute__((aligned(16))) TS xs[ROWS * C];
    __shared__ double sh[16];
    const int64_t P = nb * L;
    const int64_t p0 = (int64_t)blockIdx.x * TILE;
    for (int i = threadIdx.x; i < ROWS * CPR; i += 256) {
        const int r = i / CPR, ch = i - r * CPR;
        const int64_t pp = p0 - HALO + r;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (pp >= 0 && pp < P) v = *reinterpret_cast<const uint4*>(x + pp * C + ch * EPC);
        *reinterpret_cast<uint4*>(&xs[r * C + ch * EPC]) = v;
    }
    __syncthreads();
    const int lp = threadIdx.x / TPP, sub = threadIdx.x % TPP;
    const int64_t p = p0 + lp;
    const bool valid = p < P;
    float s1 = 0.f, s2 = 0.f;
    if (valid) {
        const int64_t t = p % L;
        float acc[HJ];
#pragma unroll
        for (int j = 0; j < HJ; ++j) acc[j] = bias[sub * HJ + j];
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            const int64_t tt = t + (tap - 1) * dil;
            if (tt < 0 || tt >= L) continue;                 // zero padding of the group row
            const TS* xr = &xs[(lp + HALO + (tap - 1) * dil) * C];
#pragma unroll 2
            for (int c0 = 0; c0 < C; c0 += EPC) {
                float v[EPC];
                unpack16<TS>(*reinterpret_cast<const uint4*>(xr + c0), v);
#pragma unroll
                for (int e = 0; e < EPC; ++e)
#pragma unroll
                    for (int j = 0; j < HJ; ++j) acc[j] += W[(sub * HJ + j) * K + tap * C + c0 + e] * v[e];
            }
        }
        float* hr = h + p * H + sub * HJ;
#pragma unroll
        for (int j = 0; j < HJ; ++j) {
            hr[j] = acc[j];
            s1 += acc[j];
            s2 += acc[j] * acc[j];
        }
    }
    group_stats_add(st, p0, p, valid, L, s1, s2, sh);
}

// GELU(GroupNorm(h)) of one position (the first GroupNorm of the layer, fused into both 1x1 passes)
template <int H, bool FAST>
ATHD_DEV void load_hg(const float* __restrict__ h, int64_t p, float mean, float rstd, const float* g1w, const float* g1b,
                      float* hv) {
#pragma unroll
    for (int j = 0; j < H; ++j) hv[j] = gelu<FAST>((h[p * H + j] - mean) * rstd * g1w[j] + g1b[j]);
}

// GroupNorm (mean, rstd) of the groups [g_first, g_first + n) a block touches, into LDS (n <= GN_TAB); the caller
// synchronises.  Blocks touching more groups (very short rows) compute per thread.
constexpr int GN_TAB = 8;
ATHD_DEV void gn_table(const double* st, double cnt, int64_t g_first, int64_t n, float* tm, float* tr) {
    if (n <= GN_TAB && (int64_t)threadIdx.x < n) gn_mr(st, g_first + threadIdx.x, cnt, tm[threadIdx.x], tr[threadIdx.x]);
}
ATHD_DEV void gn_lookup(const double* st, double cnt, int64_t g, int64_t g_first, int64_t n, const float* tm,
                        const float* tr, float& mean, float& rstd) {
    if (n <= GN_TAB) {
        mean = tm[g - g_first];
        rstd = tr[g - g_first];
    } else {
        gn_mr(st, g, cnt, mean, rstd);
    }
}

// ---- c1stat: one thread per position.  y = W h + b (2C channels) only feeds the GroupNorm statistics, and
// sum_n y_n = sum b + ws.h, sum_n y_n^2 = sum b^2 + 2 v.h + h^T G h with the 1x1 conv's moments (G = W^T W, v = W^T b,
// ws = W^T 1: ctx.h DConvW::gram1, computed in fp64 at pack time): H^2 + 3H FMAs per position instead of 2 x 2C x H
template <int C, bool FAST>
__global__ __launch_bounds__(256) void dconv_c1_stats_kernel(const float* __restrict__ h, int64_t nb, int64_t L,
                                                             const double* __restrict__ st_h,
                                                             const float* __restrict__ g1w, const float* __restrict__ g1b,
                                                             const float* __restrict__ gram, double* __restrict__ st_y) {
    constexpr int H = C / 8;
    __shared__ float tm[GN_TAB], tr[GN_TAB];
    __shared__ double sh[16];
    const int64_t P = nb * L;
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    const int64_t gf = p0 / L, ng = (std::min<int64_t>(p0 + 255, P - 1)) / L - gf + 1;
    gn_table(st_h, (double)L * H, gf, ng, tm, tr);
    __syncthreads();
    const int64_t p = p0 + threadIdx.x;
    const bool valid = p < P;
    float s1 = 0.f, s2 = 0.f;
    if (valid) {
        float mean, rstd;
        gn_lookup(st_h, (double)L * H, p / L, gf, ng, tm, tr, mean, rstd);
        float hv[H];
        load_hg<H, FAST>(h, p, mean, rstd, g1w, g1b, hv);
        const float* G = gram;
        const float* v = gram + H * H;
        const float* ws = v + H;
        float q = 0.f, lv = 0.f, lw = 0.f;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < H; ++k) t += G[j * H + k] * hv[k];
            q += hv[j] * t;
            lv += v[j] * hv[j];
            lw += ws[j] * hv[j];
        }
        s1 = ws[H] + lw;
        s2 = ws[H + 1] + (2.f * lv + q);
    }
    group_stats_add(st_y, p0, p, valid, L, s1, s2, sh);
}

// ---- c1app: one thread per position, all C channels: x[p][:] += scale * GLU(GN(y)); every weight / affine read is
// wave-uniform (scalar loads), x moves in 16-B chunks
template <int C, typename TS, bool FAST>
__global__ __launch_bounds__(256) void dconv_c1_apply_kernel(TS* __restrict__ x, const float* __restrict__ h, int64_t nb,
                                                             int64_t L, const double* __restrict__ st_h,
                                                             const float* __restrict__ g1w, const float* __restrict__ g1b,
                                                             const float* __restrict__ W, const float* __restrict__ bias,
                                                             const double* __restrict__ st_y,
                                                             const float* __restrict__ g2w, const float* __restrict__ g2b,
                                                             const float* __restrict__ scale) {
    constexpr int H = C / 8, N = 2 * C;
    constexpr int EPC = 16 / sizeof(TS);
    __shared__ float tm1[GN_TAB], tr1[GN_TAB], tm2[GN_TAB], tr2[GN_TAB];
    const int64_t P = nb * L;
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    const int64_t gf = p0 / L, ng = (std::min<int64_t>(p0 + 255, P - 1)) / L - gf + 1;
    gn_table(st_h, (double)L * H, gf, ng, tm1, tr1);
    gn_table(st_y, (double)L * N, gf, ng, tm2, tr2);
    __syncthreads();
    const int64_t p = p0 + threadIdx.x;
    if (p >= P) return;
    const int64_t g = p / L;
    float m1, r1, m2, r2;
    gn_lookup(st_h, (double)L * H, g, gf, ng, tm1, tr1, m1, r1);
    gn_lookup(st_y, (double)L * N, g, gf, ng, tm2, tr2, m2, r2);
    float hv[H];
    load_hg<H, FAST>(h, p, m1, r1, g1w, g1b, hv);
    TS* xp = x + p * C;
#pragma unroll 2
    for (int c0 = 0; c0 < C; c0 += EPC) {
        uint4 q = *reinterpret_cast<const uint4*>(xp + c0);
        float e[EPC];
        unpack16<TS>(q, e);
#pragma unroll
        for (int k = 0; k < EPC; ++k) {
            const int c = c0 + k;
            float a = bias[c], gt = bias[C + c];
#pragma unroll
            for (int j = 0; j < H; ++j) {
                a += W[c * H + j] * hv[j];
                gt += W[(C + c) * H + j] * hv[j];
            }
            a = (a - m2) * r2 * g2w[c] + g2b[c];
            gt = (gt - m2) * r2 * g2w[C + c] + g2b[C + c];
            const float o = scale[c] * (a * sigmoid<FAST>(gt));
            e[k] += o;                                // rounded once below (pack2bf: RNE, as f2bf)
        }
        if constexpr (sizeof(TS) == 2)
            q = make_uint4(pack2bf(e[0], e[1]), pack2bf(e[2], e[3]), pack2bf(e[4], e[5]), pack2bf(e[6], e[7]));
        else
            q = make_uint4(__float_as_uint(e[0]), __float_as_uint(e[1]), __float_as_uint(e[2]), __float_as_uint(e[3]));
        *reinterpret_cast<uint4*>(xp + c0) = q;
    }
}

template <int C, typename TS, bool FAST>
static void dconv_small_t(const DconvDesc& d, hipStream_t s) {
    constexpr int H = C / 8, TILE = sizeof(TS) == 2 ? 256 : 128;
    const int64_t P = d.M, L = d.L, nb = P / L;
    const double px = (double)P;
    const double xb = (double)sizeof(TS);
    const char* tn = sizeof(TS) == 2 ? "unsignedshort" : "float";   // (rocprofv3 symbol spelling)
    {
        KScope ks(s);
        if (ks.on()) ks.begin(klabel("dconv_c3_kernel<%d,%s>", C, tn), 2.0 * px * H * 3 * C, px * (C * xb + H * 4));
        hipLaunchKernelGGL((dconv_c3_kernel<C, TS>), dim3((unsigned)((P + TILE - 1) / TILE)), dim3(256), 0, s,
                           (const TS*)d.x, nb, L, d.dil, d.w3f, d.b3, d.h, d.st_h);
    }
    {
        KScope ks(s);
        if (ks.on()) ks.begin(klabel("dconv_c1_stats_kernel<%d,%s>", C, FAST ? "true" : "false"), 2.0 * px * (H * H + 3 * H), px * H * 4);
        hipLaunchKernelGGL((dconv_c1_stats_kernel<C, FAST>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, d.h, nb,
                           L, d.st_h, d.g1w, d.g1b, d.gram, d.st_y);
    }
    {
        KScope ks(s);
        if (ks.on()) ks.begin(klabel("dconv_c1_apply_kernel<%d,%s,%s>", C, tn, FAST ? "true" : "false"), 2.0 * px * 2 * C * H, px * (H * 4 + 2 * C * xb));
        hipLaunchKernelGGL((dconv_c1_apply_kernel<C, TS, FAST>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s,
                           (TS*)d.x, d.h, nb, L, d.st_h, d.g1w, d.g1b, d.w1f, d.b1, d.st_y, d.g2w, d.g2b, d.scale);
    }
}

template <int C>
static void dconv_small_c(const DconvDesc& d, hipStream_t s) {
    if (d.x_bf16) { if (d.fast) dconv_small_t<C, bf16_t, true>(d, s); else dconv_small_t<C, bf16_t, false>(d, s); }
    else { if (d.fast) dconv_small_t<C, float, true>(d, s); else dconv_small_t<C, float, false>(d, s); }
}

int dconv_small_launch(const DconvDesc& d, hipStream_t s) {
    if (d.dil < 1 || d.dil > 2 || !d.gram || !dconv_narrow(d.C) || d.L < 1) return -2;
    if (d.C == 48) dconv_small_c<48>(d, s); else dconv_small_c<96>(d, s);
    return (int)hipGetLastError();
}

}  // namespace athd
