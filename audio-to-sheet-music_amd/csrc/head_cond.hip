// Head training's text-conditioning stage (gfx950), both directions, from raw f32 weights (ATHTDemucs_v2.py:21-58 with
// ONE key, so the attention output is a per-item vector a_b and the query side drops out).
//
// Forward, X one item's (384, N) channel-first slab, columns = tokens:
//   U = X + a_b, H = W0 U + b0, G = gelu_erf(H), V = U + W2 G + b2, (mu, r) = column mean and 1 / sqrt(var + 1e-5) over
//   the 384 channels, Vh = (V - mu) r, Y = gamma Vh + beta, written channel-first.
// Backward from dY (X gets no gradient, it comes from the frozen half):
//   D = gamma dY, dV = r (D - mean_c D - Vh mean_c(D Vh)), dgamma = sum dY Vh, dbeta = sum dY, dW2 = sum dV G^T,
//   db2 = sum dV, dH = (W2^T dV) gelu'(H), dW0 = sum dH U^T, db0 = sum dH, da_b = sum_n dV + W0^T sum_n dH per item.
//
// Tiling.  A workgroup of 8 waves owns TN = 64 tokens of ONE item (tiles never straddle items; the last tile of an item
// is padded with zero columns, whose dY is zero, so their dV and dH are exactly zero).  The tile's B operand lives in
// LDS as [channel][68] (272 B rows: the four k groups of a 16x16x4 MFMA fall into four disjoint sets of 16 banks); each
// wave owns 48 output channels x 64 tokens = 3 x 4 accumulator tiles and reads its rows of the weight matrix straight
// from global memory (L2), 16 B per lane along k.  One LDS tile is reused for U, G, dY, dV and dH in turn: what a later
// phase needs of an earlier tile (the residual U, gelu'(H), Vh) stays in registers at the lane's own accumulator
// positions.  All arithmetic is f32: v_mfma_f32_16x16x4_f32 is an exact k-ordered f32 fma chain.
//
// Determinism.  No atomics.  Row sums over tokens are written per tile (part[tile][4][384]) and summed per item and then
// over items in ascending order; the weight gradients are a split-K GEMM over the tiles in a FIXED number of slices
// (WG_SLICES), summed in slice order.  Every output element is written, none is accumulated into.
#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "prof.h"

namespace athd {

namespace {

constexpr int C = HEAD_COND_C, TN = HEAD_COND_TN, LS = TN + 4;
constexpr int NW = 8, NTH = 64 * NW;             // waves, threads per workgroup
constexpr int RT = C / 16 / NW, NT = TN / 16;    // accumulator tiles per wave: 3 row tiles x 4 token tiles
constexpr int WG_SLICES = HEAD_COND_SLICES;
static_assert(RT * 16 * NW == C && NT * 16 == TN && (LS % 16) == 4, "tile plan");

struct Lane {
    int wave, r16, q4, tid;
    __device__ Lane() : wave(threadIdx.x >> 6), r16(threadIdx.x & 15), q4((threadIdx.x >> 4) & 3), tid(threadIdx.x) {}
    // accumulator element (rt, nt, r) is channel row(rt, r), token col(nt)
    __device__ int row(int rt, int r) const { return wave * (RT * 16) + rt * 16 + 4 * q4 + r; }
    __device__ int col(int nt) const { return nt * 16 + r16; }
};

typedef f32x4_t Acc[RT][NT];

// acc += W[this wave's 48 rows][0..384) . T, T the LDS tile [k][LS].  Lane (r16, q4) loads W[row][kk + 4 q4 .. + 3]; MFMA
// s of a 16-block takes k = kk + 4 q4 + s from lane group q4, for both operands.
ATHD_DEV void gemm_tile(const float* __restrict__ W, const float* __restrict__ lds, const Lane& L, Acc& acc) {
    const float* wrow = W + (int64_t)(L.wave * (RT * 16) + L.r16) * C + 4 * L.q4;
    const float* bl = lds + 4 * L.q4 * LS + L.r16;
#pragma unroll 2
    for (int kk = 0; kk < C; kk += 16) {
        float4 a[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) a[rt] = *reinterpret_cast<const float4*>(wrow + rt * 16 * C + kk);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = bl[(kk + s) * LS + nt * 16];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float av = s == 0 ? a[rt].x : s == 1 ? a[rt].y : s == 2 ? a[rt].z : a[rt].w;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[rt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[nt], acc[rt][nt], 0, 0, 0);
            }
        }
    }
}

// src[c * N + j], j < valid (columns past it read as zero), plus add[c] -> lds[c][j] and, if blk, the dense tile block
// blk[c][TN].  16-byte loads when every row of the slab is 16-byte aligned (vec), scalar otherwise.
ATHD_DEV void load_tile(const float* __restrict__ src, int64_t N, int valid, bool vec, const float* __restrict__ add,
                        float* __restrict__ lds, float* __restrict__ blk, int tid) {
    for (int i = tid; i < C * (TN / 4); i += NTH) {
        const int c = i / (TN / 4), j = (i % (TN / 4)) * 4;
        const float* p = src + (int64_t)c * N + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vec && j + 3 < valid) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            if (j < valid) v.x = p[0];
            if (j + 1 < valid) v.y = p[1];
            if (j + 2 < valid) v.z = p[2];
            if (j + 3 < valid) v.w = p[3];
        }
        if (add) {
            const float av = add[c];
            v = make_float4(v.x + av, v.y + av, v.z + av, v.w + av);
        }
        *reinterpret_cast<float4*>(lds + c * LS + j) = v;
        if (blk) *reinterpret_cast<float4*>(blk + c * TN + j) = v;
    }
}

// the LDS tile -> dst[c * N + j], j < valid
ATHD_DEV void store_tile(const float* __restrict__ lds, float* __restrict__ dst, int64_t N, int valid, bool vec, int tid) {
    for (int i = tid; i < C * (TN / 4); i += NTH) {
        const int c = i / (TN / 4), j = (i % (TN / 4)) * 4;
        const float4 v = *reinterpret_cast<const float4*>(lds + c * LS + j);
        float* p = dst + (int64_t)c * N + j;
        if (vec && j + 3 < valid) {
            *reinterpret_cast<float4*>(p) = v;
        } else {
            if (j < valid) p[0] = v.x;
            if (j + 1 < valid) p[1] = v.y;
            if (j + 2 < valid) p[2] = v.z;
            if (j + 3 < valid) p[3] = v.w;
        }
    }
}

// the LDS tile -> the dense tile block blk[c][TN], all TN columns
ATHD_DEV void store_block(const float* __restrict__ lds, float* __restrict__ blk, int tid) {
    for (int i = tid; i < C * (TN / 4); i += NTH) {
        const int c = i / (TN / 4), j = (i % (TN / 4)) * 4;
        *reinterpret_cast<float4*>(blk + c * TN + j) = *reinterpret_cast<const float4*>(lds + c * LS + j);
    }
}

ATHD_DEV void acc_to_lds(const Acc& v, float* __restrict__ lds, const Lane& L) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[L.row(rt, r) * LS + L.col(nt)] = v[rt][nt][r];
}

// Column sums over the 384 channels of the lane's columns: own registers, then the four lane groups of the wave (xor 16,
// 32), then the eight waves through red[NW][TN] in wave order.  Ends with every lane holding the totals of its NT
// columns.  One __syncthreads inside; the caller alternates between two red buffers.
ATHD_DEV void col_sums(float (&p)[NT], float* __restrict__ red, const Lane& L) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        p[nt] += __shfl_xor(p[nt], 16);
        p[nt] += __shfl_xor(p[nt], 32);
        if (L.q4 == 0) red[L.wave * TN + L.col(nt)] = p[nt];
    }
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        float s = red[L.col(nt)];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[w * TN + L.col(nt)];
        p[nt] = s;
    }
}

// Row sums over the tile's TN tokens: the lane's four token tiles in order, then the 16 lanes of a group (xor 1 .. 8);
// each row belongs to exactly one wave, which writes out[row].
template <class F>
ATHD_DEV void row_sums_of(F v, float* __restrict__ out, const Lane& L) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = v(rt, 0, r);
#pragma unroll
            for (int nt = 1; nt < NT; ++nt) s += v(rt, nt, r);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            s += __shfl_xor(s, 8);
            if (L.r16 == 0) out[L.row(rt, r)] = s;
        }
}
ATHD_DEV void row_sums_out(const Acc& v, float* __restrict__ out, const Lane& L) {
    row_sums_of([&](int rt, int nt, int r) { return v[rt][nt][r]; }, out, L);
}

// U (LDS; xsrc, add: where load_tile took it from) -> V = U + W2 gelu(W0 U + b0) + b2 normalised over the channels: vh = (V - mu) r in registers, rstd per
// column; gp = gelu'(H) if wanted; G goes to gblk (the backward's workspace) if given.  Leaves the LDS tile free (all
// waves are past their last read of it).
template <bool BWD>
ATHD_DEV void stage_forward(const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w2,
                            const float* __restrict__ b2, float* __restrict__ lds, float* __restrict__ red0,
                            float* __restrict__ red1, float* __restrict__ gblk, const float* __restrict__ xsrc,
                            int64_t N, int valid, const float* __restrict__ add, const Lane& L, Acc& vh, Acc& gp,
                            float (&rstd)[NT]) {
    Acc h;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float bv = b0[L.row(rt, r)];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) h[rt][nt][r] = bv;
        }
    gemm_tile(w0, lds, L, h);
    // the second product starts from b2 alone: the residual U is added after it, in one rounding, not carried through the
    // 384 roundings of the chain at U's magnitude
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float bv = b2[L.row(rt, r)];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                vh[rt][nt][r] = bv;
                const float x = h[rt][nt][r];
                const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
                if constexpr (BWD) gp[rt][nt][r] = cdf + x * (0.39894228040143267794f * expf(-0.5f * x * x));
                h[rt][nt][r] = x * cdf;
            }
        }
    __syncthreads();                                   // every wave is done with U
    acc_to_lds(h, lds, L);
    __syncthreads();
    if constexpr (BWD) store_block(lds, gblk, L.tid);
    gemm_tile(w2, lds, L, vh);
    // + U, read again from x at the lane's positions (the same x + a as load_tile's, bit for bit; the tile is in L2)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = L.row(rt, r);
            const float av = add[row];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                vh[rt][nt][r] += (L.col(nt) < valid ? xsrc[(int64_t)row * N + L.col(nt)] : 0.f) + av;
        }
    // LayerNorm statistics, two passes: the mean, then the variance of the centred values
    float p[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        p[nt] = 0.f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) p[nt] += vh[rt][nt][r];
    }
    col_sums(p, red0, L);
    float mu[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        mu[nt] = p[nt] * (1.0f / C);
        p[nt] = 0.f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float d = vh[rt][nt][r] - mu[nt];
                vh[rt][nt][r] = d;
                p[nt] = fmaf(d, d, p[nt]);
            }
    }
    col_sums(p, red1, L);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        rstd[nt] = 1.0f / sqrtf(p[nt] * (1.0f / C) + 1e-5f);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) vh[rt][nt][r] *= rstd[nt];
    }
}

// LDS: the tile 384 x 68 x 4 = 104448 B + 2 x 8 x 64 x 4 = 4096 B: one workgroup (two waves per SIMD) per CU
// (the backward holds Vh, gelu'(H) and the running gradient tile, 3 x 48 registers, beside the product's operands: the
// compiler parks gelu'(H) in scratch across the second product, one store and one load per tile, outside the MFMA loops)
constexpr int RED = NW * TN;

__global__ __launch_bounds__(NTH) void head_cond_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                            const float* __restrict__ w0, const float* __restrict__ b0,
                                                            const float* __restrict__ w2, const float* __restrict__ b2,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int64_t N, int vec,
                                                            float* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) float lds[C * LS];
    __shared__ float red[2 * RED];
    const Lane L;
    const int64_t b = blockIdx.y;
    const int n0 = blockIdx.x * TN;
    const int valid = N - n0 < TN ? (int)(N - n0) : TN;
    load_tile(x + b * C * N + n0, N, valid, vec != 0, a + b * C, lds, nullptr, L.tid);
    __syncthreads();
    Acc vh, gp;
    float rstd[NT];
    stage_forward<false>(w0, b0, w2, b2, lds, red, red + RED, nullptr, x + b * C * N + n0, N, valid, a + b * C, L, vh,
                         gp, rstd);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float g = gamma[L.row(rt, r)], be = beta[L.row(rt, r)];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) vh[rt][nt][r] = fmaf(g, vh[rt][nt][r], be);
        }
    acc_to_lds(vh, lds, L);
    __syncthreads();
    store_tile(lds, y + b * C * N + n0, N, valid, vec != 0, L.tid);
}

// One tile of the backward: recomputes the forward from X, then dV and dH.  Writes the tile blocks U, G, dV, dH
// ([tile][384][TN], padded columns included) for the weight-gradient GEMM and the tile's four row sums
// part[tile][{dY Vh, dY, dV, dH}][384].
__global__ __launch_bounds__(NTH) void head_cond_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                            const float* __restrict__ a, const float* __restrict__ w0,
                                                            const float* __restrict__ b0, const float* __restrict__ w2,
                                                            const float* __restrict__ b2,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ w2t, int64_t N, int vec,
                                                            float* __restrict__ ublk, float* __restrict__ gblk,
                                                            float* __restrict__ dvblk, float* __restrict__ dhblk,
                                                            float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float lds[C * LS];
    __shared__ float red[2 * RED];
    const Lane L;
    const int64_t b = blockIdx.y;
    const int64_t tile = b * gridDim.x + blockIdx.x;
    const int n0 = blockIdx.x * TN;
    const int valid = N - n0 < TN ? (int)(N - n0) : TN;
    const int64_t blk = tile * (int64_t)(C * TN);
    float* prt = part + tile * (4 * C);
    load_tile(x + b * C * N + n0, N, valid, vec != 0, a + b * C, lds, ublk + blk, L.tid);
    __syncthreads();
    Acc vh, gp;
    float rstd[NT];
    stage_forward<true>(w0, b0, w2, b2, lds, red, red + RED, gblk + blk, x + b * C * N + n0, N, valid, a + b * C, L, vh,
                        gp, rstd);
    // dY (zero in the padded columns)
    load_tile(gy + b * C * N + n0, N, valid, vec != 0, nullptr, lds, nullptr, L.tid);
    __syncthreads();
    Acc d;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) d[rt][nt][r] = lds[L.row(rt, r) * LS + L.col(nt)];
    row_sums_out(d, prt + C, L);                                           // dbeta
    row_sums_of([&](int rt, int nt, int r) { return d[rt][nt][r] * vh[rt][nt][r]; }, prt, L);       // dgamma
    float m1[NT], m2[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) m1[nt] = m2[nt] = 0.f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float g = gamma[L.row(rt, r)];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float v = g * d[rt][nt][r];
                d[rt][nt][r] = v;
                m1[nt] += v;
                m2[nt] = fmaf(v, vh[rt][nt][r], m2[nt]);
            }
        }
    col_sums(m1, red, L);
    col_sums(m2, red + RED, L);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float c1 = m1[nt] * (1.0f / C), c2 = m2[nt] * (1.0f / C);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) d[rt][nt][r] = rstd[nt] * (d[rt][nt][r] - c1 - vh[rt][nt][r] * c2);
    }
    row_sums_out(d, prt + 2 * C, L);                                       // sum_n dV: db2 and the item's share of da
    // (col_sums' barriers: every wave has read its dY)
    acc_to_lds(d, lds, L);
    __syncthreads();
    store_block(lds, dvblk + blk, L.tid);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) d[rt][nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    gemm_tile(w2t, lds, L, d);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) d[rt][nt] *= gp[rt][nt];
    row_sums_out(d, prt + 3 * C, L);                                       // sum_n dH: db0 and W0^T's operand of da
    __syncthreads();                                                       // every wave is done with dV
    acc_to_lds(d, lds, L);
    __syncthreads();
    store_block(lds, dhblk + blk, L.tid);
}

// out[j][i] = in[i][j], 384 x 384
__global__ __launch_bounds__(256) void head_cond_transpose_kernel(const float* __restrict__ in, float* __restrict__ out) {
    __shared__ float t[32][33];
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    for (int e = threadIdx.x; e < 1024; e += 256) t[e >> 5][e & 31] = in[(i0 + (e >> 5)) * C + j0 + (e & 31)];
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += 256) out[(j0 + (e >> 5)) * C + i0 + (e & 31)] = t[e & 31][e >> 5];
}

// Weight gradients: wpart[slice][m][i][j] = sum over the slice's tiles and their TN tokens of A_m[i][.] B_m[j][.], with
// (A_0, B_0) = (dV, G) for dW2 and (A_1, B_1) = (dH, U) for dW0.  Workgroup = a 128 x 128 block of one matrix in one
// slice, four waves of 64 x 64; both operands are read from the tile blocks with 16 B per lane along the token axis (the
// same k permutation as gemm_tile).  grid (9, 2, WG_SLICES).
__global__ __launch_bounds__(256) void head_cond_wgrad_kernel(const float* __restrict__ ublk,
                                                              const float* __restrict__ gblk,
                                                              const float* __restrict__ dvblk,
                                                              const float* __restrict__ dhblk, int64_t ntile,
                                                              float* __restrict__ wpart) {
    const int m = blockIdx.y, s = blockIdx.z;
    const float* A = m == 0 ? dvblk : dhblk;
    const float* Bm = m == 0 ? gblk : ublk;
    const int wave = threadIdx.x >> 6, r16 = threadIdx.x & 15, q4 = (threadIdx.x >> 4) & 3;
    const int i0 = (blockIdx.x / 3) * 128 + (wave >> 1) * 64, j0 = (blockIdx.x % 3) * 128 + (wave & 1) * 64;
    const int64_t per = (ntile + WG_SLICES - 1) / WG_SLICES;
    const int64_t t0 = s * per, t1 = t0 + per < ntile ? t0 + per : ntile;
    f32x4_t acc[4][4];
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) acc[it][jt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int64_t t = t0; t < t1; ++t) {
        const float* At = A + t * (int64_t)(C * TN) + (i0 + r16) * TN + 4 * q4;
        const float* Bt = Bm + t * (int64_t)(C * TN) + (j0 + r16) * TN + 4 * q4;
#pragma unroll
        for (int kk = 0; kk < TN; kk += 16) {
            float4 av[4], bv[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                av[it] = *reinterpret_cast<const float4*>(At + it * 16 * TN + kk);
                bv[it] = *reinterpret_cast<const float4*>(Bt + it * 16 * TN + kk);
            }
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[it].x, bv[jt].x, acc[it][jt], 0, 0, 0);
                    acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[it].y, bv[jt].y, acc[it][jt], 0, 0, 0);
                    acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[it].z, bv[jt].z, acc[it][jt], 0, 0, 0);
                    acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[it].w, bv[jt].w, acc[it][jt], 0, 0, 0);
                }
        }
    }
    float* o = wpart + ((int64_t)s * 2 + m) * (C * C);
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[(i0 + it * 16 + 4 * q4 + r) * C + j0 + jt * 16 + r16] = acc[it][jt][r];
}

// gw2, gw0 = the slices of wpart summed in slice order
__global__ __launch_bounds__(256) void head_cond_wsum_kernel(const float* __restrict__ wpart, float* __restrict__ gw2,
                                                             float* __restrict__ gw0) {
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;          // over 2 x 384 x 384
    if (e >= 2 * C * C) return;
    float4 v = *reinterpret_cast<const float4*>(wpart + e);
    for (int s = 1; s < WG_SLICES; ++s) {
        const float4 u = *reinterpret_cast<const float4*>(wpart + (int64_t)s * (2 * C * C) + e);
        v = make_float4(v.x + u.x, v.y + u.y, v.z + u.z, v.w + u.w);
    }
    float* o = e < C * C ? gw2 + e : gw0 + (e - C * C);
    *reinterpret_cast<float4*>(o) = v;
}

// item[b][q][c] = the item's tiles of part[.][q][c] summed in tile order; grid (B, 4), 384 threads
__global__ __launch_bounds__(C) void head_cond_item_kernel(const float* __restrict__ part, int tpi,
                                                           float* __restrict__ item) {
    const int64_t b = blockIdx.x;
    const int q = blockIdx.y, c = threadIdx.x;
    const float* p = part + (b * tpi * 4 + q) * C + c;
    float s = p[0];
    for (int t = 1; t < tpi; ++t) s += p[(int64_t)t * (4 * C)];
    item[(b * 4 + q) * C + c] = s;
}

// blocks 0 .. B-1: ga[b][j] = sum_n dV[j] + sum_i W0[i][j] (sum_n dH)[i], i ascending; block B: the four bias-like
// gradients, the items summed in order.  384 threads.
__global__ __launch_bounds__(C) void head_cond_vec_kernel(const float* __restrict__ item, const float* __restrict__ w0,
                                                          int64_t B, float* __restrict__ ggamma,
                                                          float* __restrict__ gbeta, float* __restrict__ gb2,
                                                          float* __restrict__ gb0, float* __restrict__ ga) {
    __shared__ float sh[C];
    const int j = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b == B) {
        float* outs[4] = {ggamma, gbeta, gb2, gb0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float s = item[q * C + j];
            for (int64_t i = 1; i < B; ++i) s += item[(i * 4 + q) * C + j];
            outs[q][j] = s;
        }
        return;
    }
    sh[j] = item[(b * 4 + 3) * C + j];
    __syncthreads();
    // four interleaved chains (i mod 4), combined pairwise, then the direct term: shorter chains, smaller partial sums
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < C; i += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] = fmaf(w0[(i + u) * C + j], sh[i + u], s[u]);
    }
    ga[b * C + j] = ((s[0] + s[1]) + (s[2] + s[3])) + item[(b * 4 + 2) * C + j];
}

bool bad_shape(int64_t B, int64_t N) { return B < 1 || B > 65535 || N < 1 || N > HEAD_COND_MAX_N; }

// 16-byte rows: the slab's base and every row stride
bool vec_ok(const void* p, int64_t N) { return (N & 3) == 0 && ((uintptr_t)p & 15) == 0; }

}  // namespace

int64_t head_cond_ws_floats(int64_t B, int64_t N) {
    if (bad_shape(B, N)) return 0;
    const int64_t ntile = B * ((N + TN - 1) / TN);
    return 4 * ntile * C * TN + (int64_t)C * C + ntile * 4 * C + B * 4 * C + (int64_t)WG_SLICES * 2 * C * C;
}

int head_cond_fwd_launch(const float* x, const float* a, const float* w0, const float* b0, const float* w2,
                         const float* b2, const float* gamma, const float* beta, int64_t B, int64_t N, float* y,
                         hipStream_t s) {
    if (!x || !a || !w0 || !b0 || !w2 || !b2 || !gamma || !beta || !y || bad_shape(B, N)) return -1;
    if (((uintptr_t)w0 | (uintptr_t)w2) & 15) return -1;
    const dim3 grid((unsigned)((N + TN - 1) / TN), (unsigned)B);
    KScope ks(s);
    if (ks.on()) ks.begin("head_cond_fwd_kernel", 4.0 * B * N * C * C, 2.0 * B * N * C * 4);
    hipLaunchKernelGGL(head_cond_fwd_kernel, grid, dim3(NTH), 0, s, x, a, w0, b0, w2, b2, gamma, beta, N,
                       (int)(vec_ok(x, N) && vec_ok(y, N)), y);
    return (int)hipGetLastError();
}

int head_cond_bwd_launch(const float* gy, const float* x, const float* a, const float* w0, const float* b0,
                         const float* w2, const float* b2, const float* gamma, int64_t B, int64_t N, float* gw0,
                         float* gb0, float* gw2, float* gb2, float* ggamma, float* gbeta, float* ga, float* ws,
                         hipStream_t s) {
    if (!gy || !x || !a || !w0 || !b0 || !w2 || !b2 || !gamma || !gw0 || !gb0 || !gw2 || !gb2 || !ggamma || !gbeta ||
        !ga || !ws || bad_shape(B, N))
        return -1;
    if (((uintptr_t)w0 | (uintptr_t)w2 | (uintptr_t)gw0 | (uintptr_t)gw2 | (uintptr_t)ws) & 15) return -1;
    const int tpi = (int)((N + TN - 1) / TN);
    const int64_t ntile = B * tpi, blk = ntile * C * TN;
    float* ublk = ws;
    float* gblk = ublk + blk;
    float* dvblk = gblk + blk;
    float* dhblk = dvblk + blk;
    float* w2t = dhblk + blk;
    float* part = w2t + C * C;
    float* item = part + ntile * 4 * C;
    float* wpart = item + B * 4 * C;
    hipLaunchKernelGGL(head_cond_transpose_kernel, dim3(C / 32, C / 32), dim3(256), 0, s, w2, w2t);
    {
        KScope ks(s);
        if (ks.on()) ks.begin("head_cond_bwd_kernel", 6.0 * B * N * C * C, 6.0 * B * N * C * 4);
        hipLaunchKernelGGL(head_cond_bwd_kernel, dim3((unsigned)tpi, (unsigned)B), dim3(NTH), 0, s, gy, x, a, w0, b0, w2,
                           b2, gamma, w2t, N, (int)(vec_ok(x, N) && vec_ok(gy, N)), ublk, gblk, dvblk, dhblk, part);
    }
    {
        KScope ks(s);
        if (ks.on()) ks.begin("head_cond_wgrad_kernel", 4.0 * ntile * TN * C * C, 4.0 * blk * 4);
        hipLaunchKernelGGL(head_cond_wgrad_kernel, dim3(9, 2, WG_SLICES), dim3(256), 0, s, ublk, gblk, dvblk, dhblk,
                           ntile, wpart);
    }
    hipLaunchKernelGGL(head_cond_wsum_kernel, dim3(2 * C * C / 4 / 256), dim3(256), 0, s, wpart, gw2, gw0);
    hipLaunchKernelGGL(head_cond_item_kernel, dim3((unsigned)B, 4), dim3(C), 0, s, part, tpi, item);
    hipLaunchKernelGGL(head_cond_vec_kernel, dim3((unsigned)(B + 1)), dim3(C), 0, s, item, w0, B, ggamma, gbeta, gb2, gb0,
                       ga);
    return (int)hipGetLastError();
}

}  // namespace athd
