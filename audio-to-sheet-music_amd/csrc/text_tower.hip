// CLAP text tower kernels (gfx950): RoBERTa-base on P x L <= tens of rows is weight-streaming bound, so the GEMM here is
// not the library's big-tile family but a skinny one that spreads the WEIGHTS over the whole chip.
//
//   tt_gemm_kernel    part[s] = X[:, slice s] . W[:, slice s]^T.  Workgroup = one 16-row slab of W x one split-K slice;
//                     its W waves split the slice again.  Weights are the MFMA A operand: each lane loads its 16-byte
//                     fragments of W[n0 + (lane & 15)][...] straight from global memory into registers, all of them
//                     before the first use (the wave's whole share is 4 .. 32 VGPRs), and they are read once.  X goes
//                     through LDS one 16-row tile at a time (zero rows past M), converted to bf16 there in bf16 mode.
//                     The waves' accumulators are added in wave order through LDS and the slice is stored; slices are
//                     added in slice order by the consumer (tt_reduce / tt_ln / tt_attn / tt_final).  No atomics, and
//                     the order depends on (N, K) only.
//   tt_embed_kernel, tt_ln_kernel   one wave per 768-wide row, fp32, two-pass variance.
//   tt_attn_kernel    one workgroup per (prompt, head); q, k, v of the head in LDS in fp32 (L <= 128); VALU.
//   tt_reduce_kernel, tt_final_kernel   the element-wise epilogues.
#include "common.h"
#include "text_tower.h"

namespace athd {

static const TtGemmPlan kPlans[] = {
    {2304, 768, 2, 4, 96},    // packed q, k, v            288 workgroups
    {768, 768, 6, 4, 32},     // attention output          288
    {3072, 768, 2, 4, 96},    // FFN in                    384
    {768, 3072, 6, 4, 128},   // FFN out                   288
    {512, 768, 8, 3, 32},     // projection linear1        256
    {512, 512, 8, 2, 32},     // projection linear2        256
};

const TtGemmPlan* tt_gemm_plan(int N, int K) {
    for (const TtGemmPlan& p : kPlans)
        if (p.N == N && p.K == K) return &p;
    return nullptr;
}

// ------------------------------------------------------------------------------------------------------- GEMM
constexpr int TT_G_MAXKC = 512;                              // largest slice (FFN out: 4 waves x 128)
constexpr int TT_G_XBYTES = 16 * (TT_G_MAXKC + 4) * 4;       // X tile, f32 rows padded by 4 floats (bf16: by 8 halves)
constexpr int TT_G_LDS = TT_G_XBYTES + 4 * 256 * 4;          // + the waves' 16x16 accumulators

template <bool BF16, int KW>
__global__ __launch_bounds__(256) void tt_gemm_kernel(const void* __restrict__ Wp, const float* __restrict__ X,
                                                      int64_t ldx, int M, int N, int K, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[TT_G_LDS];
    const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slabs = N >> 4;
    const int slab = blockIdx.x % slabs, s = blockIdx.x / slabs;
    const int Kc = KW * nw;
    const int n0 = slab * 16, kc0 = s * Kc, kw0 = wave * KW;
    const int mb0 = blockIdx.y * 64;
    const int r16 = lane & 15, q4 = lane >> 4;
    float* red = reinterpret_cast<float*>(lds + TT_G_XBYTES);

    // the wave's share of the slab: every load is issued here, ahead of the first tile's staging
    bf16x8_t wb[BF16 ? KW / 32 : 1];
    float4 wf[BF16 ? 1 : KW / 16];
    if constexpr (BF16) {
        const bf16_t* wrow = reinterpret_cast<const bf16_t*>(Wp) + (int64_t)(n0 + r16) * K + kc0 + kw0 + 8 * q4;
#pragma unroll
        for (int i = 0; i < KW / 32; ++i) wb[i] = *reinterpret_cast<const bf16x8_t*>(wrow + 32 * i);
    } else {
        const float* wrow = reinterpret_cast<const float*>(Wp) + (int64_t)(n0 + r16) * K + kc0 + kw0 + 4 * q4;
#pragma unroll
        for (int i = 0; i < KW / 16; ++i) wf[i] = *reinterpret_cast<const float4*>(wrow + 16 * i);
    }

    const int kc4 = Kc >> 2;
    for (int mt = 0; mt < 4; ++mt) {
        const int m0 = mb0 + mt * 16;
        if (m0 >= M) break;                                   // uniform over the workgroup
        // stage X[m0 .. m0+15][kc0 .. kc0+Kc) (rows past M as zeros)
        // 16 * kc4 float4 over 64 * nw threads = KW / 16 per thread; all loads are issued before the first LDS write
        float4 xg[KW / 16];
#pragma unroll
        for (int j = 0; j < KW / 16; ++j) {
            const int i = threadIdx.x + j * blockDim.x;
            const int r = i / kc4, c4 = i - r * kc4;
            xg[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m0 + r < M) xg[j] = *reinterpret_cast<const float4*>(X + (int64_t)(m0 + r) * ldx + kc0 + c4 * 4);
        }
#pragma unroll
        for (int j = 0; j < KW / 16; ++j) {
            const int i = threadIdx.x + j * blockDim.x;
            const int r = i / kc4, c4 = i - r * kc4;
            const float4 v = xg[j];
            if constexpr (BF16) {
                uint2 h;
                h.x = pack2bf(v.x, v.y);
                h.y = pack2bf(v.z, v.w);
                *reinterpret_cast<uint2*>(lds + ((size_t)r * (Kc + 8) + c4 * 4) * 2) = h;
            } else {
                *reinterpret_cast<float4*>(lds + ((size_t)r * (Kc + 4) + c4 * 4) * 4) = v;
            }
        }
        __syncthreads();
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BF16) {
            const unsigned char* xr = lds + ((size_t)r16 * (Kc + 8) + kw0 + 8 * q4) * 2;
#pragma unroll
            for (int i = 0; i < KW / 32; ++i) {
                const bf16x8_t xb = *reinterpret_cast<const bf16x8_t*>(xr + 64 * i);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[i], xb, acc, 0, 0, 0);
            }
        } else {
            const unsigned char* xr = lds + ((size_t)r16 * (Kc + 4) + kw0 + 4 * q4) * 4;
#pragma unroll
            for (int i = 0; i < KW / 16; ++i) {
                const float4 xv = *reinterpret_cast<const float4*>(xr + 64 * i);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i].x, xv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i].y, xv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i].z, xv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i].w, xv.w, acc, 0, 0, 0);
            }
        }
        // D[row n = 4 q4 + r][col m = r16] -> red[wave][m][n]
        *reinterpret_cast<float4*>(red + wave * 256 + r16 * 16 + q4 * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        __syncthreads();
        for (int i = threadIdx.x; i < 256; i += blockDim.x) {
            float v = red[i];
            for (int w = 1; w < nw; ++w) v += red[w * 256 + i];
            const int m = m0 + (i >> 4);
            if (m < M) part[((int64_t)s * M + m) * N + n0 + (i & 15)] = v;
        }
        // (the next tile's staging barrier orders these reads of red before its next writes)
    }
}

template <bool BF16>
static int gemm_launch_t(const void* W, const float* X, int64_t ldx, int M, const TtGemmPlan& p, float* part,
                         hipStream_t st) {
    const dim3 grid((unsigned)((p.N / 16) * p.S), (unsigned)((M + 63) / 64));
    const dim3 block((unsigned)(64 * p.W));
    switch (p.KW) {
        case 32: tt_gemm_kernel<BF16, 32><<<grid, block, 0, st>>>(W, X, ldx, M, p.N, p.K, part); break;
        case 96: tt_gemm_kernel<BF16, 96><<<grid, block, 0, st>>>(W, X, ldx, M, p.N, p.K, part); break;
        case 128: tt_gemm_kernel<BF16, 128><<<grid, block, 0, st>>>(W, X, ldx, M, p.N, p.K, part); break;
        default: return -1;
    }
    return (int)hipGetLastError();
}

int tt_gemm_launch(bool bf16, const void* W, const float* X, int64_t ldx, int M, const TtGemmPlan& p, float* part,
                   hipStream_t st) {
    if (M <= 0 || p.K != p.S * p.W * p.KW || p.W < 1 || p.W > 4 || p.W * p.KW > TT_G_MAXKC || (p.N & 15) || (ldx & 3))
        return -1;
    return bf16 ? gemm_launch_t<true>(W, X, ldx, M, p, part, st) : gemm_launch_t<false>(W, X, ldx, M, p, part, st);
}

// --------------------------------------------------------------------------------------------------- epilogues
ATHD_DEV float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// sum_s p[s * stride], s ascending: every slice's load is issued before the first addition (S is uniform, so the
// guards are scalar branches); one load per iteration would chain S L2 latencies
constexpr int TT_MAX_S = 8;
ATHD_DEV float4 sum_slices(const float* __restrict__ p, int S, int64_t stride) {
    float4 v[TT_MAX_S];
#pragma unroll
    for (int s = 0; s < TT_MAX_S; ++s)
        if (s < S) v[s] = *reinterpret_cast<const float4*>(p + s * stride);
    float4 a = v[0];
#pragma unroll
    for (int s = 1; s < TT_MAX_S; ++s)
        if (s < S) a = add4(a, v[s]);
    return a;
}
ATHD_DEV float tt_act(float v, int act) {
    switch (act) {
        case TT_GELU: return gelu_erf(v);
        case TT_TANH: return tanhf(v);
        case TT_RELU: return fmaxf(v, 0.f);
        default: return v;
    }
}

__global__ __launch_bounds__(256) void tt_reduce_kernel(const float* __restrict__ part, int S, int M, int N,
                                                        const float* __restrict__ bias, const float* __restrict__ res,
                                                        int64_t ldr, int act, float* __restrict__ out, int64_t ldo) {
    const int n4 = N >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * n4) return;
    const int m = (int)(i / n4), c = (int)(i - (int64_t)m * n4) * 4;
    float4 v = sum_slices(part + (int64_t)m * N + c, S, (int64_t)M * N);
    if (bias) v = add4(v, *reinterpret_cast<const float4*>(bias + c));
    if (res) v = add4(v, *reinterpret_cast<const float4*>(res + (int64_t)m * ldr + c));
    v = make_float4(tt_act(v.x, act), tt_act(v.y, act), tt_act(v.z, act), tt_act(v.w, act));
    *reinterpret_cast<float4*>(out + (int64_t)m * ldo + c) = v;
}

int tt_reduce_launch(const float* part, int S, int M, int N, const float* bias, const float* res, int64_t ldr, int act,
                     float* out, int64_t ldo, hipStream_t st) {
    if (S < 1 || S > TT_MAX_S || M <= 0 || N <= 0 || (N & 3) || (ldo & 3) || (res && (ldr & 3))) return -1;
    const int64_t n = (int64_t)M * (N / 4);
    tt_reduce_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(part, S, M, N, bias, res, ldr, act, out, ldo);
    return (int)hipGetLastError();
}

// LayerNorm of a 768-wide row held as 3 float4 per lane (columns 256 c + 4 lane ..), two-pass variance
ATHD_DEV void ln768_store(float4 (&v)[3], const float* __restrict__ w, const float* __restrict__ b,
                          float* __restrict__ out, int lane) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) sum += (v[c].x + v[c].y) + (v[c].z + v[c].w);
    const float mean = wave_sum(sum) * (1.0f / TT_H);
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c].x -= mean; v[c].y -= mean; v[c].z -= mean; v[c].w -= mean;
        sq += (v[c].x * v[c].x + v[c].y * v[c].y) + (v[c].z * v[c].z + v[c].w * v[c].w);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) * (1.0f / TT_H) + TT_LN_EPS);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int col = 256 * c + 4 * lane;
        const float4 g = *reinterpret_cast<const float4*>(w + col), o = *reinterpret_cast<const float4*>(b + col);
        *reinterpret_cast<float4*>(out + col) = make_float4(v[c].x * rstd * g.x + o.x, v[c].y * rstd * g.y + o.y,
                                                            v[c].z * rstd * g.z + o.z, v[c].w * rstd * g.w + o.w);
    }
}

__global__ __launch_bounds__(256) void tt_ln_kernel(const float* __restrict__ part, int S, int M,
                                                    const float* __restrict__ bias, const float* res,
                                                    const float* __restrict__ w, const float* __restrict__ b,
                                                    float* out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float4 v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int col = 256 * c + 4 * lane;
        float4 a = sum_slices(part + (int64_t)row * TT_H + col, S, (int64_t)M * TT_H);
        a = add4(a, *reinterpret_cast<const float4*>(bias + col));
        v[c] = add4(a, *reinterpret_cast<const float4*>(res + (int64_t)row * TT_H + col));
    }
    ln768_store(v, w, b, out + (int64_t)row * TT_H, lane);     // the row's res was read above: out may alias res
}

int tt_ln_launch(const float* part, int S, int M, const float* bias, const float* res, const float* w, const float* b,
                 float* out, hipStream_t st) {
    if (S < 1 || S > TT_MAX_S || M <= 0) return -1;
    tt_ln_kernel<<<dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st>>>(part, S, M, bias, res, w, b, out);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void tt_embed_kernel(const int32_t* __restrict__ ids, int M, int L,
                                                       const float* __restrict__ word, const float* __restrict__ type0,
                                                       const float* __restrict__ pos, const float* __restrict__ w,
                                                       const float* __restrict__ b, float* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int p = row / L, t = row - p * L;
    int cnt = 0;
    for (int j = lane; j <= t; j += 64) cnt += ids[p * L + j] != TT_PAD;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    const int id = ids[row];
    const int ps = id != TT_PAD ? cnt + 1 : TT_PAD;            // <= L + 1 <= 129 < 514
    const int idc = min(max(id, 0), TT_VOCAB - 1);             // an id outside the table is clamped into it
    float4 v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int col = 256 * c + 4 * lane;
        const float4 e = add4(*reinterpret_cast<const float4*>(word + (int64_t)idc * TT_H + col),
                              *reinterpret_cast<const float4*>(type0 + col));
        v[c] = add4(e, *reinterpret_cast<const float4*>(pos + (int64_t)ps * TT_H + col));
    }
    ln768_store(v, w, b, x + (int64_t)row * TT_H, lane);
}

int tt_embed_launch(const int32_t* ids, int P, int L, const float* word, const float* type0, const float* pos,
                    const float* w, const float* b, float* x, hipStream_t st) {
    if (P <= 0 || L <= 0 || L > TT_MAX_L) return -1;
    const int M = P * L;
    tt_embed_kernel<<<dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st>>>(ids, M, L, word, type0, pos, w, b, x);
    return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------------- attention
// LDS floats: Q [L][64], K [L][65] (a lane per key reads down a column: the pad spreads the banks), V [L][64],
// probabilities [4 waves][128]
static size_t attn_lds_bytes(int L) { return ((size_t)L * (64 + 65 + 64) + 4 * 128) * sizeof(float); }

__global__ __launch_bounds__(256) void tt_attn_kernel(const float* __restrict__ part, int S,
                                                      const float* __restrict__ bias, const int32_t* __restrict__ mask,
                                                      int M, int L, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Ks = Qs + L * 64;
    float* Vs = Ks + L * 65;
    float* Pr = Vs + L * 64;
    const int p = blockIdx.x / TT_HEADS, h = blockIdx.x - p * TT_HEADS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NQKV = 3 * TT_H;
    for (int i = threadIdx.x; i < L * 16; i += 256) {
        const int t = i >> 4, c4 = (i & 15) * 4;
        const int64_t row = (int64_t)p * L + t;
        float4 qkv[3];
#pragma unroll
        for (int which = 0; which < 3; ++which) {
            const int col = which * TT_H + h * TT_DH + c4;
            const float4 a = sum_slices(part + row * NQKV + col, S, (int64_t)M * NQKV);
            qkv[which] = add4(a, *reinterpret_cast<const float4*>(bias + col));
        }
        *reinterpret_cast<float4*>(Qs + t * 64 + c4) = qkv[0];
        Ks[t * 65 + c4 + 0] = qkv[1].x; Ks[t * 65 + c4 + 1] = qkv[1].y;
        Ks[t * 65 + c4 + 2] = qkv[1].z; Ks[t * 65 + c4 + 3] = qkv[1].w;
        *reinterpret_cast<float4*>(Vs + t * 64 + c4) = qkv[2];
    }
    __syncthreads();
    const int j0 = lane, j1 = lane + 64;
    const bool in0 = j0 < L, in1 = j1 < L;
    const bool keep0 = in0 && mask[p * L + (in0 ? j0 : 0)] != 0;
    const bool keep1 = in1 && mask[p * L + (in1 ? j1 : 0)] != 0;
    const float* k0 = Ks + (in0 ? j0 : 0) * 65;
    const float* k1 = Ks + (in1 ? j1 : 0) * 65;
    float* pr = Pr + wave * 128;
    for (int i0 = 0; i0 < L; i0 += 4) {                        // the same trip count in every wave (barriers inside)
        const int i = i0 + wave;
        const bool active = i < L;
        const float* q = Qs + (active ? i : 0) * 64;
        float a0 = 0.f, a1 = 0.f;
        for (int d = 0; d < 64; ++d) {
            const float qd = q[d];
            a0 = fmaf(qd, k0[d], a0);
            a1 = fmaf(qd, k1[d], a1);
        }
        a0 *= 0.125f;
        a1 *= 0.125f;
        const float mx = wave_max(fmaxf(keep0 ? a0 : -INFINITY, keep1 ? a1 : -INFINITY));
        const float e0 = keep0 ? expf(a0 - mx) : 0.f, e1 = keep1 ? expf(a1 - mx) : 0.f;
        const float den = wave_sum(e0 + e1);
        pr[lane] = den > 0.f ? e0 / den : 0.f;                 // (a prompt whose mask is all zero: zeros, no NaN)
        pr[lane + 64] = den > 0.f ? e1 / den : 0.f;
        __syncthreads();
        float o = 0.f;
        for (int j = 0; j < L; ++j) o = fmaf(pr[j], Vs[j * 64 + lane], o);
        if (active) out[((int64_t)p * L + i) * TT_H + h * TT_DH + lane] = o;
        __syncthreads();
    }
}

int tt_init() {
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&tt_attn_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_lds_bytes(TT_MAX_L));
}

int tt_attn_launch(const float* qkv_part, int S, const float* bias, const int32_t* mask, int P, int L, float* out,
                   hipStream_t st) {
    if (S < 1 || S > TT_MAX_S || P <= 0 || L <= 0 || L > TT_MAX_L) return -1;
    tt_attn_kernel<<<dim3((unsigned)(P * TT_HEADS)), dim3(256), attn_lds_bytes(L), st>>>(qkv_part, S, bias, mask, P * L, L,
                                                                                      out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------- final
__global__ __launch_bounds__(256) void tt_final_kernel(const float* __restrict__ part, int S, int P,
                                                       const float* __restrict__ bias, int normalize,
                                                       float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= P) return;
    float4 v[2];
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = 256 * c + 4 * lane;
        const float4 a = sum_slices(part + (int64_t)row * TT_PROJ + col, S, (int64_t)P * TT_PROJ);
        v[c] = add4(a, *reinterpret_cast<const float4*>(bias + col));
        sq += (v[c].x * v[c].x + v[c].y * v[c].y) + (v[c].z * v[c].z + v[c].w * v[c].w);
    }
    float nrm = 1.0f;
    if (normalize) nrm = fmaxf(sqrtf(wave_sum(sq)), 1e-12f);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = 256 * c + 4 * lane;
        float4 r = v[c];
        if (normalize) r = make_float4(r.x / nrm, r.y / nrm, r.z / nrm, r.w / nrm);
        *reinterpret_cast<float4*>(out + (int64_t)row * TT_PROJ + col) = r;
    }
}

int tt_final_launch(const float* part, int S, int P, const float* bias, int normalize, float* out, hipStream_t st) {
    if (S < 1 || S > TT_MAX_S || P <= 0) return -1;
    tt_final_kernel<<<dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st>>>(part, S, P, bias, normalize, out);
    return (int)hipGetLastError();
}

}  // namespace athd
