// Head training's decoder level (gfx950), both directions, from raw f32 weights (ATHTDemucs_v2.py:61-139; include/athd.h
// `athd_head_dec_level*`).  One level = ConvTranspose (k 8, s 4, p 2) along one axis of a channel-first
// slab, GroupNorm(1) + GELU (levels 0..2), a linear resize of that axis and the scaled skip.  The frequency decoder is
// the operation with `inner` = Ts contiguous columns per position, the time decoder with inner = 1.
//
// Per item, x (Ci, M, inner), tokens n = m inner + t:
//   c[co, 4 g - 2 + k1] = b[co] + sum_ci W[ci, co, k1] x[ci, g] + W[ci, co, k1 + 4] x[ci, g - 1],  g in [0, M], k1 in [0, 4)
// is a GEMM with rows (k1, co), K = (tap, ci) and columns (g, t): the second tap's operand sits `inner` tokens back, and
// the bounds test on g - tap keeps a tile from reading across the item's start or end.  The data gradient
//   dx[ci, m] = sum_{k, co} W[ci, co, k] dc[co, 4 m - 2 + k]
// has rows ci, K = (k, co), columns (m, t); the weight gradient
//   dW[ci, (co, k)] = sum_{b, m, t} x[ci, m, t] dc[co, 4 m - 2 + k, t]
// has K = the tokens of all items, split into a FIXED number of slices per level whose results are summed in slice
// order.  All three run in one tiled kernel (64 x 128 outputs per workgroup of four waves, K steps of 16 through LDS,
// the next step's operands loaded while the MFMAs of this one run) on v_mfma_f32_16x16x4_f32, an exact k-ordered f32 fma
// chain; the operands are gathered with scalar loads, so any 4-byte alignment, inner and Lt work.  Level 3 (Co = 4) runs
// the same kernel for its forward and its weight gradient: the tiles are mostly padding, but the level is
// bandwidth-bound either way and no second code path has to be kept.  Its data gradient (32 products per output) is a
// plain kernel that sums in double: see head_dec_dx3_kernel.
//
// Everything between the GEMMs is elementwise on the pre-norm tensor c and one gradient tensor of its size, both in the
// caller's workspace: the statistics (two passes: the mean, then the centred squares), the output (norm, GELU, resize,
// skip), the adjoint of the resize as a GATHER per source position, gelu', and the GroupNorm backward.
//
// Determinism.  No atomics.  Sums over positions are written per block (fixed tree inside the block) and merged in block
// order, then item order.  Every output element is written exactly once, none is accumulated into or read.
#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "prof.h"

namespace athd {

namespace {

constexpr int TM = 64, TC = 128, TK = 16, NTH = 256;   // workgroup tile rows x columns, K step, threads
constexpr int LSA = TM + 4, LSB = TC + 4;              // LDS row strides: the four k groups of an MFMA hit disjoint banks
constexpr int CHS = 8192;                              // elements per block of the statistics passes
constexpr int CHG = 1024;                              // positions per block of the gradient passes
constexpr int DEC_CI[4] = {384, 192, 96, 48}, DEC_CO[4] = {192, 96, 48, 4};
constexpr int DW_SLICES[4] = {8, 16, 32, 64};          // split-K slices of the weight gradient, fixed per level

struct Dims {
    int Ci, Co;
    int64_t M, inner, N, P;                            // N = M inner tokens, P = 4 M inner positions per channel
};

// ------------------------------------------------------------------------------------------------ the tiled GEMM
// Op: kbegin / kend (the K range of this workgroup), init (per-thread constants), load (one K step's share of both
// operand tiles into registers, zeros outside the problem), put (those registers into LDS as As[k][row], Bs[k][col]),
// store (one output element).
template <class Op>
__global__ __launch_bounds__(NTH) void head_dec_gemm_kernel(Op op) {
    __shared__ float As[TK * LSA];
    __shared__ float Bs[TK * LSB];
    const int tid = threadIdx.x, wave = tid >> 6, r16 = tid & 15, q4 = (tid >> 4) & 3;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 64;
    typename Op::St st;
    op.init(st, tid);
    f32x4_t acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float ra[4], rb[8];
    const int64_t k0 = op.kbegin(), k1 = op.kend();
    if (k0 < k1) op.load(st, k0, ra, rb);
    for (int64_t k = k0; k < k1; k += TK) {
        op.put(st, ra, rb, As, Bs);
        __syncthreads();
        if (k + TK < k1) op.load(st, k + TK, ra, rb);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kl = 4 * q4 + s;
            float a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[kl * LSA + wr + i * 16 + r16];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[kl * LSB + wc + j * 16 + r16];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                op.store(st, (int)blockIdx.y * TM + wr + i * 16 + 4 * q4 + r, (int)blockIdx.x * TC + wc + j * 16 + r16,
                         acc[i][j][r]);
}

// operands owned by column (token): a thread keeps one column of B and one row of A and walks k
ATHD_DEV void put_by_column(int tid, const float (&ra)[4], const float (&rb)[8], float* As, float* Bs) {
#pragma unroll
    for (int j = 0; j < 4; ++j) As[((tid >> 6) + 4 * j) * LSA + (tid & 63)] = ra[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) Bs[((tid >> 7) + 2 * j) * LSB + (tid & 127)] = rb[j];
}

// c = ConvT(x) + bias.  grid (column tiles over (M + 1) inner, row tiles over 4 Co, B)
struct FwdOp {
    const float *x, *w, *bias;
    float* c;
    Dims d;
    struct St {
        int64_t xoff, woff;   // x: item base + column; w: co * 8 + k1
        int g;                // the column's position group
        bool cv, rv;
        int tid;
    };
    ATHD_DEV int64_t kbegin() const { return 0; }
    ATHD_DEV int64_t kend() const { return 2 * d.Ci; }
    ATHD_DEV void init(St& s, int tid) const {
        s.tid = tid;
        const int64_t col = (int64_t)blockIdx.x * TC + (tid & 127);
        s.cv = col < (d.M + 1) * d.inner;
        s.g = (int)(col / d.inner);
        s.xoff = (int64_t)blockIdx.z * d.Ci * d.N + col;
        const int row = (int)blockIdx.y * TM + (tid & 63);
        s.rv = row < 4 * d.Co;
        const int k1 = row / d.Co;
        s.woff = (int64_t)(row - k1 * d.Co) * 8 + k1;
    }
    ATHD_DEV void load(const St& s, int64_t k, float (&ra)[4], float (&rb)[8]) const {
        const int tap = k >= d.Ci ? 1 : 0;              // Ci is a multiple of TK: one tap per K step
        const int ci0 = (int)k - tap * d.Ci;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ci = ci0 + (s.tid >> 6) + 4 * j;
            ra[j] = s.rv ? w[(int64_t)ci * d.Co * 8 + s.woff + 4 * tap] : 0.f;
        }
        const int m = s.g - tap;
        const bool ok = s.cv && m >= 0 && m < d.M;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ci = ci0 + (s.tid >> 7) + 2 * j;
            rb[j] = ok ? x[s.xoff + (int64_t)ci * d.N - (int64_t)tap * d.inner] : 0.f;
        }
    }
    ATHD_DEV void put(const St& s, const float (&ra)[4], const float (&rb)[8], float* As, float* Bs) const {
        put_by_column(s.tid, ra, rb, As, Bs);
    }
    ATHD_DEV void store(const St&, int row, int col, float v) const {
        if (row >= 4 * d.Co || col >= (d.M + 1) * d.inner) return;
        const int k1 = row / d.Co, co = row - k1 * d.Co;
        const int g = (int)(col / d.inner), t = (int)(col - g * d.inner);
        const int64_t o = 4 * (int64_t)g - 2 + k1;
        if (o < 0 || o >= 4 * d.M) return;
        c[((int64_t)blockIdx.z * d.Co + co) * d.P + o * d.inner + t] = v + bias[co];
    }
};

// dx = W . dc.  grid (column tiles over M inner, row tiles over Ci, B)
struct DxOp {
    const float *dc, *w;
    float* dx;
    Dims d;
    struct St {
        int64_t doff;         // dc: item base + t
        int64_t m;
        bool cv, rv;
        int row, tid;
    };
    ATHD_DEV int64_t kbegin() const { return 0; }
    ATHD_DEV int64_t kend() const { return 8 * d.Co; }
    ATHD_DEV void init(St& s, int tid) const {
        s.tid = tid;
        const int64_t col = (int64_t)blockIdx.x * TC + (tid & 127);
        s.cv = col < d.N;
        s.m = col / d.inner;
        s.doff = (int64_t)blockIdx.z * d.Co * d.P + (col - s.m * d.inner);
        s.row = (int)blockIdx.y * TM + (tid & 63);
        s.rv = s.row < d.Ci;
    }
    ATHD_DEV void load(const St& s, int64_t k, float (&ra)[4], float (&rb)[8]) const {
        const int k8 = (int)k / d.Co;                   // Co is a multiple of TK (levels 0..2): one tap per K step
        const int co0 = (int)k - k8 * d.Co;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + (s.tid >> 6) + 4 * j;
            ra[j] = s.rv ? w[((int64_t)s.row * d.Co + co) * 8 + k8] : 0.f;
        }
        const int64_t o = 4 * s.m - 2 + k8;
        const bool ok = s.cv && o >= 0 && o < 4 * d.M;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int co = co0 + (s.tid >> 7) + 2 * j;
            rb[j] = ok ? dc[s.doff + (int64_t)co * d.P + o * d.inner] : 0.f;
        }
    }
    ATHD_DEV void put(const St& s, const float (&ra)[4], const float (&rb)[8], float* As, float* Bs) const {
        put_by_column(s.tid, ra, rb, As, Bs);
    }
    ATHD_DEV void store(const St&, int row, int col, float v) const {
        if (row >= d.Ci || col >= d.N) return;
        dx[((int64_t)blockIdx.z * d.Ci + row) * d.N + col] = v;
    }
};

// wpart[slice] = x . dc^T over the slice's tokens.  grid (column tiles over 8 Co, row tiles over Ci, slices); a thread
// keeps one token of the K step and walks the rows and columns, so the token's (b, m, t) is decoded once per step
struct DwOp {
    const float *x, *dc;
    float* wpart;
    Dims d;
    int64_t KT, per;          // B N tokens in all, tokens per slice (a multiple of TK)
    struct St {
        int tid;
    };
    ATHD_DEV int64_t kbegin() const { return (int64_t)blockIdx.z * per; }
    ATHD_DEV int64_t kend() const {
        const int64_t e = ((int64_t)blockIdx.z + 1) * per;
        return e < KT ? e : KT;
    }
    ATHD_DEV void init(St& s, int tid) const { s.tid = tid; }
    ATHD_DEV void load(const St& s, int64_t k, float (&ra)[4], float (&rb)[8]) const {
        const int64_t kk = k + (s.tid & 15);
        const bool ok = kk < kend();
        const int64_t b = ok ? kk / d.N : 0;
        const int64_t n = ok ? kk - b * d.N : 0;
        const int64_t m = n / d.inner, t = n - m * d.inner;
        const int r0 = s.tid >> 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ci = (int)blockIdx.y * TM + r0 + 16 * j;
            ra[j] = (ok && ci < d.Ci) ? x[(b * d.Ci + ci) * d.N + n] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int jj = (int)blockIdx.x * TC + r0 + 16 * j;
            const int64_t o = 4 * m - 2 + (jj & 7);
            rb[j] = (ok && jj < 8 * d.Co && o >= 0 && o < 4 * d.M)
                        ? dc[(b * d.Co + (jj >> 3)) * d.P + o * d.inner + t]
                        : 0.f;
        }
    }
    ATHD_DEV void put(const St& s, const float (&ra)[4], const float (&rb)[8], float* As, float* Bs) const {
        const int kl = s.tid & 15, r0 = s.tid >> 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) As[kl * LSA + r0 + 16 * j] = ra[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[kl * LSB + r0 + 16 * j] = rb[j];
    }
    ATHD_DEV void store(const St&, int row, int col, float v) const {
        if (row >= d.Ci || col >= 8 * d.Co) return;
        wpart[((int64_t)blockIdx.z * d.Ci + row) * (8 * d.Co) + col] = v;
    }
};

// Level 3's data gradient (Ci = 48, Co = 4: 32 products per output), a plain kernel: one thread per token keeps its 32
// values of dc and forms the 48 sums in double, rounded once.  torch's own kernel for this shape is exact to the final
// rounding on this GPU (4e-8 of the largest value against float64), which an f32 chain of 32 does not stay within four
// times of.  grid (blocks of 256 tokens, B)
__global__ __launch_bounds__(256) void head_dec_dx3_kernel(const float* __restrict__ dc, const float* __restrict__ w,
                                                           Dims d, float* __restrict__ dx) {
    __shared__ float ws[48 * 32];
    for (int i = threadIdx.x; i < 48 * 32; i += 256) ws[i] = w[i];
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= d.N) return;
    const int64_t b = blockIdx.y, m = n / d.inner, t = n - m * d.inner;
    double v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int64_t o = 4 * m - 2 + (j & 7);
        v[j] = (o >= 0 && o < 4 * d.M) ? (double)dc[(b * 4 + (j >> 3)) * d.P + o * d.inner + t] : 0.0;
    }
    for (int ci = 0; ci < 48; ++ci) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 32; ++j) s = fma((double)ws[ci * 32 + j], v[j], s);
        dx[(b * 48 + ci) * d.N + n] = (float)s;
    }
}

// gw = the slices of wpart summed in slice order
__global__ __launch_bounds__(256) void head_dec_wsum_kernel(const float* __restrict__ wpart, int64_t E, int slices,
                                                            float* __restrict__ gw) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float v = wpart[e];
    for (int s = 1; s < slices; ++s) v += wpart[(int64_t)s * E + e];
    gw[e] = v;
}

// ------------------------------------------------------------------------------------------------ block sums
// the block's 256 values summed by a fixed tree; the total is returned to thread 0 (sh: 256 floats; ends on a barrier)
ATHD_DEV float block_sum(float v, float* sh, int tid) {
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// part[b][block] = the block's CHS elements of item b's c: sum of c (mr == nullptr) or of (c - mu)^2
__global__ __launch_bounds__(256) void head_dec_sum_kernel(const float* __restrict__ c, int64_t n,
                                                           const float* __restrict__ mr, float* __restrict__ part) {
    __shared__ float sh[256];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y, base = (int64_t)blockIdx.x * CHS;
    const float mu = mr ? mr[2 * b] : 0.f;
    float s = 0.f;
    for (int j = 0; j < CHS / 256; ++j) {
        const int64_t i = base + j * 256 + tid;
        if (i < n) {
            const float v = c[b * n + i];
            if (mr) {
                const float dv = v - mu;
                s = fmaf(dv, dv, s);
            } else {
                s += v;
            }
        }
    }
    s = block_sum(s, sh, tid);
    if (tid == 0) part[b * gridDim.x + blockIdx.x] = s;
}

// the item's blocks in order -> mode 0: mr[b][0] = mean; mode 1: mr[b][1] = 1 / sqrt(var + 1e-5), and stats[b] = mr[b]
__global__ __launch_bounds__(256) void head_dec_stat_kernel(const float* __restrict__ part, int nch, int64_t n, int mode,
                                                            float* __restrict__ mr, float* __restrict__ stats) {
    __shared__ float sh[256];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    float s = 0.f;
    for (int i = tid; i < nch; i += 256) s += part[b * nch + i];
    s = block_sum(s, sh, tid);
    if (tid != 0) return;
    if (mode == 0) {
        mr[2 * b] = s / (float)n;
    } else {
        const float r = 1.0f / sqrtf(s / (float)n + 1e-5f);
        mr[2 * b + 1] = r;
        stats[2 * b] = mr[2 * b];
        stats[2 * b + 1] = r;
    }
}

// ------------------------------------------------------------------------------------------------ resize
// torch's linear rule with align_corners = False, in its own f32 arithmetic
struct Lin {
    int i0, i1;
    float w0, w1;
};
ATHD_DEV Lin lin_src(int64_t l, float scale, int64_t in_len) {
    float src = scale * ((float)l + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    int64_t i0 = (int64_t)src;
    if (i0 > in_len - 1) i0 = in_len - 1;
    Lin r;
    r.i0 = (int)i0;
    r.i1 = (int)(i0 < in_len - 1 ? i0 + 1 : i0);
    r.w1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    r.w0 = 1.0f - r.w1;
    return r;
}

ATHD_DEV float gelu_cdf(float z) { return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)); }

// y = resize(h) + 0.1 resize(skip), h = gelu(gamma (c - mu) r + beta) or c.  grid (blocks over Lt inner, Co, B)
template <bool NORM>
__global__ __launch_bounds__(256) void head_dec_out_kernel(const float* __restrict__ c, const float* __restrict__ mr,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ skip, Dims d, int64_t Lt, int64_t S,
                                                           float* __restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Lt * d.inner) return;
    const int64_t l = idx / d.inner, t = idx - l * d.inner;
    const int co = blockIdx.y;
    const int64_t bc = (int64_t)blockIdx.z * d.Co + co;
    const Lin a = lin_src(l, (float)(4 * d.M) / (float)Lt, 4 * d.M);
    const float* cc = c + bc * d.P + t;
    float h0 = cc[(int64_t)a.i0 * d.inner], h1 = cc[(int64_t)a.i1 * d.inner];
    if constexpr (NORM) {
        const float mu = mr[2 * blockIdx.z], r = mr[2 * blockIdx.z + 1], g = gamma[co], be = beta[co];
        const float z0 = fmaf(g, (h0 - mu) * r, be), z1 = fmaf(g, (h1 - mu) * r, be);
        h0 = z0 * gelu_cdf(z0);
        h1 = z1 * gelu_cdf(z1);
    }
    float v = a.w0 * h0 + a.w1 * h1;
    if (skip) {
        const Lin s = lin_src(l, (float)S / (float)Lt, S);
        const float* sk = skip + bc * S * d.inner + t;
        v += 0.1f * (s.w0 * sk[(int64_t)s.i0 * d.inner] + s.w1 * sk[(int64_t)s.i1 * d.inner]);
    }
    y[bc * Lt * d.inner + idx] = v;
}

// The adjoint of the resize as a gather: source position o collects every l whose i0 or i1 is o, in ascending l.  The
// candidates come from inverting the rule in double with a margin for the rule's own f32 rounding; each is tested with
// the forward's exact arithmetic.  Then gelu' and gamma (NORM): g = gamma dz, part = {sum dz ch, sum dz} per block;
// without the norm g = dc and part[1] = sum dc.  grid (blocks of CHG positions, Co, B)
template <bool NORM>
__global__ __launch_bounds__(256) void head_dec_grad_kernel(const float* __restrict__ gy, const float* __restrict__ c,
                                                            const float* __restrict__ mr,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, Dims d, int64_t Lt,
                                                            float* __restrict__ g, float* __restrict__ part) {
    __shared__ float sh[256];
    const int tid = threadIdx.x, co = blockIdx.y;
    const int64_t bc = (int64_t)blockIdx.z * d.Co + co, L4 = 4 * d.M;
    const float scale = (float)L4 / (float)Lt;
    const double inv = (double)Lt / (double)L4;
    const int64_t mg = 2 + (Lt >> 20);
    float mu = 0.f, r = 0.f, ga = 0.f, be = 0.f;
    if constexpr (NORM) mu = mr[2 * blockIdx.z], r = mr[2 * blockIdx.z + 1], ga = gamma[co], be = beta[co];
    float p0 = 0.f, p1 = 0.f;
    for (int j = 0; j < CHG / 256; ++j) {
        const int64_t idx = (int64_t)blockIdx.x * CHG + j * 256 + tid;
        if (idx >= d.P) continue;
        const int64_t o = idx / d.inner, t = idx - o * d.inner;
        int64_t lo = (int64_t)floor(((double)o - 0.5) * inv - 0.5) - mg;
        int64_t hi = (int64_t)ceil(((double)o + 1.5) * inv - 0.5) + mg;
        if (lo < 0) lo = 0;
        if (hi > Lt - 1) hi = Lt - 1;
        const float* gp = gy + bc * Lt * d.inner + t;
        float acc = 0.f;
        for (int64_t l = lo; l <= hi; ++l) {
            const Lin a = lin_src(l, scale, L4);
            const float wgt = (a.i0 == o ? a.w0 : 0.f) + (a.i1 == o ? a.w1 : 0.f);
            if (a.i0 == o || a.i1 == o) acc = fmaf(gp[l * d.inner], wgt, acc);
        }
        if constexpr (NORM) {
            const float ch = (c[bc * d.P + idx] - mu) * r;
            const float z = fmaf(ga, ch, be);
            const float dz = acc * (gelu_cdf(z) + z * (0.39894228040143267794f * expf(-0.5f * z * z)));
            g[bc * d.P + idx] = ga * dz;
            p0 = fmaf(dz, ch, p0);
            p1 += dz;
        } else {
            g[bc * d.P + idx] = acc;
            p1 += acc;
        }
    }
    p0 = block_sum(p0, sh, tid);
    p1 = block_sum(p1, sh, tid);
    if (tid == 0) {
        float* o = part + (bc * gridDim.x + blockIdx.x) * 2;
        o[0] = p0;
        o[1] = p1;
    }
}

// item[b][co] = {sum dz ch, sum dz} over the channel's blocks in order; m12[b] = {mean D, mean D ch} over the item,
// D = gamma dz, the channels in order.  grid B, 256 threads (Co <= 192)
__global__ __launch_bounds__(256) void head_dec_gmerge_kernel(const float* __restrict__ part, int nch, int Co,
                                                              const float* __restrict__ gamma, int64_t n,
                                                              float* __restrict__ item, float* __restrict__ m12) {
    __shared__ float sh[2][256];
    const int co = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (co < Co) {
        const float* p = part + (b * Co + co) * (int64_t)nch * 2;
        float s0 = 0.f, s1 = 0.f;
        for (int i = 0; i < nch; ++i) s0 += p[2 * i], s1 += p[2 * i + 1];
        item[(b * Co + co) * 2] = s0;
        item[(b * Co + co) * 2 + 1] = s1;
        sh[0][co] = gamma[co] * s0;
        sh[1][co] = gamma[co] * s1;
    }
    __syncthreads();
    if (co == 0) {
        float a0 = 0.f, a1 = 0.f;
        for (int i = 0; i < Co; ++i) a0 += sh[0][i], a1 += sh[1][i];
        m12[2 * b] = a1 / (float)n;
        m12[2 * b + 1] = a0 / (float)n;
    }
}

// g <- dc = r (g - mean D - ch mean(D ch)) in place (each element read and written by one thread); bpart = sum dc per
// block.  grid as head_dec_grad_kernel
__global__ __launch_bounds__(256) void head_dec_dc_kernel(const float* __restrict__ c, const float* __restrict__ mr,
                                                          const float* __restrict__ m12, Dims d, float* __restrict__ g,
                                                          float* __restrict__ bpart) {
    __shared__ float sh[256];
    const int tid = threadIdx.x;
    const int64_t bc = (int64_t)blockIdx.z * d.Co + blockIdx.y;
    const float mu = mr[2 * blockIdx.z], r = mr[2 * blockIdx.z + 1];
    const float m1 = m12[2 * blockIdx.z], m2 = m12[2 * blockIdx.z + 1];
    float p = 0.f;
    for (int j = 0; j < CHG / 256; ++j) {
        const int64_t idx = (int64_t)blockIdx.x * CHG + j * 256 + tid;
        if (idx >= d.P) continue;
        const float ch = (c[bc * d.P + idx] - mu) * r;
        const float v = r * (g[bc * d.P + idx] - m1 - ch * m2);
        g[bc * d.P + idx] = v;
        p += v;
    }
    p = block_sum(p, sh, tid);
    if (tid == 0) bpart[bc * gridDim.x + blockIdx.x] = p;
}

// gb[co] = the items in order of (the channel's blocks in order of bpart[.. * bstride + boff]); ggamma, gbeta = the
// items of `item` in order (NORM levels).  One block, 256 threads
__global__ __launch_bounds__(256) void head_dec_vec_kernel(const float* __restrict__ bpart, int bstride, int boff,
                                                           int nch, int Co, int64_t B, const float* __restrict__ item,
                                                           float* __restrict__ gb, float* __restrict__ ggamma,
                                                           float* __restrict__ gbeta) {
    const int co = threadIdx.x;
    if (co >= Co) return;
    float tb = 0.f, tg = 0.f, te = 0.f;
    for (int64_t b = 0; b < B; ++b) {
        const float* p = bpart + (b * Co + co) * (int64_t)nch * bstride + boff;
        float s = 0.f;
        for (int i = 0; i < nch; ++i) s += p[(int64_t)i * bstride];
        tb = b ? tb + s : s;
        if (item) {
            tg = b ? tg + item[(b * Co + co) * 2] : item[(b * Co + co) * 2];
            te = b ? te + item[(b * Co + co) * 2 + 1] : item[(b * Co + co) * 2 + 1];
        }
    }
    gb[co] = tb;
    if (item) {
        ggamma[co] = tg;
        gbeta[co] = te;
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool bad_shape(int level, int64_t B, int64_t M, int64_t inner, int64_t Lt) {
    return level < 0 || level > 3 || B < 1 || B > 65535 || M < 1 || M > HEAD_DEC_MAX_M || inner < 1 ||
           inner > HEAD_DEC_MAX_INNER || Lt < 1 || Lt > HEAD_DEC_MAX_LT || M * inner > HEAD_DEC_MAX_TOKENS ||
           Lt * inner > 4 * HEAD_DEC_MAX_TOKENS;
}

int64_t up4(int64_t n) { return (n + 3) & ~(int64_t)3; }

struct Plan {                                           // float offsets into the workspace
    Dims d;
    int nchs, nchg, slices;
    int64_t c, g, spart, mr, gpart, item, m12, bpart, wpart, total;
};

Plan plan(int level, int64_t B, int64_t M, int64_t inner) {
    Plan p;
    p.d = Dims{DEC_CI[level], DEC_CO[level], M, inner, M * inner, 4 * M * inner};
    const int64_t n = p.d.Co * p.d.P;                   // elements of c per item
    p.nchs = (int)((n + CHS - 1) / CHS);
    p.nchg = (int)((p.d.P + CHG - 1) / CHG);
    p.slices = DW_SLICES[level];
    int64_t o = 0;
    p.c = o, o += up4(B * n);
    p.g = o, o += up4(B * n);
    p.spart = o, o += up4(B * p.nchs);
    p.mr = o, o += up4(B * 2);
    p.gpart = o, o += up4(B * p.d.Co * p.nchg * 2);
    p.item = o, o += up4(B * p.d.Co * 2);
    p.m12 = o, o += up4(B * 2);
    p.bpart = o, o += up4(B * p.d.Co * p.nchg);
    p.wpart = o, o += up4((int64_t)p.slices * p.d.Ci * p.d.Co * 8);
    p.total = o;
    return p;
}

// a launch inside the context's profile window (prof.h), labelled with its algorithmic bytes
#define DEC_LAUNCH(label, bytes, ...)                   \
    do {                                                \
        KScope ks_(s);                                  \
        if (ks_.on()) ks_.begin(label, 0.0, bytes);     \
        hipLaunchKernelGGL(__VA_ARGS__);                \
    } while (0)

template <class Op>
void launch_gemm(const char* name, const Op& op, int64_t cols, int rows, unsigned z, double flops, double bytes,
                 hipStream_t s) {
    KScope ks(s);
    if (ks.on()) ks.begin(name, flops, bytes);
    hipLaunchKernelGGL(head_dec_gemm_kernel<Op>, dim3((unsigned)((cols + TC - 1) / TC), (unsigned)((rows + TM - 1) / TM), z),
                       dim3(NTH), 0, s, op);
}

void launch_conv(const Plan& p, const float* x, const float* w, const float* bias, float* c, int64_t B, hipStream_t s) {
    const Dims& d = p.d;
    launch_gemm("head_dec_gemm_kernel<fwd>", FwdOp{x, w, bias, c, d}, (d.M + 1) * d.inner, 4 * d.Co, (unsigned)B,
                16.0 * B * d.N * d.Ci * d.Co, 4.0 * B * (d.Ci * d.N + d.Co * d.P), s);
}

}  // namespace

int64_t head_dec_ws_floats(int level, int64_t B, int64_t M, int64_t inner, int64_t Lt) {
    if (bad_shape(level, B, M, inner, Lt)) return 0;
    return plan(level, B, M, inner).total;
}

int head_dec_fwd_launch(int level, const float* x, const float* w, const float* bias, const float* gamma,
                        const float* beta, const float* skip, int64_t B, int64_t M, int64_t inner, int64_t S, int64_t Lt,
                        float* y, float* stats, float* ws, hipStream_t s) {
    if (bad_shape(level, B, M, inner, Lt) || !x || !w || !bias || !y || !ws) return -1;
    const bool norm = level < 3;
    if (norm && (!gamma || !beta || !stats)) return -1;
    if ((skip == nullptr) != (S == 0) || S < 0 || S > HEAD_DEC_MAX_LT || S * inner > 4 * HEAD_DEC_MAX_TOKENS) return -1;
    const Plan p = plan(level, B, M, inner);
    const Dims& d = p.d;
    const int64_t n = d.Co * d.P;
    float* c = ws + p.c;
    launch_conv(p, x, w, bias, c, B, s);
    const dim3 og((unsigned)((Lt * inner + 255) / 256), (unsigned)d.Co, (unsigned)B);
    const double obytes = 4.0 * B * d.Co * (3.0 * Lt * inner + 2.0 * (skip ? Lt * inner : 0));
    if (norm) {
        float* spart = ws + p.spart;
        float* mr = ws + p.mr;
        for (int mode = 0; mode < 2; ++mode) {
            DEC_LAUNCH("head_dec_sum_kernel", 4.0 * B * n, head_dec_sum_kernel, dim3((unsigned)p.nchs, (unsigned)B),
                       dim3(256), 0, s, c, n, mode ? mr : nullptr, spart);
            hipLaunchKernelGGL(head_dec_stat_kernel, dim3((unsigned)B), dim3(256), 0, s, spart, p.nchs, n, mode, mr,
                               stats);
        }
        DEC_LAUNCH("head_dec_out_kernel", obytes, head_dec_out_kernel<true>, og, dim3(256), 0, s, c, mr, gamma, beta, skip,
                   d, Lt, S, y);
    } else {
        DEC_LAUNCH("head_dec_out_kernel", obytes, head_dec_out_kernel<false>, og, dim3(256), 0, s, c, nullptr, nullptr,
                   nullptr, skip, d, Lt, S, y);
    }
    return (int)hipGetLastError();
}

int head_dec_bwd_launch(int level, const float* gy, const float* x, const float* w, const float* bias,
                        const float* gamma, const float* beta, const float* stats, int64_t B, int64_t M, int64_t inner,
                        int64_t Lt, float* gx, float* gw, float* gb, float* ggamma, float* gbeta, float* ws,
                        hipStream_t s) {
    if (bad_shape(level, B, M, inner, Lt) || !gy || !x || !w || !bias || !gx || !gw || !gb || !ws) return -1;
    const bool norm = level < 3;
    if (norm && (!gamma || !beta || !stats || !ggamma || !gbeta)) return -1;
    const Plan p = plan(level, B, M, inner);
    const Dims& d = p.d;
    const int64_t n = d.Co * d.P;
    float* c = ws + p.c;
    float* g = ws + p.g;
    float* gpart = ws + p.gpart;
    const dim3 gg((unsigned)p.nchg, (unsigned)d.Co, (unsigned)B);
    const double gbytes = 4.0 * B * (2.0 * n + (double)d.Co * Lt * inner);
    if (norm) {
        launch_conv(p, x, w, bias, c, B, s);            // the forward's c again: nothing but x and stats was kept
        DEC_LAUNCH("head_dec_grad_kernel", gbytes, head_dec_grad_kernel<true>, gg, dim3(256), 0, s, gy, c, stats, gamma,
                   beta, d, Lt, g, gpart);
        hipLaunchKernelGGL(head_dec_gmerge_kernel, dim3((unsigned)B), dim3(256), 0, s, gpart, p.nchg, d.Co, gamma, n,
                           ws + p.item, ws + p.m12);
        DEC_LAUNCH("head_dec_dc_kernel", 12.0 * B * n, head_dec_dc_kernel, gg, dim3(256), 0, s, c, stats, ws + p.m12, d, g,
                   ws + p.bpart);
        hipLaunchKernelGGL(head_dec_vec_kernel, dim3(1), dim3(256), 0, s, ws + p.bpart, 1, 0, p.nchg, d.Co, B,
                           ws + p.item, gb, ggamma, gbeta);
    } else {
        DEC_LAUNCH("head_dec_grad_kernel", gbytes, head_dec_grad_kernel<false>, gg, dim3(256), 0, s, gy, nullptr, nullptr,
                   nullptr, nullptr, d, Lt, g, gpart);
        hipLaunchKernelGGL(head_dec_vec_kernel, dim3(1), dim3(256), 0, s, gpart, 2, 1, p.nchg, d.Co, B, nullptr, gb,
                           nullptr, nullptr);
    }
    const double gflops = 16.0 * B * d.N * d.Ci * d.Co, mbytes = 4.0 * B * (d.Ci * d.N + d.Co * d.P);
    if (norm) {
        launch_gemm("head_dec_gemm_kernel<dx>", DxOp{g, w, gx, d}, d.N, d.Ci, (unsigned)B, gflops, mbytes, s);
    } else {
        KScope ks(s);
        if (ks.on()) ks.begin("head_dec_dx3_kernel", gflops, mbytes);
        hipLaunchKernelGGL(head_dec_dx3_kernel, dim3((unsigned)((d.N + 255) / 256), (unsigned)B), dim3(256), 0, s, g, w, d,
                           gx);
    }
    const int64_t KT = B * d.N;
    const int64_t per = ((KT + p.slices - 1) / p.slices + TK - 1) / TK * TK;
    launch_gemm("head_dec_gemm_kernel<dw>", DwOp{x, g, ws + p.wpart, d, KT, per}, 8 * d.Co, d.Ci, (unsigned)p.slices,
                gflops, mbytes, s);
    const int64_t E = (int64_t)d.Ci * d.Co * 8;
    hipLaunchKernelGGL(head_dec_wsum_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, ws + p.wpart, E, p.slices,
                       gw);
    return (int)hipGetLastError();
}

}  // namespace athd
