// Validation level: the row metrics of src/loss.py (sdr_loss :9-30, sisdr_loss :33-68, new_sdr_metric :71-87, the L1 of
// combined_L1_sdr_loss :150) for every row of a batch in one call, and the dataset segments of
// src/dataloader.py:104-121 (random_segments = False) taken on the device.  Training ends (further down): the gradient
// of the two combined losses with respect to est from the same sums, and the random / augmented segments of
// src/dataloader.py:86-134.
//
// loss_rows: a pure streaming reduction, 8 * rows * n bytes per sweep, two sweeps.
//   sweep 1  sum t^2, sum (t-e)^2, sum |t-e|, sum e, sum t           -> SDR, new-SDR, L1 and the row means
//   sweep 2  sum (e-me)(t-mt), sum (t-mt)^2, sum (e-me)^2             -> SI-SDR, centred with the means of sweep 1
// (raw moments in one sweep would cancel n mean^2 against the raw sums on a DC offset).  All sums in fp64.
// A row is cut into chunks of LR_CHUNK elements; block (row, b) of a sweep takes chunks b, b + nb, ... and writes ONE
// partial sum per quantity to the scratch; a second kernel adds a row's nb partials in ascending b.  No atomics: the
// table is the same bits on every run with the same pointers.  Rows are folded into gridDim.x (rows * nb blocks).
// Loads are 16 bytes wide where the row's base allows it: a scalar head up to the first 16-byte boundary of the est
// row, float4 groups, a scalar tail.  When the target row does not reach a boundary at the same element (the two
// pointers differ mod 16) the same groups are read with scalar loads.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace athd {

constexpr int LR_THREADS = 256;
constexpr int64_t LR_CHUNK = 16384;              // elements per chunk: 16 float4 per thread and array
constexpr int64_t LR_GROUPS = LR_CHUNK / 4;      // float4 groups per chunk
constexpr int64_t LR_MAX_NB = 1024;              // blocks per row

constexpr int64_t LR_MAX_GRID = (int64_t)1 << 23;   // blocks of 256 threads: a grid dimension stays below 2^32 threads

static int64_t lr_blocks_per_row(int64_t rows, int64_t n) {
    const int64_t want = std::max<int64_t>((n / 4 + LR_GROUPS - 1) / LR_GROUPS, 1);
    return std::min<int64_t>(want, std::min<int64_t>(LR_MAX_NB, std::max<int64_t>(LR_MAX_GRID / rows, 1)));
}

// Split of one row: elements [0, head) scalar, [head, head + 4 * groups) in groups of 4, the rest scalar.
struct RowSplit {
    int64_t head, groups, tail0;
    bool vec;
};
ATHD_DEV RowSplit row_split(const float* e, const float* t, int64_t n) {
    RowSplit s;
    const int64_t mis = (int64_t)(((uintptr_t)e >> 2) & 3);
    s.head = ((4 - mis) & 3) < n ? ((4 - mis) & 3) : n;
    s.groups = (n - s.head) / 4;
    s.tail0 = s.head + 4 * s.groups;
    s.vec = (((uintptr_t)(t + s.head)) & 15) == 0;
    return s;
}

ATHD_DEV void load4(const float* p, bool vec, float (&v)[4]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}

// K per-thread sums -> one partial per quantity: waves by shuffles, the 4 waves in ascending order.
template <int K>
ATHD_DEV void block_store(double (&acc)[K], double* __restrict__ dst) {
    __shared__ double sh[4 * K];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum_d(acc[k]);
        if ((threadIdx.x & 63) == 0) sh[w * K + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) dst[threadIdx.x] = ((sh[threadIdx.x] + sh[K + threadIdx.x]) + sh[2 * K + threadIdx.x]) +
                                            sh[3 * K + threadIdx.x];
}

// PASS 0: acc = { sum t^2, sum (t-e)^2, sum |t-e|, sum e, sum t };  PASS 1: acc = { <e,t>, |t|^2, |e|^2 } centred.
template <int PASS>
ATHD_DEV void accumulate(double (&acc)[PASS ? 3 : 5], float ef, float tf, double me, double mt) {
    if constexpr (PASS == 0) {
        const double e = ef, t = tf, d = t - e;
        acc[0] += t * t;
        acc[1] += d * d;
        acc[2] += fabs(d);
        acc[3] += e;
        acc[4] += t;
    } else {
        const double e = (double)ef - me, t = (double)tf - mt;
        acc[0] += e * t;
        acc[1] += t * t;
        acc[2] += e * e;
    }
}

// grid: rows * nb blocks; block i = (row i / nb, b = i % nb).  part: [rows][nb][K].  rowsum (PASS 1): [rows][5].
template <int PASS>
__global__ __launch_bounds__(LR_THREADS) void loss_rows_sweep_kernel(const float* __restrict__ est,
                                                                     const float* __restrict__ tgt, int64_t n, int nb,
                                                                     const double* __restrict__ rowsum,
                                                                     double* __restrict__ part) {
    constexpr int K = PASS ? 3 : 5;
    const int64_t r = (int64_t)blockIdx.x / nb;
    const int b = (int)((int64_t)blockIdx.x % nb);
    const float* e = est + r * n;
    const float* t = tgt + r * n;
    const RowSplit sp = row_split(e, t, n);
    double me = 0.0, mt = 0.0;
    if constexpr (PASS == 1) {
        me = rowsum[5 * r + 3] / (double)n;
        mt = rowsum[5 * r + 4] / (double)n;
    }
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const float* eg = e + sp.head;
    const float* tg = t + sp.head;
    for (int64_t c = b; c * LR_GROUPS < sp.groups; c += nb) {
        const int64_t g1 = (c + 1) * LR_GROUPS < sp.groups ? (c + 1) * LR_GROUPS : sp.groups;
#pragma unroll 4
        for (int64_t g = c * LR_GROUPS + threadIdx.x; g < g1; g += LR_THREADS) {
            float ev[4], tv[4];
            load4(eg + 4 * g, sp.vec, ev);
            load4(tg + 4 * g, sp.vec, tv);
#pragma unroll
            for (int j = 0; j < 4; ++j) accumulate<PASS>(acc, ev[j], tv[j], me, mt);
        }
    }
    if (b == 0) {      // the row's scalar head and tail: at most 3 + 3 elements (all of a row shorter than 4)
        const int64_t i = threadIdx.x < sp.head ? (int64_t)threadIdx.x : sp.tail0 + ((int64_t)threadIdx.x - sp.head);
        if (i < n) accumulate<PASS>(acc, e[i], t[i], me, mt);
    }
    block_store<K>(acc, part + ((int64_t)r * nb + b) * K);
}

// one thread per row: the nb partials of sweep 1 in ascending order -> rowsum [rows][5]
__global__ __launch_bounds__(LR_THREADS) void loss_rows_rowsum_kernel(const double* __restrict__ part, int64_t rows,
                                                                      int nb, double* __restrict__ rowsum) {
    const int64_t r = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
    if (r >= rows) return;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nb; ++b)
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += part[(r * nb + b) * 5 + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) rowsum[5 * r + k] = s[k];
}

ATHD_DEV double clamp30(double v) { return v < -30.0 ? -30.0 : (v > 30.0 ? 30.0 : v); }

// one thread per row: the nb partials of sweep 2 in ascending order, then the four metrics
__global__ __launch_bounds__(LR_THREADS) void loss_rows_final_kernel(const double* __restrict__ rowsum,
                                                                     const double* __restrict__ part2, int64_t rows,
                                                                     int64_t n, int nb, double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
    if (r >= rows) return;
    double et = 0.0, tt = 0.0, ee = 0.0;
    for (int b = 0; b < nb; ++b) {
        et += part2[(r * nb + b) * 3];
        tt += part2[(r * nb + b) * 3 + 1];
        ee += part2[(r * nb + b) * 3 + 2];
    }
    const double raw = 10.0 * log10((rowsum[5 * r] + 1e-8) / (rowsum[5 * r + 1] + 1e-8));
    const double al = et / (tt + 1e-8);
    const double st = al * al * tt;
    double en = ee - 2.0 * al * et + al * al * tt;
    en = en < 0.0 ? 0.0 : en;
    out[4 * r] = clamp30(raw);
    out[4 * r + 1] = clamp30(10.0 * log10((st + 1e-8) / (en + 1e-8)));
    out[4 * r + 2] = raw;
    out[4 * r + 3] = rowsum[5 * r + 2] / (double)n;
}

static bool loss_rows_shape_ok(int64_t rows, int64_t n) {
    return rows >= 1 && rows <= ((int64_t)1 << 20) && n >= 1 && n < ((int64_t)1 << 31);
}

// doubles: sweep-1 partials [rows][nb][5], row sums [rows][5], sweep-2 partials [rows][nb][3]
size_t loss_rows_scratch_bytes(int64_t rows, int64_t n) {
    if (!loss_rows_shape_ok(rows, n)) return 0;
    const int64_t nb = lr_blocks_per_row(rows, n);
    return (size_t)(rows * nb * 8 + rows * 5) * sizeof(double);
}

int loss_rows_launch(const float* est, const float* tgt, int64_t rows, int64_t n, void* scratch, double* out,
                     hipStream_t s) {
    if (!est || !tgt || !scratch || !out || !loss_rows_shape_ok(rows, n)) return -1;
    if (((uintptr_t)est & 3) || ((uintptr_t)tgt & 3) || ((uintptr_t)scratch & 7) || ((uintptr_t)out & 7)) return -1;
    const int nb = (int)lr_blocks_per_row(rows, n);
    double* part1 = (double*)scratch;
    double* rowsum = part1 + rows * nb * 5;
    double* part2 = rowsum + rows * 5;
    const unsigned grid = (unsigned)(rows * nb);                  // <= LR_MAX_GRID
    const unsigned rgrid = (unsigned)((rows + LR_THREADS - 1) / LR_THREADS);
    hipLaunchKernelGGL(loss_rows_sweep_kernel<0>, dim3(grid), dim3(LR_THREADS), 0, s, est, tgt, n, nb,
                       (const double*)nullptr, part1);
    hipLaunchKernelGGL(loss_rows_rowsum_kernel, dim3(rgrid), dim3(LR_THREADS), 0, s, part1, rows, nb, rowsum);
    hipLaunchKernelGGL(loss_rows_sweep_kernel<1>, dim3(grid), dim3(LR_THREADS), 0, s, est, tgt, n, nb, rowsum, part2);
    hipLaunchKernelGGL(loss_rows_final_kernel, dim3(rgrid), dim3(LR_THREADS), 0, s, rowsum, part2, rows, n, nb, out);
    return (int)hipGetLastError();
}

// ---- loss gradients: d total / d est for total = -(w_sdr mean sdr + w_si mean sisdr) + w_l1 mean |e - t| (the two
//      combined losses of src/loss.py:90-162; the clamps pass the gradient on the closed interval, as torch.clamp).
//      coef: the table by the four launches above (so its bits are those of loss_rows), then one thread per row turns
//      the row's sums into GC_STRIDE doubles.  apply: grad_i = cs (e_i - t_i) + cp (e_i - me) + cq (t_i - mt) +
//      cl sign(e_i - t_i), the four scalars from the row's coefficients, the weights, 1 / rows and the upstream
//      gradient; fp64 per element, rounded once.  The centring adds no mean term: sum (e - me) = sum (t - mt) = 0.
constexpr int GC_STRIDE = 8;   // { a_sdr, p, q, gate_sdr, gate_si, mean e, mean t, 0 } (include/athd.h)
constexpr double K_DB = 4.342944819032518;   // 10 / ln 10

// The SDR gate reads the unclamped column of the table.  The SI-SDR column is clamped: a value strictly inside
// +-30 is an open gate; at exactly +-30 the unclamped value (the expressions of loss_rows_final_kernel on the same
// sums) decides between "on the boundary" (open) and "beyond it" (closed).
__global__ __launch_bounds__(LR_THREADS) void loss_grad_coef_kernel(const double* __restrict__ rowsum,
                                                                    const double* __restrict__ part2,
                                                                    const double* __restrict__ table, int64_t rows,
                                                                    int64_t n, int nb, double* __restrict__ coef) {
    const int64_t r = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
    if (r >= rows) return;
    double et = 0.0, tt = 0.0, ee = 0.0;
    for (int b = 0; b < nb; ++b) {
        et += part2[(r * nb + b) * 3];
        tt += part2[(r * nb + b) * 3 + 1];
        ee += part2[(r * nb + b) * 3 + 2];
    }
    const double al = et / (tt + 1e-8);
    const double st = al * al * tt;
    double en = ee - 2.0 * al * et + al * al * tt;
    en = en < 0.0 ? 0.0 : en;
    const double raw = table[4 * r + 2], sic = table[4 * r + 1];
    const double siu = 10.0 * log10((st + 1e-8) / (en + 1e-8));
    const bool g1 = raw >= -30.0 && raw <= 30.0;
    const bool g2 = fabs(sic) < 30.0 || (siu >= -30.0 && siu <= 30.0);
    const double c = et * 1e-8 / (tt + 1e-8);
    double* o = coef + GC_STRIDE * r;
    o[0] = 2.0 * K_DB / (rowsum[5 * r + 1] + 1e-8);
    o[1] = -2.0 * K_DB / (en + 1e-8);
    o[2] = K_DB * (2.0 * al * tt / ((tt + 1e-8) * (st + 1e-8)) + 2.0 * al / (en + 1e-8) +
                   2.0 * c / ((tt + 1e-8) * (en + 1e-8)));
    o[3] = g1 ? 1.0 : 0.0;
    o[4] = g2 ? 1.0 : 0.0;
    o[5] = rowsum[5 * r + 3] / (double)n;
    o[6] = rowsum[5 * r + 4] / (double)n;
    o[7] = 0.0;
}

struct GradScalars {
    double cs, cp, cq, cl, me, mt;
    bool zero;
};

ATHD_DEV float grad_value(const GradScalars& k, float ef, float tf) {
    if (k.zero) return 0.f;
    const double e = ef, t = tf, d = e - t;
    const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    return (float)(k.cs * d + k.cp * (e - k.me) + k.cq * (t - k.mt) + k.cl * sg);
}

// grid: rows * nb blocks as in the sweeps; 12 bytes per element.  16-byte accesses need est, target and grad rows to
// reach a boundary at the same element.
__global__ __launch_bounds__(LR_THREADS) void loss_grad_apply_kernel(const float* __restrict__ est,
                                                                     const float* __restrict__ tgt, int64_t rows,
                                                                     int64_t n, int nb, const double* __restrict__ coef,
                                                                     double w_sdr, double w_si, double w_l1,
                                                                     const float* __restrict__ upstream,
                                                                     float* __restrict__ grad) {
    const int64_t r = (int64_t)blockIdx.x / nb;
    const int b = (int)((int64_t)blockIdx.x % nb);
    const float* e = est + r * n;
    const float* t = tgt + r * n;
    float* o = grad + r * n;
    RowSplit sp = row_split(e, t, n);
    sp.vec = sp.vec && (((uintptr_t)(o + sp.head)) & 15) == 0;
    const double* c = coef + GC_STRIDE * r;
    const double up = upstream ? (double)*upstream : 1.0;
    const double inv_rows = 1.0 / (double)rows;
    GradScalars k;
    k.cs = c[3] != 0.0 ? up * w_sdr * c[0] * inv_rows : 0.0;
    k.cp = c[4] != 0.0 ? -(up * w_si * c[1] * inv_rows) : 0.0;
    k.cq = c[4] != 0.0 ? -(up * w_si * c[2] * inv_rows) : 0.0;
    k.cl = up * w_l1 / ((double)rows * (double)n);
    k.me = c[5];
    k.mt = c[6];
    k.zero = k.cs == 0.0 && k.cp == 0.0 && k.cq == 0.0 && k.cl == 0.0;
    const float* eg = e + sp.head;
    const float* tg = t + sp.head;
    float* og = o + sp.head;
    for (int64_t ch = b; ch * LR_GROUPS < sp.groups; ch += nb) {
        const int64_t g1 = (ch + 1) * LR_GROUPS < sp.groups ? (ch + 1) * LR_GROUPS : sp.groups;
#pragma unroll 4
        for (int64_t g = ch * LR_GROUPS + threadIdx.x; g < g1; g += LR_THREADS) {
            float ev[4], tv[4], gv[4];
            load4(eg + 4 * g, sp.vec, ev);
            load4(tg + 4 * g, sp.vec, tv);
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = grad_value(k, ev[j], tv[j]);
            if (sp.vec) {
                *reinterpret_cast<float4*>(og + 4 * g) = make_float4(gv[0], gv[1], gv[2], gv[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) og[4 * g + j] = gv[j];
            }
        }
    }
    if (b == 0) {      // the row's scalar head and tail, as in the sweeps
        const int64_t i = threadIdx.x < sp.head ? (int64_t)threadIdx.x : sp.tail0 + ((int64_t)threadIdx.x - sp.head);
        if (i < n) o[i] = grad_value(k, e[i], t[i]);
    }
}

int loss_grad_coef_launch(const float* est, const float* tgt, int64_t rows, int64_t n, void* scratch, double* table,
                          double* coef, hipStream_t s) {
    if (!coef || ((uintptr_t)coef & 7)) return -1;
    const int rc = loss_rows_launch(est, tgt, rows, n, scratch, table, s);
    if (rc != 0) return rc;
    const int nb = (int)lr_blocks_per_row(rows, n);
    const double* rowsum = (const double*)scratch + rows * nb * 5;
    const double* part2 = rowsum + rows * 5;
    hipLaunchKernelGGL(loss_grad_coef_kernel, dim3((unsigned)((rows + LR_THREADS - 1) / LR_THREADS)), dim3(LR_THREADS),
                       0, s, rowsum, part2, (const double*)table, rows, n, nb, coef);
    return (int)hipGetLastError();
}

int loss_grad_apply_launch(const float* est, const float* tgt, int64_t rows, int64_t n, const double* coef,
                           double w_sdr, double w_si, double w_l1, const float* upstream, float* grad, hipStream_t s) {
    if (!est || !tgt || !coef || !grad || !loss_rows_shape_ok(rows, n)) return -1;
    if (((uintptr_t)est & 3) || ((uintptr_t)tgt & 3) || ((uintptr_t)grad & 3) || ((uintptr_t)upstream & 3) ||
        ((uintptr_t)coef & 7))
        return -1;
    const int nb = (int)lr_blocks_per_row(rows, n);
    hipLaunchKernelGGL(loss_grad_apply_kernel, dim3((unsigned)(rows * nb)), dim3(LR_THREADS), 0, s, est, tgt, rows, n,
                       nb, coef, w_sdr, w_si, w_l1, upstream, grad);
    return (int)hipGetLastError();
}

// ---- dataset segments: out (rows, 2, S) channel-major from stems (n_src, length, 2) frame-interleaved.  Tile
//      (row, x) of rows * ceil(S / 256), tiles strided over the grid: thread j reads frame seg * S + j of source src (one 8-byte load where the
//      base allows it) and stores its two channels, each a coalesced 4-byte store.  A frame beyond `length`, a source
//      outside [0, n_src) and a negative segment give zeros; nothing outside `stems` is read.
__global__ __launch_bounds__(256) void gather_segments_kernel(const float* __restrict__ stems, int n_src, int64_t length,
                                                              const int32_t* __restrict__ src,
                                                              const int64_t* __restrict__ seg, int64_t S, int64_t bx,
                                                              int64_t tiles, int vec, float* __restrict__ out) {
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r = tile / bx;
    const int64_t j = (tile % bx) * 256 + threadIdx.x;
    if (j >= S) continue;
    const int sr = src[r];
    const int64_t sg = seg[r];
    float a = 0.f, b = 0.f;
    if (sr >= 0 && sr < n_src && sg >= 0 && sg <= length / S) {
        const int64_t pos = sg * S + j;
        if (pos < length) {
            const float* p = stems + ((int64_t)sr * length + pos) * 2;
            if (vec) {
                const float2 q = *reinterpret_cast<const float2*>(p);
                a = q.x; b = q.y;
            } else {
                a = p[0]; b = p[1];
            }
        }
    }
    out[(r * 2) * S + j] = a;
    out[(r * 2 + 1) * S + j] = b;
  }
}

int gather_segments_launch(const float* stems, int n_src, int64_t length, const int32_t* src, const int64_t* seg,
                           int64_t rows, int64_t S, float* out, hipStream_t s) {
    if (!stems || !src || !seg || !out || n_src <= 0 || length <= 0 || rows <= 0 || S <= 0) return -1;
    if (((uintptr_t)stems & 3) || ((uintptr_t)out & 3) || ((uintptr_t)src & 3) || ((uintptr_t)seg & 7)) return -1;
    const int64_t bx = (S + 255) / 256;
    if (bx > INT64_MAX / rows) return -1;
    const int64_t tiles = rows * bx;
    hipLaunchKernelGGL(gather_segments_kernel, dim3((unsigned)std::min<int64_t>(tiles, LR_MAX_GRID)), dim3(256), 0, s,
                       stems, n_src, length, src, seg, S, bx, tiles, (int)(((uintptr_t)stems & 7) == 0), out);
    return (int)hipGetLastError();
}

// ---- training segments (src/dataloader.py:86-134 on the device): the same tiles, but row r starts at any sample
//      start[r], every sample is (float)((double)x * gain[r]) (the reference multiplies stempeg's float64 array and
//      rounds once with .float(): the same bits for f32-representable samples; gain 1.0 returns x) and the channels
//      are exchanged where swap[r] is set.  A frame address is 8-byte aligned whenever the base is, whatever the
//      start, so the load route is chosen once per launch.  A source outside [0, n_src) or a start outside
//      [0, length] gives zeros.
__global__ __launch_bounds__(256) void gather_train_segments_kernel(const float* __restrict__ stems, int n_src,
                                                                    int64_t length, const int32_t* __restrict__ src,
                                                                    const int64_t* __restrict__ start,
                                                                    const double* __restrict__ gain,
                                                                    const uint8_t* __restrict__ swap, int64_t S,
                                                                    int64_t bx, int64_t tiles, int vec,
                                                                    float* __restrict__ out) {
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r = tile / bx;
    const int64_t j = (tile % bx) * 256 + threadIdx.x;
    if (j >= S) continue;
    const int sr = src[r];
    const int64_t st = start[r];
    float a = 0.f, b = 0.f;
    if (sr >= 0 && sr < n_src && st >= 0 && st < length && j < length - st) {
        const float* p = stems + ((int64_t)sr * length + st + j) * 2;
        float x, y;
        if (vec) {
            const float2 q = *reinterpret_cast<const float2*>(p);
            x = q.x; y = q.y;
        } else {
            x = p[0]; y = p[1];
        }
        const double gn = gain[r];
        x = (float)((double)x * gn);
        y = (float)((double)y * gn);
        const bool sw = swap[r] != 0;
        a = sw ? y : x;
        b = sw ? x : y;
    }
    out[(r * 2) * S + j] = a;
    out[(r * 2 + 1) * S + j] = b;
  }
}

int gather_train_segments_launch(const float* stems, int n_src, int64_t length, const int32_t* src,
                                 const int64_t* start, const double* gain, const uint8_t* swap, int64_t rows, int64_t S,
                                 float* out, hipStream_t s) {
    if (!stems || !src || !start || !gain || !swap || !out || n_src <= 0 || length <= 0 || rows <= 0 || S <= 0)
        return -1;
    if (((uintptr_t)stems & 3) || ((uintptr_t)out & 3) || ((uintptr_t)src & 3) || ((uintptr_t)start & 7) ||
        ((uintptr_t)gain & 7))
        return -1;
    const int64_t bx = (S + 255) / 256;
    if (bx > INT64_MAX / rows) return -1;
    const int64_t tiles = rows * bx;
    hipLaunchKernelGGL(gather_train_segments_kernel, dim3((unsigned)std::min<int64_t>(tiles, LR_MAX_GRID)), dim3(256), 0,
                       s, stems, n_src, length, src, start, gain, swap, S, bx, tiles,
                       (int)(((uintptr_t)stems & 7) == 0), out);
    return (int)hipGetLastError();
}

}  // namespace athd
