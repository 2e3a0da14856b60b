// Embedding comparison: the device side of embedding_comparison.py:109-111 (row normalisation), :177-184
// (cosine_similarity / euclidean_distances of scikit-learn, written out as formulas) and :307-333 (analyze_clustering).
//
//   pass 1  ec_norm_kernel     one block per row.  The row (d <= 4096: 16 values per thread) is held in registers, so the
//                              pass reads the table once: sum of squares in fp64, norm rounded to f32, den = norm + 1e-8f
//                              and v = e / den in f32 (numpy's float32 arithmetic).  Writes normed (if asked) and
//                              den[i] to the scratch.
//   pass 2  ec_tile_kernel     one block per upper-triangular 64 x 64 tile (ti <= tj).  Both row panels are staged through
//                              LDS in chunks of 32 columns, k-major (As[k][row]), each value divided by its row's den on
//                              the way in - the same f32 division as pass 1, so the tile sees the bits of `normed` without
//                              reading it (it may be NULL).  A thread owns a 4 x 4 block: one 16-byte LDS read per panel
//                              and 16 + 8 fp64 FMAs per k: g_ij and, in the same ascending-k chains, the g_ii of its
//                              rows and the g_jj of its columns, so that rows of identical bits get g_ii = g_jj = g_ij
//                              bit for bit (distance exactly 0, and the diagonal's numerator is its own g_ii).
//                              Every pair i <= j is computed once and stored twice ([i,j] and [j,i]): both matrices
//                              are bit-symmetric by construction.  For the statistics the block
//                              reduces, per class (same / different category, pairs i < j only), the count, the sum and
//                              the sum of squares centred on the TILE's mean, and writes the six doubles to the scratch.
//   pass 3  ec_stats_kernel    one block: the tile partials in a fixed order -> counts, means, then
//                              sum (x - m)^2 = sum over tiles of [M2_t + n_t (m_t - m)^2], which is exact algebra, has no
//                              cancellation and gives 0 for constant data.
// No floating-point atomics anywhere; every reduction has a fixed order: the outputs are the same bits on every run.
// Loads are 16 bytes wide wherever the group of four lies inside the row and starts on a 16-byte boundary (checked per
// row: with row_stride % 4 != 0 the rows differ), scalar otherwise.
#include "common.h"
#include "kernels.h"

namespace athd {

constexpr int EC_TILE = 64;                // tile edge of pass 2 (athd/embedding_comparison.py::TILE)
constexpr int EC_THREADS = 256;
constexpr int EC_KC = 32;                  // columns per staged chunk
constexpr int EC_MAX = 4096;               // largest n and d
constexpr int EC_PER_THREAD = EC_MAX / EC_THREADS / 4;   // float4 groups per thread in pass 1 (4)

static_assert(EC_TILE == 64, "the 4 x 4 thread blocks and the staging below are written for a 64 x 64 tile");

// sum over the block, the same value in every thread: waves by shuffles, the 4 waves in ascending order.
// `sh` holds 4 doubles; safe to call back to back (the trailing barrier frees sh for the next call).
ATHD_DEV double ec_block_sum(double v, double* sh) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;
}

// four values of a row from column k0 on; columns >= d read as 0.  One 16-byte load when the group is whole and aligned.
ATHD_DEV void ec_load4(const float* __restrict__ row, int k0, int d, float (&v)[4]) {
    if (k0 + 4 <= d && (((uintptr_t)(row + k0)) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(row + k0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = k0 + e < d ? row[k0 + e] : 0.f;
    }
}

__global__ __launch_bounds__(EC_THREADS) void ec_norm_kernel(const float* __restrict__ emb, int d, int64_t row_stride,
                                                             float* __restrict__ normed, float* __restrict__ den) {
    __shared__ double sh[4];
    const int i = blockIdx.x;
    const float* row = emb + (int64_t)i * row_stride;
    float v[EC_PER_THREAD][4];
    double ss = 0.0;
#pragma unroll
    for (int p = 0; p < EC_PER_THREAD; ++p) {
        const int k0 = 4 * ((int)threadIdx.x + EC_THREADS * p);
        if (k0 < d) {
            ec_load4(row, k0, d, v[p]);
        } else {
            v[p][0] = v[p][1] = v[p][2] = v[p][3] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fma((double)v[p][e], (double)v[p][e], ss);
    }
    ss = ec_block_sum(ss, sh);
    const float dn = (float)sqrt(ss) + 1e-8f;
    if (threadIdx.x == 0) den[i] = dn;
    if (!normed) return;
#pragma unroll
    for (int p = 0; p < EC_PER_THREAD; ++p) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[p][e] = v[p][e] / dn;
        const int k0 = 4 * ((int)threadIdx.x + EC_THREADS * p);
        if (k0 < d) {
            float* o = normed + (int64_t)i * d + k0;
            if (k0 + 4 <= d && (((uintptr_t)o) & 15) == 0) {
                *reinterpret_cast<float4*>(o) = make_float4(v[p][0], v[p][1], v[p][2], v[p][3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k0 + e < d) o[e] = v[p][e];
            }
        }
    }
}

// stage rows [r0, r0 + 64) x columns [kc, kc + 32) of the normalised table into S[k][row]; rows >= n and columns >= d
// are zeros.  512 groups of four: group f = (row f % 64, columns 4 (f / 64) ..): a wave's 64 lanes write 64 consecutive
// floats of one k (no bank conflict) and read one 16-byte group from each of 64 rows.
ATHD_DEV void ec_stage(const float* __restrict__ emb, int n, int d, int64_t row_stride, const float* __restrict__ den,
                       int r0, int kc, float (&S)[EC_KC][EC_TILE]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int f = (int)threadIdx.x + EC_THREADS * p;
        const int r = f & (EC_TILE - 1), kq = f >> 6;
        const int row = r0 + r, k0 = kc + 4 * kq;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (row < n && k0 < d) {
            ec_load4(emb + (int64_t)row * row_stride, k0, d, v);
            const float dn = den[row];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] / dn;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) S[4 * kq + e][r] = v[e];
    }
}

// part: [tiles][6] = { n_intra, sum_intra, M2_intra, n_inter, sum_inter, M2_inter } of the tile's pairs i < j
__global__ __launch_bounds__(EC_THREADS) void ec_tile_kernel(const float* __restrict__ emb, int n, int d,
                                                             int64_t row_stride, const int32_t* __restrict__ category,
                                                             const float* __restrict__ den,
                                                             float* __restrict__ sim, float* __restrict__ dist,
                                                             double* __restrict__ part, int want_stats) {
    __shared__ __attribute__((aligned(16))) float As[EC_KC][EC_TILE];
    __shared__ __attribute__((aligned(16))) float Bs[EC_KC][EC_TILE];
    __shared__ double sh[4];
    const int T = (n + EC_TILE - 1) / EC_TILE;
    int ti = 0, rest = (int)blockIdx.x;           // linear id -> (ti, tj), ti <= tj, row-major over the upper triangle
    while (rest >= T - ti) {
        rest -= T - ti;
        ++ti;
    }
    const int tj = ti + rest;
    const int ty = (int)threadIdx.x >> 4, tx = (int)threadIdx.x & 15;
    const int i0 = ti * EC_TILE + 4 * ty, j0 = tj * EC_TILE + 4 * tx;

    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    double gi[4] = {0.0, 0.0, 0.0, 0.0}, gj[4] = {0.0, 0.0, 0.0, 0.0};

    for (int kc = 0; kc < d; kc += EC_KC) {
        ec_stage(emb, n, d, row_stride, den, ti * EC_TILE, kc, As);
        ec_stage(emb, n, d, row_stride, den, tj * EC_TILE, kc, Bs);
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < EC_KC; ++k) {
            const float4 a4 = *reinterpret_cast<const float4*>(&As[k][4 * ty]);
            const float4 b4 = *reinterpret_cast<const float4*>(&Bs[k][4 * tx]);
            const double a[4] = {(double)a4.x, (double)a4.y, (double)a4.z, (double)a4.w};
            const double b[4] = {(double)b4.x, (double)b4.y, (double)b4.z, (double)b4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                gi[r] = fma(a[r], a[r], gi[r]);
                gj[r] = fma(b[r], b[r], gj[r]);
            }
        }
        __syncthreads();
    }

    // epilogue: the pairs i <= j of this thread's block, each stored at [i,j] and [j,i]
    float sv[4][4];
    int cls[4][4];                                // 0 intra, 1 inter, -1 not a pair i < j < n
    int ci[4], cj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool in_i = i0 + r < n, in_j = j0 + r < n;
        ci[r] = (want_stats && in_i) ? category[i0 + r] : 0;
        cj[r] = (want_stats && in_j) ? category[j0 + r] : 0;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + r, j = j0 + c;
            sv[r][c] = 0.f;
            cls[r][c] = -1;
            if (i >= n || j >= n || i > j) continue;
            const double gij = acc[r][c];                 // i == j: the same chain as gi[r], bit for bit
            const double si = gi[r] == 0.0 ? 1.0 : sqrt(gi[r]);
            const double sj = gj[c] == 0.0 ? 1.0 : sqrt(gj[c]);
            const float s = (float)(gij / (si * sj));
            sv[r][c] = s;
            if (i < j) cls[r][c] = ci[r] == cj[c] ? 0 : 1;
            if (sim) {
                sim[(int64_t)i * n + j] = s;
                sim[(int64_t)j * n + i] = s;
            }
            if (dist) {
                const double d2 = gi[r] + gj[c] - 2.0 * gij;
                const float dv = i == j ? 0.f : (float)sqrt(d2 > 0.0 ? d2 : 0.0);
                dist[(int64_t)i * n + j] = dv;
                dist[(int64_t)j * n + i] = dv;
            }
        }
    }
    if (!want_stats) return;                      // uniform over the grid

    double cnt[2] = {0.0, 0.0}, sum[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (cls[r][c] == q) {
                    cnt[q] += 1.0;
                    sum[q] += (double)sv[r][c];
                }
    double out[6];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const double nq = ec_block_sum(cnt[q], sh);
        const double sq = ec_block_sum(sum[q], sh);
        const double mean = nq > 0.0 ? sq / nq : 0.0;
        double m2 = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (cls[r][c] == q) {
                    const double dv = (double)sv[r][c] - mean;
                    m2 = fma(dv, dv, m2);
                }
        out[3 * q] = nq;
        out[3 * q + 1] = sq;
        out[3 * q + 2] = ec_block_sum(m2, sh);
    }
    if (threadIdx.x < 6) {
        double v = out[0];
#pragma unroll
        for (int q = 1; q < 6; ++q) v = (int)threadIdx.x == q ? out[q] : v;
        part[(int64_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}

// one block.  stats = { intra_mean, intra_std, inter_mean, inter_std, separation, n_intra, n_inter, 0 }; an empty class
// gives 0 / 0 = NaN for its mean and std, and the separation inherits it.
__global__ __launch_bounds__(EC_THREADS) void ec_stats_kernel(const double* __restrict__ part, int tiles,
                                                              double* __restrict__ stats) {
    __shared__ double sh[4];
    double res[2][3];
    for (int q = 0; q < 2; ++q) {
        double cnt = 0.0, sum = 0.0;
        for (int t = (int)threadIdx.x; t < tiles; t += EC_THREADS) {
            cnt += part[(int64_t)t * 6 + 3 * q];
            sum += part[(int64_t)t * 6 + 3 * q + 1];
        }
        cnt = ec_block_sum(cnt, sh);
        sum = ec_block_sum(sum, sh);
        const double mean = sum / cnt;
        double m2 = 0.0;
        for (int t = (int)threadIdx.x; t < tiles; t += EC_THREADS) {
            const double nt = part[(int64_t)t * 6 + 3 * q];
            if (nt > 0.0) {
                const double dm = part[(int64_t)t * 6 + 3 * q + 1] / nt - mean;
                m2 += part[(int64_t)t * 6 + 3 * q + 2] + nt * dm * dm;
            }
        }
        m2 = ec_block_sum(m2, sh);
        res[q][0] = mean;
        res[q][1] = sqrt(m2 / cnt);
        res[q][2] = cnt;
    }
    if (threadIdx.x == 0) {
        stats[0] = res[0][0];
        stats[1] = res[0][1];
        stats[2] = res[1][0];
        stats[3] = res[1][1];
        stats[4] = res[0][0] - res[1][0];
        stats[5] = res[0][2];
        stats[6] = res[1][2];
        stats[7] = 0.0;
    }
}

static bool ec_shape_ok(int n, int d) { return n >= 1 && n <= EC_MAX && d >= 1 && d <= EC_MAX; }
static int ec_tiles(int n) {
    const int T = (n + EC_TILE - 1) / EC_TILE;
    return T * (T + 1) / 2;
}

// doubles: tile partials [tiles][6]; floats: den[n]
size_t embed_compare_scratch_bytes(int n, int d) {
    if (!ec_shape_ok(n, d)) return 0;
    return (size_t)(6 * ec_tiles(n)) * sizeof(double) + (size_t)n * sizeof(float);
}

int embed_compare_launch(const float* emb, int n, int d, int64_t row_stride, const int32_t* category, float* normed,
                         float* sim, float* dist, double* stats, void* scratch, size_t scratch_bytes, hipStream_t s) {
    if (!emb || !scratch || !ec_shape_ok(n, d) || row_stride < d || (stats && !category)) return -1;
    if (((uintptr_t)emb & 3) || ((uintptr_t)category & 3) || ((uintptr_t)normed & 3) || ((uintptr_t)sim & 3) ||
        ((uintptr_t)dist & 3) || ((uintptr_t)stats & 7) || ((uintptr_t)scratch & 7))
        return -1;
    if (scratch_bytes < embed_compare_scratch_bytes(n, d)) return -5;
    if (!normed && !sim && !dist && !stats) return 0;
    const int tiles = ec_tiles(n);
    double* part = (double*)scratch;
    float* den = (float*)(part + (size_t)6 * tiles);
    hipLaunchKernelGGL(ec_norm_kernel, dim3((unsigned)n), dim3(EC_THREADS), 0, s, emb, d, row_stride, normed, den);
    if (sim || dist || stats) {
        hipLaunchKernelGGL(ec_tile_kernel, dim3((unsigned)tiles), dim3(EC_THREADS), 0, s, emb, n, d, row_stride, category,
                           (const float*)den, sim, dist, part, stats ? 1 : 0);
        if (stats) hipLaunchKernelGGL(ec_stats_kernel, dim3(1), dim3(EC_THREADS), 0, s, (const double*)part, tiles, stats);
    }
    return (int)hipGetLastError();
}

}  // namespace athd
