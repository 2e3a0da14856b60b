// Feature export of athd_encode (gfx950): the frozen encoder / transformer outputs, which the forward keeps
// channels-last (and, in throughput mode, partly as bf16), written as f32 in the reference's channel-first layout for a
// torch head.  Plain transposing copies: a tile goes through LDS so that the global reads run along the source's
// contiguous axis and the global writes along the destination's.  Bandwidth kernels, no tuning beyond that.
#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "prof.h"

namespace athd {

// --------------------------------------------------------------------------------------------- channels-last -> first
// Tile of XT rows x XT channels, pitch XT + 1 floats: the read phase stores tile[r][c] with c along the lanes and the
// write phase loads tile[r][c] with r along the lanes; with the odd pitch both touch 32 distinct banks per 32-lane
// half (ds_read_b32 / ds_write_b32 bank on (address / 4) % 32).
constexpr int XT = 64;

template <bool BF>
__global__ __launch_bounds__(256) void export_cf_kernel(const void* __restrict__ src, int64_t rows, int C, int Cs,
                                                        float* __restrict__ out) {
    __shared__ float tile[XT][XT + 1];
    const int64_t b = blockIdx.z;
    const int64_t r0 = (int64_t)blockIdx.x * XT;
    const int c0 = blockIdx.y * XT;
    const int cw = min(XT, Cs - c0);                          // channels of this tile (Cs = 4: 4 of them)
    const int rh = (int)min<int64_t>(XT, rows - r0);          // rows of this tile
    // read: consecutive threads along the channels of a row, then the next row (cw == C: one contiguous run)
    const int64_t sbase = (b * rows + r0) * C + c0;
    for (int i = threadIdx.x; i < rh * cw; i += 256) {
        const int r = cw == XT ? i >> 6 : i / cw;
        const int c = i - r * cw;
        const int64_t o = sbase + (int64_t)r * C + c;
        float v;
        if constexpr (BF) v = __uint_as_float((uint32_t)((const uint16_t*)src)[o] << 16);
        else v = ((const float*)src)[o];
        tile[r][c] = v;
    }
    __syncthreads();
    // write: consecutive threads along the rows of a channel
    const int64_t obase = (b * Cs + c0) * rows + r0;
    for (int i = threadIdx.x; i < cw * XT; i += 256) {
        const int c = i >> 6, r = i & (XT - 1);
        if (r < rh) out[obase + (int64_t)c * rows + r] = tile[r][c];
    }
}

int export_cf_launch(const void* src, int src_bf16, int64_t nb, int64_t rows, int C, int Cs, float* out, hipStream_t s) {
    if (!src || !out || nb <= 0 || nb > 65535 || rows <= 0 || C <= 0 || Cs <= 0 || Cs > C) return -1;
    const int64_t rt = (rows + XT - 1) / XT;
    if (rt > 0x7fffffffLL) return -1;
    const dim3 grid((unsigned)rt, (unsigned)((Cs + XT - 1) / XT), (unsigned)nb);
    KScope ks(s);
    if (ks.on())
        ks.begin(src_bf16 ? "export_cf_kernel<true>" : "export_cf_kernel<false>", 0.0,
                 (double)nb * rows * Cs * ((src_bf16 ? 2 : 4) + 4));
    if (src_bf16) hipLaunchKernelGGL(export_cf_kernel<true>, grid, dim3(256), 0, s, src, rows, C, Cs, out);
    else hipLaunchKernelGGL(export_cf_kernel<false>, grid, dim3(256), 0, s, src, rows, C, Cs, out);
    return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------- spectrogram
// specT[b][t][f] = {Re L, Im L, Re R, Im R} (frame-major, spectral.hip) -> z[b][ch][f][t] = {Re, Im}: the same
// transpose over (frame, bin), a tile of ST frames x ST bins per audio channel.  Reads: 16 B per lane along f; writes:
// 8 B per lane along t.  Pitch ST + 1 float2: lanes along f (read phase) and along t (write phase) both fall on
// distinct 8-byte slots.
constexpr int ST = 32;

__global__ __launch_bounds__(256) void export_spec_kernel(const float* __restrict__ specT, int Tspec,
                                                          float* __restrict__ z) {
    __shared__ float2 tile[2][ST][ST + 1];
    const int64_t b = blockIdx.z;
    const int f0 = blockIdx.x * ST, t0 = blockIdx.y * ST;
    const int th = min(ST, Tspec - t0);
    for (int i = threadIdx.x; i < th * ST; i += 256) {
        const int t = i >> 5, f = i & (ST - 1);
        const float4 v = *reinterpret_cast<const float4*>(specT + ((b * Tspec + t0 + t) * 2048LL + f0 + f) * 4);
        tile[0][f][t] = make_float2(v.x, v.y);
        tile[1][f][t] = make_float2(v.z, v.w);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * ST * ST; i += 256) {
        const int t = i & (ST - 1), f = (i >> 5) & (ST - 1), ch = i >> 10;
        if (t < th)
            *reinterpret_cast<float2*>(z + (((b * 2 + ch) * 2048LL + f0 + f) * Tspec + t0 + t) * 2) = tile[ch][f][t];
    }
}

int export_spec_launch(const float* specT, int64_t B, int64_t Tspec, float* z, hipStream_t s) {
    if (!specT || !z || B <= 0 || B > 65535 || Tspec <= 0 || Tspec > 65535LL * ST) return -1;
    const dim3 grid(2048 / ST, (unsigned)((Tspec + ST - 1) / ST), (unsigned)B);
    KScope ks(s);
    if (ks.on()) ks.begin("export_spec_kernel", 0.0, (double)B * Tspec * 2048 * 4 * 8);
    hipLaunchKernelGGL(export_spec_kernel, grid, dim3(256), 0, s, specT, (int)Tspec, z);
    return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------- waveform statistics
// tnorm_std[b] = {mean, std} of input_norm_params_kernel (norm.hip; the plain unbiased std, not 1e-5 + std)
__global__ void export_norm_kernel(const float* __restrict__ tnorm_std, int B, float* __restrict__ meant,
                                   float* __restrict__ stdt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    meant[b] = tnorm_std[2 * b];
    stdt[b] = tnorm_std[2 * b + 1];
}

int export_norm_launch(const float* tnorm_std, int64_t B, float* meant, float* stdt, hipStream_t s) {
    if (!tnorm_std || !meant || !stdt || B <= 0 || B > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(export_norm_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, tnorm_std, (int)B, meant,
                       stdt);
    return (int)hipGetLastError();
}

}  // namespace athd
