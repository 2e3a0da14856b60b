// Pieces shared by the bf16 attention kernels on v_mfma_f32_32x32x16_bf16: attn32_kernel (attn.hip, the product) and
// attn_pp_kernel (attn_pp.hip, kbench and tests only).  Device code: include from a .hip translation unit.
#pragma once
#include <math.h>

#include "common.h"
#include "attn.h"

namespace athd {

// Block -> (query block, head, batch), XCD-aware (cdna_hip_programming.md T1): block i runs on XCD i % 8, so the
// tiles (bh-major, the ceil(Nq/128) query blocks of one (b, h) consecutive) are cut into 8 contiguous ranges, one
// per XCD.  All query blocks of a (b, h) then run on one XCD at about the same time and its K / V come from HBM
// once into that XCD's L2, instead of once per XCD they were spread over.
ATHD_DEV void attn_tile(const AttnDesc& d, int& qb, int& h, int64_t& b, int qblock = 128) {
    const int t = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int gq = (d.Nq + qblock - 1) / qblock;
    qb = t % gq;
    const int bh = t / gq;
    h = bh % d.heads;
    b = bh / d.heads;
}

typedef __attribute__((ext_vector_type(8))) __bf16 bf16v8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16v4;
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;          // ds_read_b64_tr_b16 operand
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;   // (arrays of these stay in registers)
typedef __attribute__((address_space(3))) void a32_lds_void;
typedef __attribute__((address_space(1))) void a32_gbl_void;

// s_setprio(1) around the QK^T and PV MFMA clusters (cdna_hip_programming.md T5): a wave in its MFMA cluster wins
// issue arbitration over the co-resident waves' softmax VALU; kbench A/B on one box: +3.3 % (N=2072), +4.6 % (N=1034)
#define A32_PRIO(x) __builtin_amdgcn_s_setprio(x)

constexpr float A32_SUMCHK = 1024.0f;               // max lane row sum of a tile before the exact-max rescale
constexpr int A32_KP = 72;                          // output staging row pitch (bf16)
constexpr int A32_VP = 64;                          // V row pitch (bf16), swizzled chunks

ATHD_DEV int a32_vchunk(int key, int chunk) { return chunk ^ (((key >> 1) & 1) << 2); }

// value of lane l ^ 32 combined with the lane's own, by v_permlane32_swap (no LDS round trip)
ATHD_DEV float half_swap_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
ATHD_DEV float half_swap_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// v_max3_f32 without the canonicalising v_max(x, x) that fmaxf puts on MFMA results (inputs are never NaN here).
// HAZARD (round 6, tools/hazard/README.md): hipcc inserts no wait states before an inline-asm instruction that reads
// an MFMA result (or a v_exp / v_rcp result): an asm VALU right after v_mfma_f32_32x32x16_bf16 reads the accumulator
// registers before the MFMA has written them, where compiler-emitted VALU reads get s_nop 9.  The round-2..5 kernel's
// per-tile max read the last QK^T MFMA's accumulators this way (a max of partly accumulated scores); the round-6
// kernel's max (tile_max, first tile and rare rescales only) puts explicit wait states before it.
ATHD_DEV float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// max over a tile's scores of the lane's query.  The vmax3 asm reads MFMA results and hipcc pads nothing before it (see
// vmax3): the caller's MFMAs are fenced off by sched_barrier and 12 explicit wait states (compiler VALU reads get 10).
template <int NKB>
ATHD_DEV float a32_tile_max(const f32x16_t (&sc)[NKB]) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 11" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    float mxk[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {                             // independent chains, one per key block
        float m = vmax3(sc[kb][0], sc[kb][1], sc[kb][2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2) m = vmax3(m, sc[kb][i], sc[kb][i + 1]);
        mxk[kb] = vmax3(m, sc[kb][15], sc[kb][15]);
    }
    float mx = mxk[0];
#pragma unroll
    for (int kb = 1; kb < NKB; ++kb) mx = vmax3(mx, mxk[kb], mxk[kb]);
    return half_swap_max(mx);
}

// P -> bf16: registers j0 .. j0 + 7 of a score block as the B operand of one PV k-step
ATHD_DEV bf16v8 a32_pack_p(const f32x16_t& sp, int j0) {
    const uint32_t w[4] = {pack2bf(sp[j0 + 0], sp[j0 + 1]), pack2bf(sp[j0 + 2], sp[j0 + 3]),
                           pack2bf(sp[j0 + 4], sp[j0 + 5]), pack2bf(sp[j0 + 6], sp[j0 + 7])};
    return __builtin_bit_cast(bf16v8, w);
}

// (The other pieces the two kernels spell out alike - exp2 + row sums, the key-tail mask, the normalise / stage / store
// epilogue, and attn32_kernel's QK^T macro as a lambda - stay written out in each kernel: as shared functions they
// change hipcc's code for attn32_kernel<3,2,true>.)

// Operands both kernels take: all bf16, 8-element aligned, queries prescaled (attn.h), and K / V row pitches that fit
// the LDS-DMA staging's per-lane byte offsets (key row in the tile x row pitch: 24-bit multiplies).
inline bool attn32_ok(const AttnDesc& d) {
    return d.q_bf16 && d.k_bf16 && d.v_bf16 && d.o_bf16 && fabsf(d.scale * 1.4426950408889634f - 1.f) < 1e-6f &&
           d.q_ld % 8 == 0 && d.k_ld % 8 == 0 && d.v_ld % 8 == 0 && d.o_ld % 8 == 0 && d.q_off % 8 == 0 &&
           d.k_off % 8 == 0 && d.v_off % 8 == 0 && d.Nq > 0 && d.Nk > 0 && d.k_ld > 0 && d.v_ld > 0 &&
           (int64_t)d.k_ld * 2 < (1 << 24) && (int64_t)d.v_ld * 2 < (1 << 24);
}

}  // namespace athd
