// Flash-style multi-head attention for the cross-domain transformer (d_head = 64, 8 heads).
// Two kernels: attn32_kernel<3,2,true> (bf16 mode) and attn_kernel<0> (f32 parity mode).
//
// Orientation: each wave computes S^T = K . Q^T for 64 keys x 32 queries, so the MFMA accumulator puts one
// query per lane column and 16 keys per lane in registers.  The column (query) max/sum of the online softmax
// are then in-lane reductions plus two cross-group shuffles, and P^T is already laid out as the B operand of
// O^T += V^T . P^T (the k order inside a step is permuted identically for A and B; see common comments in
// gemm.hip).  K is staged in LDS as [key][d], V transposed as [d][key].  Grid: (ceil(Nq/128), heads, batch).
#include "common.h"
#include "prof.h"
#include "attn.h"
#include "attn32.h"

namespace athd {

ATHD_DEV void load8(const void* base, int is_bf16, int64_t off, float* v) {
    if (is_bf16) {
        uint4 q = *reinterpret_cast<const uint4*>((const bf16_t*)base + off);
        const bf16_t* h = reinterpret_cast<const bf16_t*>(&q);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = bf2f(h[j]);
    } else {
        const float4* p = reinterpret_cast<const float4*>((const float*)base + off);
        float4 a = p[0], b = p[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}

// f32 parity mode: fp32 MFMA (16x16x4), operands of either type converted to f32 on load.
template <int MODE>
__global__ __launch_bounds__(256) void attn_kernel(const AttnDesc d) {
    static_assert(MODE == 0, "kept for the symbol attn_kernel<0> (profiles and tools key on it); 0 = f32 MFMA");
    constexpr int LDK = 64 + 4;
    __shared__ __attribute__((aligned(16))) float Ks[64 * LDK];
    __shared__ __attribute__((aligned(16))) float Vt[64 * LDK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    int qblk, h;
    int64_t b;
    attn_tile(d, qblk, h, b);
    const int q0 = qblk * 128 + wave * 32;
    const float sl2 = d.scale * 1.4426950408889634f;

    // Q^T fragments (B operand of S^T = K Q^T): lane holds Q[q][32c + 8g + j]
    float qv[2][2][8];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int q = q0 + 16 * nt + c16;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (q < d.Nq) load8(d.Q, d.q_bf16, b * d.q_bs + (int64_t)q * d.q_ld + d.q_off + h * 64 + 32 * c + 8 * g, qv[nt][c]);
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) qv[nt][c][j] = 0.f;
            }
        }
    }

    f32x4_t o[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float mrun[2] = {-INFINITY, -INFINITY};
    float lrun[2] = {0.f, 0.f};

    for (int k0 = 0; k0 < d.Nk; k0 += 64) {
        // ---- stage K [key][d] and V^T [d][key] ----
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int gi = tid + 256 * it;
            const int key = gi >> 3, d0 = 8 * (gi & 7);
            float kv[8], vv[8];
            if (k0 + key < d.Nk) {
                load8(d.K, d.k_bf16, b * d.k_bs + (int64_t)(k0 + key) * d.k_ld + d.k_off + h * 64 + d0, kv);
                load8(d.V, d.v_bf16, b * d.v_bs + (int64_t)(k0 + key) * d.v_ld + d.v_off + h * 64 + d0, vv);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) { kv[j] = 0.f; vv[j] = 0.f; }
            }
            *reinterpret_cast<float4*>(&Ks[key * LDK + d0]) = make_float4(kv[0], kv[1], kv[2], kv[3]);
            *reinterpret_cast<float4*>(&Ks[key * LDK + d0 + 4]) = make_float4(kv[4], kv[5], kv[6], kv[7]);
#pragma unroll
            for (int j = 0; j < 8; ++j) Vt[(d0 + j) * LDK + key] = vv[j];
        }
        __syncthreads();

        // ---- S^T = K Q^T : 4 key tiles x 2 query tiles ----
        f32x4_t s[4][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) s[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float* kp = &Ks[(16 * mt + c16) * LDK + 32 * c + 8 * g];
                float4 a0 = reinterpret_cast<const float4*>(kp)[0], a1 = reinterpret_cast<const float4*>(kp)[1];
                float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
                for (int ss = 0; ss < 8; ++ss)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        s[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ss], qv[nt][c][ss], s[mt][nt], 0, 0, 0);
            }
        }
        // ---- online softmax over keys (per query column) ----
        float p[4][2][4];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            float mx = -INFINITY;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = k0 + 16 * mt + 4 * g + r;
                    float v = (key < d.Nk) ? s[mt][nt][r] * sl2 : -INFINITY;
                    p[mt][nt][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mnew = fmaxf(mrun[nt], mx);
            const float alpha = exp2f(mrun[nt] - mnew);
            mrun[nt] = mnew;
            float ls = 0.f;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = exp2f(p[mt][nt][r] - mnew);
                    p[mt][nt][r] = e;
                    ls += e;
                }
            lrun[nt] = lrun[nt] * alpha + ls;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][nt][r] *= alpha;
        }
        // ---- O^T += V^T P^T ----
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float a = Vt[(16 * dt + c16) * LDK + 16 * mt + 4 * g + r];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        o[dt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, p[mt][nt][r], o[dt][nt], 0, 0, 0);
                }
        __syncthreads();
    }
    // ---- normalise and store O[q][h*64 + d] ----
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        float l = lrun[nt];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.f / l;
        const int q = q0 + 16 * nt + c16;
        if (q >= d.Nq) continue;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const int64_t off = b * d.o_bs + (int64_t)q * d.o_ld + h * 64 + 16 * dt + 4 * g;
            float4 v = make_float4(o[dt][nt][0] * inv, o[dt][nt][1] * inv, o[dt][nt][2] * inv, o[dt][nt][3] * inv);
            if (d.o_bf16) {
                bf16_t t4[4] = {f2bf(v.x), f2bf(v.y), f2bf(v.z), f2bf(v.w)};
                *reinterpret_cast<uint2*>((bf16_t*)d.O + off) = *reinterpret_cast<uint2*>(t4);
            } else {
                *reinterpret_cast<float4*>((float*)d.O + off) = v;
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------
// bf16 path on v_mfma_f32_32x32x16_bf16 (prescaled queries: scores are log2-unit logits).
//
// Per wave 32 queries, per tile 64 keys.  S^T = K Q^T as two 32x32 blocks (keys x queries): lane l holds query
// r = l & 31 and keys (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of each block, so the online softmax is in-lane plus one
// exchange between the two 32-lane halves.  The accumulators start at -m (the running max) instead of 0, so the MFMA
// itself subtracts the max: p = exp2(S) is one v_exp_f32 per score.  The max is set exactly on the first tile and
// moves afterwards only when a lane's row sum of P exceeds A32_SUMCHK (defer-max; see the softmax below).
//
// O^T += V^T P^T: for PV k-step kk (16 keys of key block kk >> 1) lane (r, h) feeds its own registers
// 8 (kk & 1) .. +7 as the B operand, i.e. keys 4h + {0..3} and 4h + 8 + {0..3} of the 16 - the k order inside the step
// is permuted, and the A operand (V^T) is read in the same permuted order with two ds_read_b64_tr_b16 (rows
// 4h + q and 4h + 8 + q; lane 4q+p of a 16-lane group addresses row k0+q, columns d0+4p..+3 and receives column
// d0+(lane&15) of rows k0..k0+3, i.e. 4 consecutive keys of one d).  No cross-lane movement of P.  MFMA issue per tile
// and wave: 8 (QK) + 8 (PV) 32x32x16 = 512 cycles; the 32x32 shape blocks vector issue for 8 of every 32 cycles (vs 8
// of 16 for 16x16x32), which leaves room for the 32 exps, the max and the row sums of each lane.
//
// LDS: K [key][64] with the 16-B chunk XOR-swizzled by (key >> 1) & 7 (a32_kidx), V [key][64] with the chunk swizzled
// by ((key >> 1) & 1) << 2 so that each 32-lane half of a transposed read (4 keys x 32 d) covers all 64 banks.  2-deep
// ring filled by LDS-DMA for the next tile before the tile's MFMAs, one barrier per tile.  The output tile is staged
// through LDS and stored as whole 128-B rows.
//
// The A/B variants this kernel came out of (16x16x32 kernel, register staging, other tile shapes, the round-5 softmax,
// ...) and their numbers: DESIGN.md §3, round 6, "Attention variants tried and dropped".

#define ATHD_A32_QK(INIT)                                                                                      \
    do {                                                                                                       \
        const float init_ = (INIT);                                                                            \
        _Pragma("unroll") for (int kb = 0; kb < NKB; ++kb)                                                    \
            _Pragma("unroll") for (int i = 0; i < 16; ++i) sc[kb][i] = init_;                                  \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                      \
            _Pragma("unroll") for (int kb = 0; kb < NKB; ++kb) {                                              \
                const bf16v8 a_ = *reinterpret_cast<const bf16v8*>(&K_[a32_kidx(32 * kb + r, 2 * ks + hh)]);   \
                sc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_, qf[ks], sc[kb], 0, 0, 0);                 \
            }                                                                                                  \
        if (kt0 + KT > d.Nk) {                                                                                 \
            int lim_ = d.Nk - kt0 - 4 * hh;            /* key index - kt0 - 4 hh vs constants: no per-key adds */ \
            asm volatile("" : "+v"(lim_));             /* (keeps the compares in this branch, not hoisted) */  \
            _Pragma("unroll") for (int kb = 0; kb < NKB; ++kb)                                                \
                _Pragma("unroll") for (int i = 0; i < 16; ++i)                                                 \
                    if (32 * kb + (i & 3) + 8 * (i >> 2) >= lim_) sc[kb][i] = -INFINITY;                       \
        }                                                                                                      \
    } while (0)

// K tile element index of (key, 16-B chunk): pitch 64, chunk XOR-swizzled by (key >> 1) & 7 - the QK^T fragment reads
// (lanes = 32 consecutive keys, one chunk) then put the 16 lanes of every ds_read_b128 group on 16 distinct 4-bank
// groups (key & 1 picks the bank half of the 128-B row).
ATHD_DEV int a32_kidx(int key, int chunk) { return key * 64 + 8 * (chunk ^ ((key >> 1) & 7)); }

// K / V tiles are staged by global_load_lds_dwordx4 straight into LDS (no VGPR round trip and none of the
// ds_write_b128 transfer cost, which with 4 waves' 16 KB of fragment reads per tile kept the LDS ~90 % busy).  One
// wave instruction fills 1 KB = 8 keys x 128 B, lane -> (key base + lane / 8, physical chunk lane % 8); the lane fetches
// the logical chunk that the tile's swizzle places there.
template <int MINW, int NKB, bool DMA>
__global__ __launch_bounds__(256, MINW) void attn32_kernel(const AttnDesc d) {
    static_assert(DMA, "kept for the symbol attn32_kernel<3,2,true> (profiles and tools key on it); LDS-DMA staging only");
    constexpr int KT = 32 * NKB;                                  // keys per tile
    constexpr int KSZ = KT * 64;                                  // K slot elements
    // K ring, V ring; the output staging (4 waves x 32 rows x 72) reuses the front
    constexpr int SMEM_E = 2 * KSZ + 2 * KT * A32_VP;
    static_assert(SMEM_E >= 4 * 32 * A32_KP, "output staging fits");
    __shared__ __attribute__((aligned(16))) bf16_t smem_a32[SMEM_E];
    bf16_t (*Ks)[KSZ] = reinterpret_cast<bf16_t (*)[KSZ]>(smem_a32);
    bf16_t (*Vs)[KT * A32_VP] = reinterpret_cast<bf16_t (*)[KT * A32_VP]>(smem_a32 + 2 * KSZ);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    int qblk, h;
    int64_t b;
    attn_tile(d, qblk, h, b);
    const int qw0 = qblk * 128 + wave * 32;
    const bool active = qw0 < d.Nq;                               // wave-uniform
    const int q = min(qw0 + r, d.Nq - 1);                          // rows past Nq compute on a copy, never stored

    // Q^T fragments (B operand): lane (r, h) holds Q[q][16 ks + 8h .. +7]
    bf16v8 qf[4];
    {
        const bf16_t* Qp = (const bf16_t*)d.Q + b * d.q_bs + (int64_t)q * d.q_ld + d.q_off + h * 64 + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16v8*>(Qp + 16 * ks);
    }

    const bf16_t* Kb = (const bf16_t*)d.K + b * d.k_bs + d.k_off + h * 64;
    const bf16_t* Vb = (const bf16_t*)d.V + b * d.v_bs + d.v_off + h * 64;
    // LDS-DMA staging of tile KT0 into slot ST: wave w fills keys 8 (w + 4 j) .. +7 of K and of V, j < KT / 32
    const int dkey = lane >> 3, dph = lane & 7;
    // A tile's sources are a wave-uniform base (the tile's first key row) plus a 32-bit per-lane byte offset (key row
    // in the tile, clamped to the last key, times the row pitch, plus the swizzled chunk), so each piece is one v_min +
    // one v_mad_u32_u24 and the load takes the SGPR-base form (64-bit per-piece address arithmetic cost ~100 issue
    // cycles per tile).  Keys past Nk re-read the last key: finite data, their scores are masked to -inf.
    // The swizzles depend on key & 15 only, and KT0 is a multiple of 64, so they are tile-invariant.
    const uint32_t kldb = (uint32_t)d.k_ld * 2u, vldb = (uint32_t)d.v_ld * 2u;
    uint32_t kswz[KT / 32], vswz[KT / 32];
#pragma unroll
    for (int j = 0; j < KT / 32; ++j) {
        const int kk = 8 * (wave + 4 * j) + dkey;
        kswz[j] = 16u * (uint32_t)(dph ^ ((kk >> 1) & 7));
        vswz[j] = 16u * (uint32_t)a32_vchunk(kk, dph);
    }
#define ATHD_A32_DMA(KT0, ST)                                                                                  \
    {                                                                                                          \
        const char* kt_ = (const char*)(Kb + (int64_t)(KT0) * d.k_ld);                                         \
        const char* vt_ = (const char*)(Vb + (int64_t)(KT0) * d.v_ld);                                         \
        const int last_ = d.Nk - 1 - (KT0);                                                                    \
        _Pragma("unroll") for (int j = 0; j < KT / 32; ++j) {                                                 \
            const uint32_t kc_ = (uint32_t)min(8 * (wave + 4 * j) + dkey, last_);                              \
            uint32_t ko_ = __umul24(kc_, kldb) + kswz[j];                                     \
            uint32_t vo_ = __umul24(kc_, vldb) + vswz[j];                                     \
            asm volatile("" : "+v"(ko_), "+v"(vo_));     /* opaque: keeps (uniform base, 32-bit offset) */   \
            __builtin_amdgcn_global_load_lds((a32_gbl_void*)(kt_ + ko_),                                       \
                                             (a32_lds_void*)&Ks[ST][8 * (wave + 4 * j) * 64], 16, 0, 0);        \
            __builtin_amdgcn_global_load_lds((a32_gbl_void*)(vt_ + vo_),                                       \
                                             (a32_lds_void*)&Vs[ST][8 * (wave + 4 * j) * A32_VP], 16, 0, 0);   \
        }                                                                                                      \
    }

    // transposed-read addresses (elements): lane 4q'+p of 16-lane group g' -> key row 4h + q' (+8, +16 s2, +32 kb),
    // d columns 32 db + 16 (g' & 1) + 4p
    const int g16 = lane >> 4, i16 = lane & 15, qr = i16 >> 2, pc = i16 & 3;
    const int vrow = 4 * hh + qr;                                  // + 16 s2 + 32 kb (+ 8): same (row >> 1) & 1
    int voff[2];
#pragma unroll
    for (int db = 0; db < 2; ++db) {
        const int col = 32 * db + 16 * (g16 & 1) + 4 * pc;
        voff[db] = vrow * A32_VP + 8 * a32_vchunk(vrow, col >> 3) + (col & 7);
    }

    f32x16_t o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float mrun = 0.f, lrun = 0.f;

    const int ntiles = (d.Nk + KT - 1) / KT;
    ATHD_A32_DMA(0, 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < ntiles; ++t) {
        const int kt0 = t * KT;
        const bool more = t + 1 < ntiles;
        if (more) {
            // slot cur ^ 1 was last read in iteration t - 1, which ended with a barrier
            ATHD_A32_DMA(kt0 + KT, cur ^ 1)
        }
        if (active) {
            const bf16_t* K_ = Ks[cur];
            const bf16_t* V_ = Vs[cur];
            // ---- S^T = K Q^T - m ----
            f32x16_t sc[NKB];
            // (ATHD_A32_QK: key tail -> scores of keys >= Nk are -inf)
            A32_PRIO(1);
            ATHD_A32_QK(-mrun);
            A32_PRIO(0);
            // ---- online softmax (log2 units): no per-tile max ----
            // The running max is set exactly on the first tile.  Later tiles exponentiate against it at once, and the
            // lane's own row sum (its 32 P values, computed anyway) tells whether any of its P exceeds A32_SUMCHK: only
            // then (rare, __any) are the scores recomputed, their exact max taken, O and l rescaled and the tile
            // re-exponentiated - so P <= A32_SUMCHK always (the defer-max bound; bf16 P keeps its relative precision at
            // any scale).  Saves the 17 v_max3 + swap + compare of every tile (~90 of ~900 issue cycles per tile).
            auto exp_sum = [&]() -> float {                       // P = exp2(S) in place; the lane's row sum
                athd_f2v ls2[NKB];                                 // one chain per key block
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) {
                    ls2[kb] = (athd_f2v){0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < 16; i += 2) {
                        sc[kb][i] = __builtin_amdgcn_exp2f(sc[kb][i]);
                        sc[kb][i + 1] = __builtin_amdgcn_exp2f(sc[kb][i + 1]);
                        ls2[kb] += (athd_f2v){sc[kb][i], sc[kb][i + 1]};
                    }
                }
#pragma unroll
                for (int kb = 1; kb < NKB; ++kb) ls2[0] += ls2[kb];
                return ls2[0].x + ls2[0].y;
            };
            // (a lambda, not `mrun = ...`: with mrun assigned directly hipcc allocates the kernel's registers differently)
            auto set_max = [&](float m) { mrun = m; };
            if (t == 0) {                                          // first tile: the exact max (O and l are zero)
                set_max(a32_tile_max<NKB>(sc));
                // the scores already in registers, shifted by the max (instead of QK^T again from -m: 32 v_sub against
                // 8 MFMAs + 32 v_mov + the K re-read)
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) sc[kb][i] -= mrun;
            }
            float ls = exp_sum();
            if (__any(!(ls <= A32_SUMCHK))) {                      // some P > A32_SUMCHK (or not finite): rescale
                ATHD_A32_QK(-mrun);
                const float m_old = mrun;
                set_max(mrun + fmaxf(a32_tile_max<NKB>(sc), 0.f));
                const float alpha = __builtin_amdgcn_exp2f(m_old - mrun);
                lrun *= alpha;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    o0[i] *= alpha;
                    o1[i] *= alpha;
                }
                ATHD_A32_QK(-mrun);
                ls = exp_sum();
            }
            lrun += ls;
            // ---- O^T += V^T P^T ----
            A32_PRIO(1);
#pragma unroll
            for (int kk = 0; kk < 2 * NKB; ++kk) {
                const f32x16_t& sp = sc[kk >> 1];
                const int j0 = 8 * (kk & 1);
                const bf16v8 pb = a32_pack_p(sp, j0);
                const int rb = (32 * (kk >> 1) + 16 * (kk & 1)) * A32_VP;
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const bf16_t* base = &V_[rb + voff[db]];
                    const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)base);
                    const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(base + 8 * A32_VP));
                    const bf16v8 a = __builtin_shufflevector(__builtin_bit_cast(bf16v4, lo),
                                                             __builtin_bit_cast(bf16v4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
                    if (db == 0) o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb, o0, 0, 0, 0);
                    else o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb, o1, 0, 0, 0);
                }
            }
            A32_PRIO(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's DMA into slot cur ^ 1 landed
        __syncthreads();
        cur ^= 1;
    }
    // ---- normalise; stage the wave's 32 x 64 output tile in LDS; store whole 128-B rows ----
    const float l = half_swap_sum(lrun);
    const float inv = 1.f / l;
    bf16_t* stage = smem_a32 + wave * 32 * A32_KP;                 // 4 waves x 32 rows x 72 (static_assert above)
    if (active) {
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const f32x16_t& oo = db ? o1 : o0;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int dcol = 32 * db + 8 * g4 + 4 * hh;
                *reinterpret_cast<uint2*>(&stage[r * A32_KP + dcol]) =
                    make_uint2(pack2bf(oo[4 * g4] * inv, oo[4 * g4 + 1] * inv),
                               pack2bf(oo[4 * g4 + 2] * inv, oo[4 * g4 + 3] * inv));
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);                         // lgkmcnt(0): the wave's own LDS writes landed
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int id = it * 64 + lane, row = id >> 3, ch = id & 7;
            const int qq = qw0 + row;
            if (qq < d.Nq) {
                const uint4 v = *reinterpret_cast<const uint4*>(&stage[row * A32_KP + 8 * ch]);
                *reinterpret_cast<uint4*>((bf16_t*)d.O + b * d.o_bs + (int64_t)qq * d.o_ld + h * 64 + 8 * ch) = v;
            }
        }
    }
}

#undef ATHD_A32_DMA
#undef ATHD_A32_QK

// bf16 mode -> attn32_kernel (the forward's Q/K/V/O are bf16, 8-element aligned, Q prescaled; any other bf16-mode
// operand set is refused); f32 parity mode -> attn_kernel<0> (fp32 MFMA)
int attn_launch(const AttnDesc& d, int mode, hipStream_t s) {
    if (d.heads * 64 > d.o_ld && d.o_ld != 0) return -2;
    const bool a32 = mode == 1 && attn32_ok(d);
    if (!a32 && mode != 0) return -3;
    dim3 grid((unsigned)((d.Nq + 127) / 128) * (unsigned)d.heads * (unsigned)d.nb);   // attn_tile decodes it
    KScope ks(s);
    if (ks.on()) {
        const double nh = (double)d.nb * d.heads;
        const double fl = 4.0 * nh * d.Nq * d.Nk * 64;
        const double by = nh * 64 * (d.Nq * (d.q_bf16 ? 2 : 4) + d.Nk * ((d.k_bf16 ? 2 : 4) + (d.v_bf16 ? 2 : 4)) +
                                     d.Nq * (d.o_bf16 ? 2 : 4));
        ks.begin(a32 ? "attn32_kernel<3,2,true>" : "attn_kernel<0>", fl, by);
    }
    if (a32) hipLaunchKernelGGL((attn32_kernel<3, 2, true>), grid, dim3(256), 0, s, d);
    else hipLaunchKernelGGL(attn_kernel<0>, grid, dim3(256), 0, s, d);
    return (int)hipGetLastError();
}

}  // namespace athd
