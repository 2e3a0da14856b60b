// CLAP text tower (RoBERTa-base + pooler + projection): launchers of text_tower.hip, used by text_tower.cpp (the
// athd_text_* C ABI) and by the test entries of ktest.cpp.  Not part of athd_forward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace athd {

constexpr int TT_VOCAB = 50265, TT_NPOS = 514, TT_H = 768, TT_HEADS = 12, TT_DH = 64, TT_FFN = 3072, TT_PROJ = 512,
              TT_LAYERS = 12, TT_PAD = 1, TT_MAX_P = 256, TT_MAX_L = 128;
constexpr float TT_LN_EPS = 1e-12f;

enum TtAct { TT_NONE = 0, TT_GELU = 1, TT_TANH = 2, TT_RELU = 3 };

// One skinny-GEMM shape: N/16 slabs x S split-K slices workgroups of W waves; every wave contracts KW of K
// (K == S * W * KW).  The split is a property of (N, K) alone, never of M, so a row's bits do not depend on M.
struct TtGemmPlan { int N, K, S, W, KW; };
const TtGemmPlan* tt_gemm_plan(int N, int K);      // nullptr: not one of the tower's six shapes
constexpr int TT_MAX_SN = 6144;                    // max over the plans of S * N (floats of split-K slices per row)

// one-time launch configuration (the attention kernel's dynamic LDS limit); athd_text_finalize and the test entries
int tt_init();

// part (S, M, N) f32: slice s = X[:, sKc:(s+1)Kc] . W[:, sKc:(s+1)Kc]^T.  X: M rows of K floats, row stride ldx
// (rounded to bf16 in bf16 mode); W: (N, K) row-major, bf16 bits or f32.
int tt_gemm_launch(bool bf16, const void* W, const float* X, int64_t ldx, int M, const TtGemmPlan& p, float* part,
                   hipStream_t st);
// out[m, n] = act((sum_s part[s, m, n]) + bias[n] (+ res[m, n])), s ascending
int tt_reduce_launch(const float* part, int S, int M, int N, const float* bias, const float* res, int64_t ldr, int act,
                     float* out, int64_t ldo, hipStream_t st);
// out[m, :] = LayerNorm_768((sum_s part[s, m, :]) + bias + res[m, :]) * w + b   (out may alias res)
int tt_ln_launch(const float* part, int S, int M, const float* bias, const float* res, const float* w, const float* b,
                 float* out, hipStream_t st);
// x[p L + t, :] = LayerNorm(word[clamp(id)] + type[0] + position[pos]) with RoBERTa's pos = cumsum(id != 1) (id != 1) + 1
int tt_embed_launch(const int32_t* ids, int P, int L, const float* word, const float* type0, const float* pos,
                    const float* w, const float* b, float* x, hipStream_t st);
// One workgroup per (prompt, head): q, k, v = (sum_s qkv_part[s]) + bias (columns [0,768) q, [768,1536) k, [1536,2304) v)
// -> out (P L, 768).  Keys with mask 0 get probability exactly 0.
int tt_attn_launch(const float* qkv_part, int S, const float* bias, const int32_t* mask, int P, int L, float* out,
                   hipStream_t st);
// out[p, :] = (sum_s part[s, p, :]) + bias, divided by max(||.||2, 1e-12) when normalize
int tt_final_launch(const float* part, int S, int P, const float* bias, int normalize, float* out, hipStream_t st);

}  // namespace athd
