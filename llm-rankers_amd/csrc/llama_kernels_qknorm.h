// Qwen3 family (hf: models/qwen3/modeling_qwen3.py: Qwen3Attention.q_norm / k_norm): an RMSNorm over head_dim on every query and key
// head, behind the projection and in front of the rotation, with a learned weight [head_dim] per layer for q and for k.  head_dim
// 128 only (every Qwen3 size); no projection bias, no window (rk_engine_finalize refuses the combinations).
//
// The norm sits in the two places that rotate a row - the prefill's rotary kernel and the row load of the cached decode step - and
// BOTH form it with qkn_pairs below, on the thread mapping they already share (rope128_kernel's, rope_lane8's loads): a thread holds
// 8 pairs of a head, elements i0 .. i0 + 7 and their partners at + 64, 8 adjacent lanes (an aligned group) cover a head.  So the key
// a step writes to the cache is bit for bit the key a prefill writes for that token.
#pragma once
#include "llama_kernels.h"

// This lane's 8 pairs of `head` (128 fp16 GEMM outputs), normed with w[128] (fp32) and rotated on the table entries co / si.
// In a FIXED form, nothing left to the compiler's contraction:
//   sum of squares: the lane's 16 fp32 values in the order i0 .. i0 + 7, 64 + i0 .. 64 + i0 + 7 as a chain of fmas, then
//                   row8_sum_f over the head's 8 lanes (every lane of the group gets the same bits);
//   rs = rsqrtf(ss / 128 + eps);  x * rs * w as two rounded products;  rope_rot with fused = (j == 0), as every caller of it;
//   ONE fp16 rounding, f2h_sat, behind norm and rotation.
// An all-zero head: ss = 0, rs = rsqrtf(eps) is finite (eps > 0: rk_llama_set_qk_norm's caller is refused otherwise), every
// product is 0 - zeros, not NaN.  The three shuffles read the lane's own aligned group of 8 only: the callers keep such a group
// together (all of it active or none).
__device__ __forceinline__ void qkn_pairs(const half_t* __restrict__ head, const float* __restrict__ w, float eps, int i0,
                                          const float (&co)[8], const float (&si)[8], half8& oa, half8& ob) {
#pragma clang fp contract(off)
  const half8 a = *(const half8*)(head + i0), b = *(const half8*)(head + 64 + i0);
  const f32x4 wa0 = *(const f32x4*)(w + i0), wa1 = *(const f32x4*)(w + i0 + 4);
  const f32x4 wb0 = *(const f32x4*)(w + 64 + i0), wb1 = *(const f32x4*)(w + 64 + i0 + 4);
  float xa[8], xb[8], ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) { xa[j] = (float)a[j]; ss = __builtin_fmaf(xa[j], xa[j], ss); }
#pragma unroll
  for (int j = 0; j < 8; ++j) { xb[j] = (float)b[j]; ss = __builtin_fmaf(xb[j], xb[j], ss); }
  ss = row8_sum_f(ss);
  const float rs = rsqrtf(ss / 128.0f + eps);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x1 = xa[j] * rs * (j < 4 ? wa0[j & 3] : wa1[j & 3]);
    const float x2 = xb[j] * rs * (j < 4 ? wb0[j & 3] : wb1[j & 3]);
    float lo, hi;
    rope_rot(x1, x2, co[j], si[j], j == 0, lo, hi);
    oa[j] = f2h_sat(lo);
    ob[j] = f2h_sat(hi);
  }
}

// The step's row load (attn_dec_cached_body's `rotated` with QKN): this lane's 8 dims of normed and rotated head hd (of q | k) of
// `row` - the first half's (elements i0 .. i0 + 7) or with `hi` their partners'.  w: the layer's norm weights, q | k, [256] fp32.
__device__ __forceinline__ half8 qkn_lane8(const half_t* row, const float* w, float eps, int n_heads, int hd, int i0, bool hi,
                                           const float (&co)[8], const float (&si)[8]) {
  half8 oa, ob;
  qkn_pairs(row + (size_t)hd * 128, w + (hd >= n_heads ? 128 : 0), eps, i0, co, si, oa, ob);
  return hi ? ob : oa;
}

// The prefill's in-place rotation (rope128_kernel<false>: one workgroup per token, a thread takes 8 consecutive pairs of one head)
// with the norm.  The first n_heads + n_kv heads of a row are normed and rotated; the value heads behind them are not touched.
// An item is (head, group lane): c >> 3, c & 7 - the 8 lanes of an aligned group hold the 8 items of ONE head and the bound
// (n_heads + n_kv) * 8 is a multiple of 8, so a group enters and leaves the loop together and qkn_pairs' shuffles read active lanes
// only, whether the items fill a wave or not ((3, 3): 48 items) and in every trip of the loop ((40, 8): 384 items, two trips).
__global__ __launch_bounds__(256) void rope128_qkn_kernel(half_t* __restrict__ qkv, const int* __restrict__ pos,
                                                          const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                          int ld, int n_heads, int n_kv, const float* __restrict__ w, float eps) {
  const int t = blockIdx.x;
  const int p = pos[t];
  half_t* row = qkv + (size_t)t * ld;
  const float* cr = cos_t + (size_t)p * 64;
  const float* sr = sin_t + (size_t)p * 64;
  for (int c = threadIdx.x; c < (n_heads + n_kv) * 8; c += 256) {
    const int head = c >> 3, i0 = (c & 7) * 8;
    float co[8], si[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { co[j] = cr[i0 + j]; si[j] = sr[i0 + j]; }
    half_t* x = row + head * 128;
    half8 oa, ob;
    qkn_pairs(x, w + (head >= n_heads ? 128 : 0), eps, i0, co, si, oa, ob);
    *(half8*)(x + i0) = oa;
    *(half8*)(x + 64 + i0) = ob;
  }
}

// The decode step with the new row's q and k normed and rotated by qkn_lane8: attn_dec_cached_body as it is - the chunking, the
// cache write, the wave merge, the partials attn_dec_combine_kernel<128> merges - with the row transform swapped.  Every lane of a
// wave is active where the body calls `rotated` (the new key in front of every branch, the queries inside a wave-uniform one), and
// a key's 16 lanes are two aligned groups of 8 (c = 0 .. 7 the first half's dims, 8 .. 15 their partners') that both load the whole
// head: each forms the head's sum from the same 16 x 8 values in the same order.
template <int D, int R>
__global__ __launch_bounds__(256) void attn_dec_cached_qkn_kernel(LlamaDecAttnArgs p) {
  static_assert(D == 128, "q / k head norm: head_dim 128");
  attn_dec_cached_body<D, R, false, false, true>(p);
}
