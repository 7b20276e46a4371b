// Decoder-only (Llama / Qwen2 family) kernels for gfx950 at head_dim = 64: Llama-3.2-1B, TinyLlama-1.1B, SmolLM2, Qwen2.5-0.5B.
// The semantics are the ones quoted at the top of llama_kernels.h at this width: rotate_half pairs element i with i + 32, scaling
// = 64**-0.5, rotary tables [max_pos][32], causal mask, fp32 softmax, repeat_kv.  Here is what is this width's own: the rotation, and
// the numbers of the prefill attention's LDS at this width.  What does not see the head width (bias_add8 / bias_v8 / rope_rot) is llama_kernels.h's, and so are the kernels templated on it:
// the prefill attention (attn_causal_tile_kernel<64, .>) and the decode step (cache fill, cached attention, combine), which rotates
// a 64-wide row by rope64_pairs below.
#pragma once
#include "llama_kernels.h"

// The 8 rotated pairs a thread owns (elements i0 .. i0 + 7 of a head's first half and their partners 32 further), in ONE form for
// the prefill (rope64_kernel) and the step (attn_dec_cached_kernel<64>), with and without the Qwen2 bias: fp32 sum of the fp16 GEMM
// output and the bias (bias-free: + 0.0f, which is what an all-zero bias adds - so "an all-zero bias gives the bias-free bits" holds
// by construction, not by what a compiler contracts), then rope_rot's fused form for every pair, then ONE fp16 rounding.
template <bool BIAS>
__device__ __forceinline__ void rope64_pairs(const half_t* __restrict__ head, const float* __restrict__ bias_head, int i0,
                                             const float (&co)[8], const float (&si)[8], half8& oa, half8& ob) {
  const half8 a = *(const half8*)(head + i0), b = *(const half8*)(head + 32 + i0);
  float xa[8], xb[8];
  if constexpr (BIAS) {
    bias_add8(xa, a, bias_head + i0);
    bias_add8(xb, b, bias_head + 32 + i0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) { xa[j] = (float)a[j] + 0.0f; xb[j] = (float)b[j] + 0.0f; }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float lo, hi;
    rope_rot(xa[j], xb[j], co[j], si[j], true, lo, hi);
    oa[j] = f2h_sat(lo);
    ob[j] = f2h_sat(hi);
  }
}

// In place on the fused QKV buffer [T, ld]: the first n_rot heads of a row (all query heads, then all key heads) are rotated by
// the row's position.  cos / sin: [max_pos, 32] fp32.  One workgroup per token; a thread takes 8 consecutive pairs of one head:
// 16-byte accesses.  BIAS (Qwen2): bias [(n_rot + n_v) * 64] fp32 in q | k | v order is added before the rotation - ONE fp16
// rounding for q and k, after bias and rotation - and to the n_v value heads behind them (touched only here).
template <bool BIAS>
__global__ __launch_bounds__(256) void rope64_kernel(half_t* __restrict__ qkv, const int* __restrict__ pos,
                                                     const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                     int ld, int n_rot, const float* __restrict__ bias, int n_v) {
  const int t = blockIdx.x;
  const int p = pos[t];
  half_t* row = qkv + (size_t)t * ld;
  const float* cr = cos_t + (size_t)p * 32;
  const float* sr = sin_t + (size_t)p * 32;
  for (int c = threadIdx.x; c < n_rot * 4; c += 256) {
    const int head = c >> 2, i0 = (c & 3) * 8;
    float co[8], si[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { co[j] = cr[i0 + j]; si[j] = sr[i0 + j]; }
    half_t* x = row + head * 64;
    half8 oa, ob;
    rope64_pairs<BIAS>(x, BIAS ? bias + head * 64 : nullptr, i0, co, si, oa, ob);
    *(half8*)(x + i0) = oa;
    *(half8*)(x + 32 + i0) = ob;
  }
  if constexpr (BIAS) {
    for (int c = threadIdx.x; c < n_v * 8; c += 256) {
      const int off = (n_rot + (c >> 3)) * 64 + (c & 7) * 8;
      *(half8*)(row + off) = bias_v8(*(const half8*)(row + off), bias + off);
    }
  }
}

// The LDS of the prefill attention at this width (attn_causal_tile_kernel<64, .>, llama_kernels.h): its two row strides as
// numbers, for the plan's report - the LDS is static, nothing is requested at launch - and for the tests, which read them here.
#define ATC64_KSTR 72    // sK row stride in halfs (144 B: 16-B aligned)
#define ATC64_VSTR 68    // sVt row stride in halfs (136 B: 8-B aligned)
#define ATC64_LDS_BYTES ((64 * ATC64_KSTR + 64 * ATC64_VSTR) * 2)
static_assert(ATC64_KSTR == 64 + ATC_KPAD && ATC64_VSTR == ATC_VSTR, "the tile kernel's strides at D = 64");
