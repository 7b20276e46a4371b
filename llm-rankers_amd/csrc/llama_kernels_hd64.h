// Decoder-only (Llama / Qwen2 family) kernels for gfx950 at head_dim = 64: Llama-3.2-1B, TinyLlama-1.1B, SmolLM2, Qwen2.5-0.5B.
// The semantics are the ones quoted at the top of llama_kernels.h at this width: rotate_half pairs element i with i + 32, scaling
// = 64**-0.5, rotary tables [max_pos][32], causal mask, fp32 softmax, repeat_kv.  Here is what is this width's own: the rotation
// and the prefill attention.  The 128-wide kernels of llama_kernels.h are not touched by anything here; what does not see the
// head width (bias_add8 / bias_v8 / rope_rot, AttnCausalArgs) is theirs, and so is the decode step (cache fill, cached attention,
// combine), one family templated on the width that rotates a 64-wide row by rope64_pairs below.
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

// Flash-style causal attention, d = 64: attn_causal128_kernel's design at half the width, ONE kernel for every sequence length.
// AttnCausalArgs as there, with q heads at column 0, k heads at n_heads*64, v heads at (n_heads + n_kv)*64 and ctx [T, ldctx] of
// n_heads*64 columns.  grid = (ceil(maxL / 128), n_heads, B); 256 threads = 4 waves x 32 queries.  Per 64-key tile: K rows and V
// TRANSPOSED are staged in LDS (17.5 KiB); S^T = K Q^T by MFMA 32x32x16 (four k16 steps; A = K rows, B = Q^T) so a lane owns ONE
// query column and the online-softmax state is per-lane scalars; the fp16 probabilities are already in B-operand position for
// O^T = V^T P^T (two 32-row d fragments).  Tiles above the diagonal are skipped, the diagonal tile is masked per lane.  A row's
// arithmetic depends on its own sequence only (its position, its keys in tiles of 64 in order): batch-independent.
#define ATC64_KSTR 72    // sK row stride in halfs (144 B: 16-B aligned)
#define ATC64_VSTR 68    // sVt row stride in halfs (136 B: 8-B aligned)
#define ATC64_LDS_BYTES ((64 * ATC64_KSTR + 64 * ATC64_VSTR) * 2)
// The windowed form (Mistral's sliding window, AttnCausalWinArgs::window = W > 0: query i sees keys max(0, i - W + 1) .. i; the entry
// attn_causal64_win_kernel) differs from the plain one in the tiles it skips and the keys it masks, nothing else: the tile loop
// starts at the first tile that holds a visible key of the block's first query, a wave skips a tile that ends below its first
// query's bound, and a tile that starts below the bound of the wave's last query inside the sequence gets the lower mask - the causal
// edge's -1e30.  So a sequence no longer than W gets the plain kernel's bits from it.  (A lane whose keys of a tile are ALL below
// its bound - the tile is another lane's - forms weights exp2(0) = 1 against its maximum of -1e30; its own first visible tile
// comes later, moves the maximum to a real score and multiplies all of that by alpha = exp2(-1e30 - m) = 0, exactly.)
#define ATC64_WIN 0
#define ATC64_KERNEL attn_causal64_kernel
#define ATC64_ARGS AttnCausalArgs
#include "attn_causal64.inc"
#undef ATC64_WIN
#undef ATC64_KERNEL
#undef ATC64_ARGS
#define ATC64_WIN 1
#define ATC64_KERNEL attn_causal64_win_kernel
#define ATC64_ARGS AttnCausalWinArgs
#include "attn_causal64.inc"
#undef ATC64_WIN
#undef ATC64_KERNEL
#undef ATC64_ARGS
