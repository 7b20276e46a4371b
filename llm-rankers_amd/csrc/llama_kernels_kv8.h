// FP8 K / V cache of the Llama decoding step (rk_llama_set_kv_fp8; DESIGN.md section 3 "FP8 K/V cache"): head_dim 128 only.
//
// Format (engine-private).  A group is the 128 values of ONE key or value vector of one (cache row, kv head, position) - a key as
// the fp16 cache holds it (bias, head norm, rotation, one fp16 rounding), a value behind the Qwen2 bias.  Per group one int8
// exponent e by the weight quantiser's rule (gemm_fp8.h: the smallest e with absmax <= 448 * 2^e, clamped to [-15, 7], all-zero:
// -15), per value one OCP e4m3fn byte rne_sat(x * 2^-e).  q * 2^e is an fp16 number by the weights' argument.
// Layout per layer: K bytes [rows][n_kv][P][128] | V bytes | K exponents [rows][n_kv][P'] | V exponents, P' = P rounded up to 32
// (a wave reads its 32 keys' exponents as two aligned 16-byte loads); every region starts on a multiple of 32 bytes.
//
// ONE quantiser, kv8_quant16, on the lane mapping of attn_dec_cached_body (lane c of a vector's 16 holds dims 8 c .. 8 c + 7),
// called by every writer - the fill (prefill, session admit), the step's owning workgroup, the drafting step's append - so a key a
// step writes is byte for byte the key the fill writes for that token.  MODE 1 stores bytes and exponents; MODE 2 (option
// llama_kv_fp8 = 0) stores the dequantised fp16 values into a cache of the fp16 layout: the same helper, the same rounding.
#pragma once
#include "gemm_fp8.h"
#include "llama_kernels.h"
#include "llama_kernels_qknorm.h"

// A lane's half8 of a vector held by 16 adjacent lanes (an aligned group, all of it active) -> its 8 bytes, the vector's exponent,
// and (returned) the dequantised half8.  The maximum through a fixed tree over the 16 lanes, the exponent in integers, the byte
// by integer rounding (fp8_group_exp / fp8_encode: the weight quantiser's); no atomics.  x * 2^-e is exact in f32.  The
// dequantised values come from kv8_deq8, the reader's own conversion.
__device__ __forceinline__ half8 kv8_quant16(const half8 x, kv8_u2& q, int& e) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf((float)x[j]));
  a = fmaxf(a, __shfl_xor(a, 1));
  a = fmaxf(a, __shfl_xor(a, 2));
  a = fmaxf(a, __shfl_xor(a, 4));
  a = fmaxf(a, __shfl_xor(a, 8));
  e = fp8_group_exp(a);
  const float down = __builtin_bit_cast(float, (127 - e) << 23);
  unsigned w[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j >> 2] |= fp8_encode((float)x[j] * down) << (8 * (j & 3));
  q = kv8_u2{w[0], w[1]};
  return kv8_deq8(q, e);
}
// 8 bytes x 2^e -> the half8 the fp16 kernel loads from the dequantised cache: fp8_frag's route (byte -> f32 -> f16 -> x 2^e in
// fp16, every stage exact), the one SkinnyFeedFp8 takes.
__device__ __forceinline__ half8 kv8_deq8(const kv8_u2 q, int e) { return fp8_frag(q[0], q[1], e); }

struct LlamaDecAttnKv8Args : LlamaDecAttnKeysArgs {   // kc / vc: the byte planes (MODE 1) or the fp16 planes (MODE 2)
  int8_t* ke;            // key exponents [rows][n_kv][pe]
  int8_t* ve;            // value exponents
  int pe;                // P rounded up to 32
};

// kv_cache_fill_kernel<128, SLOTS> on an FP8-cache engine: the fp16 entry's body (llama_kernels.h) in the cache's MODE.
template <bool SLOTS, int MODE>
__global__ __launch_bounds__(256) void kv8_cache_fill_kernel(const half_t* __restrict__ qkv, const int* __restrict__ seq_off,
                                                             const int* __restrict__ slots, int n_slots, Kv8Cache cc, int ld,
                                                             int n_heads, int n_kv, int P) {
  kv_cache_fill_body<128, SLOTS, MODE>(qkv, seq_off, slots, n_slots, cc, ld, n_heads, n_kv, P);
}

// kv_cache_append_kernel<128, BIAS, QKN> on an FP8-cache engine: a (kv head)'s 16 items are 16 adjacent threads, the bound a
// multiple of 16.
template <bool BIAS, bool QKN, int MODE>
__global__ __launch_bounds__(256) void kv8_cache_append_kernel(LlamaDecAttnKv8Args p) {
  constexpr int D = 128, LK = 16, NL = 8;
  const int b = blockIdx.x;
  if (!p.live[b]) return;                                 // uniform
  const int pos = p.pos[b];
  if (pos < 0 || pos > p.P - 1) return;                   // uniform: no write outside the cache
  const int crow = b / p.g1;
  const half_t* row = p.qkv + (size_t)b * p.ld;
  for (int it = threadIdx.x; it < p.n_kv * LK; it += 256) {
    const int kvh = it / LK, c = it % LK;
    const int i0 = (c % NL) * 8;
    const bool hi = c >= NL;
    float co[8], si[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { co[j] = p.cos_t[(size_t)pos * (D / 2) + i0 + j]; si[j] = p.sin_t[(size_t)pos * (D / 2) + i0 + j]; }
    auto rotated = [&](int hd) {
      if constexpr (QKN) return qkn_lane8(row, p.qkn, p.qkn_eps, p.n_heads, hd, i0, hi, co, si);
      else return rope_lane8<D, BIAS>(row, p.bias, hd, i0, hi, co, si);
    };
    half8 knew = rotated(p.n_heads + kvh);
    const size_t voff = (size_t)(p.n_heads + p.n_kv + kvh) * D + c * 8;
    half8 vnew = *(const half8*)(row + voff);
    if constexpr (BIAS) vnew = bias_v8(vnew, p.bias + voff);
    kv8_u2 kq, vq;
    int ek, ev;
    knew = kv8_quant16(knew, kq, ek);
    vnew = kv8_quant16(vnew, vq, ev);
    const size_t dst = (((size_t)crow * p.n_kv + kvh) * p.P + pos) * D + c * 8;
    if constexpr (MODE == 1) {
      *(kv8_u2*)((uint8_t*)p.kc + dst) = kq;
      *(kv8_u2*)((uint8_t*)p.vc + dst) = vq;
      if (c == 0) {
        const size_t ed = ((size_t)crow * p.n_kv + kvh) * p.pe + pos;
        p.ke[ed] = (int8_t)ek;
        p.ve[ed] = (int8_t)ev;
      }
    } else {
      *(half8*)(p.kc + dst) = knew;
      *(half8*)(p.vc + dst) = vnew;
    }
  }
}

// The step's attention on an FP8-cache engine: attn_dec_cached_body with KV8 = MODE (1: the byte reader; 2: the fp16 reader with the
// rounded own key).  The KEYS form reads bytes (MODE 2's drafting step runs the fp16 attn_dec_keys_*_kernel: it forms no key).
template <int R, bool BIAS, bool WIN, bool QKN, int MODE>
__global__ __launch_bounds__(256) void attn_dec_kv8_kernel(LlamaDecAttnKv8Args p) {
  attn_dec_cached_body<128, R, BIAS, WIN, QKN, false, LlamaDecAttnKv8Args, MODE>(p);
}
template <int R, bool BIAS, bool WIN, bool QKN>
__global__ __launch_bounds__(256) void attn_dec_keys_kv8_kernel(LlamaDecAttnKv8Args p) {
  attn_dec_cached_body<128, R, BIAS, WIN, QKN, true, LlamaDecAttnKv8Args, 1>(p);
}

// rk_debug_kv8_quant: n vectors of 128 [n][128] through kv8_quant16 - 16 threads a vector.
__global__ __launch_bounds__(256) void kv8_quant_rows_kernel(const half_t* __restrict__ x, int n, uint8_t* __restrict__ q,
                                                             int8_t* __restrict__ ex, half_t* __restrict__ deq) {
  const int it = blockIdx.x * 256 + threadIdx.x, v = it >> 4, c = it & 15;
  if (v >= n) return;                                     // a vector's 16 threads together
  kv8_u2 b;
  int e;
  const half8 d = kv8_quant16(*(const half8*)(x + (size_t)v * 128 + c * 8), b, e);
  *(kv8_u2*)(q + (size_t)v * 128 + c * 8) = b;
  *(half8*)(deq + (size_t)v * 128 + c * 8) = d;
  if (c == 0) ex[v] = (int8_t)e;
}
