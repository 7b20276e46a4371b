// Decoder-only (Llama / Qwen2 family) kernels for gfx950 at head_dim = 64: Llama-3.2-1B, TinyLlama-1.1B, SmolLM2, Qwen2.5-0.5B.
// The semantics are the ones quoted at the top of llama_kernels.h at this width: rotate_half pairs element i with i + 32, scaling
// = 64**-0.5, rotary tables [max_pos][32], causal mask, fp32 softmax, repeat_kv.  The 128-wide kernels of llama_kernels.h are not
// touched by anything here; what does not see the head width (bias_add8 / bias_v8 / rope_rot, AttnCausalArgs, LDC_CHUNK) is theirs.
#pragma once
#include "llama_kernels.h"

// The 8 rotated pairs a thread owns (elements i0 .. i0 + 7 of a head's first half and their partners 32 further), in ONE form for
// the prefill (rope64_kernel) and the step (attn_dec_cached64_body), with and without the Qwen2 bias: fp32 sum of the fp16 GEMM
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
__global__ __launch_bounds__(256) void attn_causal64_kernel(AttnCausalArgs p) {
  __shared__ __attribute__((aligned(16))) half_t sK[64 * ATC64_KSTR];
  __shared__ __attribute__((aligned(16))) half_t sVt[64 * ATC64_VSTR];
  const int b = blockIdx.z, h = blockIdx.y, qt = blockIdx.x;
  const int tok0 = p.seq_off[b];
  const int L = p.seq_off[b + 1] - tok0;
  if (qt * 128 >= L) return;   // uniform for the whole block
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hh = lane >> 5, l31 = lane & 31;
  const int kvh = h / (p.n_heads / p.n_kv);
  const half_t* kbase = p.qkv + (size_t)(p.n_heads + kvh) * 64;
  const half_t* vbase = p.qkv + (size_t)(p.n_heads + p.n_kv + kvh) * 64;
  const int q0 = qt * 128 + wave * 32;
  const bool wave_active = q0 < L;
  const int qpos = q0 + l31;
  const int qrow = qpos < L ? qpos : L - 1;
  half8 qf[4];
  {
    const half_t* qptr = p.qkv + (size_t)(tok0 + qrow) * p.ld + h * 64 + 8 * hh;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *(const half8*)(qptr + 16 * s);
  }
  f32x16 o[2];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[f][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const int last_q = min(qt * 128 + 127, L - 1);
  const int nkt = (last_q >> 6) + 1;                 // key tiles this block of queries can see (causal)
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();                                   // the previous tile's fragments are read
    // ---- stage K (row-major) and V^T (key pairs) of keys kt*64 .. kt*64+63; rows beyond L are clamped copies (masked) ----
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i, row = c >> 3, cc = c & 7;
      const int key = min(kt * 64 + row, L - 1);
      *(half8*)(sK + row * ATC64_KSTR + cc * 8) = *(const half8*)(kbase + (size_t)(tok0 + key) * p.ld + cc * 8);
    }
    {
      const int kp = tid >> 3, cc = tid & 7;
      const int k0 = min(kt * 64 + 2 * kp, L - 1), k1 = min(kt * 64 + 2 * kp + 1, L - 1);
      const half8 v0 = *(const half8*)(vbase + (size_t)(tok0 + k0) * p.ld + cc * 8);
      const half8 v1 = *(const half8*)(vbase + (size_t)(tok0 + k1) * p.ld + cc * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const half2v pr = {v0[j], v1[j]};
        *(half2v*)(sVt + (cc * 8 + j) * ATC64_VSTR + 2 * kp) = pr;
      }
    }
    __syncthreads();
    if (!wave_active || kt * 64 > q0 + 31) continue;    // this wave's queries see none of these keys
    f32x16 s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const half8 k0 = *(const half8*)(sK + l31 * ATC64_KSTR + 16 * s + 8 * hh);
      const half8 k1 = *(const half8*)(sK + (32 + l31) * ATC64_KSTR + 16 * s + 8 * hh);
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(k0, qf[s], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(k1, qf[s], s1, 0, 0, 0);
    }
    // ---- online softmax (log2 domain); lane = query qpos, register r <-> key key_base + (r&3) + 8(r>>2) (+32 for s1) ----
    const int key_base = kt * 64 + 4 * hh;
    const bool need_mask = kt * 64 + 63 > q0 || kt * 64 + 63 >= L;   // the tile touches the diagonal or the sequence end
    float tmax = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] *= p.scale_log2e;
      s1[r] *= p.scale_log2e;
      if (need_mask) {
        const int key0 = key_base + (r & 3) + 8 * (r >> 2);
        s0[r] = (key0 <= qpos && key0 < L) ? s0[r] : -1e30f;
        s1[r] = (key0 + 32 <= qpos && key0 + 32 < L) ? s1[r] : -1e30f;
      }
      tmax = fmaxf(tmax, fmaxf(s0[r], s1[r]));
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float m_new = fmaxf(m_run, tmax);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = __builtin_amdgcn_exp2f(s0[r] - m_new);
      s1[r] = __builtin_amdgcn_exp2f(s1[r] - m_new);
      psum += s0[r] + s1[r];
    }
    psum += __shfl_xor(psum, 32);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    l_run = l_run * alpha + psum;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[f][r] *= alpha;
    m_run = m_new;
    // ---- O^T += V^T P^T ----
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        half8 pf;
#pragma unroll
        for (int i = 0; i < 8; ++i) pf[i] = (half_t)(sub == 0 ? s0[8 * sp + i] : s1[8 * sp + i]);
        const int kb = sub * 32 + 16 * sp + 4 * hh;   // keys kb..kb+3 and kb+8..kb+11 <-> regs 8sp..8sp+7
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const half_t* vr = sVt + (f * 32 + l31) * ATC64_VSTR + kb;
          const half4 v0 = *(const half4*)vr, v1 = *(const half4*)(vr + 8);
          const half8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
          o[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[f], 0, 0, 0);
        }
      }
    }
  }
  if (wave_active && qpos < L) {
    // a query always sees its own key, so l_run > 0
    const float inv = 1.0f / l_run;
    half_t* dst = p.ctx + (size_t)(tok0 + qpos) * p.ldctx + h * 64;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        half4 a;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = f2h_sat(o[f][4 * q + j] * inv);
        *(half4*)(dst + f * 32 + 8 * q + 4 * hh) = a;
      }
  }
}

// =========================== incremental decoding: one new row per sequence against a K / V cache ===========================
// Per layer K [rows][n_kv][P][64] then V, fp16, the keys of one kv head contiguous.  kv_cache_fill64_kernel copies the prompt's
// rows out of the prefill's fused QKV buffer (after rope64_kernel); grid = (longest prompt, n_seq), a thread moves one 16-byte
// piece of K and of V.
__global__ __launch_bounds__(256) void kv_cache_fill64_kernel(const half_t* __restrict__ qkv, const int* __restrict__ seq_off,
                                                              half_t* __restrict__ kc, half_t* __restrict__ vc, int ld,
                                                              int n_heads, int n_kv, int P) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int tok0 = seq_off[b];
  if (t >= seq_off[b + 1] - tok0 || t >= P) return;
  const half_t* row = qkv + (size_t)(tok0 + t) * ld + (size_t)n_heads * 64;
  for (int c = threadIdx.x; c < n_kv * 8; c += 256) {
    const int h = c >> 3, piece = (c & 7) * 8;
    const size_t dst = (((size_t)b * n_kv + h) * P + t) * 64 + piece;
    *(half8*)(kc + dst) = *(const half8*)(row + h * 64 + piece);
    *(half8*)(vc + dst) = *(const half8*)(row + (size_t)(n_kv + h) * 64 + piece);
  }
}

// The decoding session's fill (rk_llama_session_admit): sequence b of the call goes to cache row slots[b].
__global__ __launch_bounds__(256) void kv_cache_fill64_slots_kernel(const half_t* __restrict__ qkv, const int* __restrict__ seq_off,
                                                                    const int* __restrict__ slots, int n_slots,
                                                                    half_t* __restrict__ kc, half_t* __restrict__ vc, int ld,
                                                                    int n_heads, int n_kv, int P) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int tok0 = seq_off[b], slot = slots[b];
  if (t >= seq_off[b + 1] - tok0 || t >= P || slot < 0 || slot >= n_slots) return;
  const half_t* row = qkv + (size_t)(tok0 + t) * ld + (size_t)n_heads * 64;
  for (int c = threadIdx.x; c < n_kv * 8; c += 256) {
    const int h = c >> 3, piece = (c & 7) * 8;
    const size_t dst = (((size_t)slot * n_kv + h) * P + t) * 64 + piece;
    *(half8*)(kc + dst) = *(const half8*)(row + h * 64 + piece);
    *(half8*)(vc + dst) = *(const half8*)(row + (size_t)(n_kv + h) * 64 + piece);
  }
}

#define LDC64_PSTR 68    // floats per partial of a 64-wide head: 64 accumulators, maximum, sum, 2 unused (16-byte rows)

__device__ __forceinline__ float row8_sum_f(float v) {   // sum over an aligned group of 8 lanes, every lane gets it; fixed order
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// Single-token attention over the cache, d = 64: the contract of attn_dec_cached128_body (AttnDecCached128Args with every 128
// read as 64: caches [rows][n_kv][P][64], tables [max_pos][32], bias [(n_heads + 2 n_kv) * 64], part [rows][n_heads][nch][LDC64_PSTR],
// ctx [rows, n_heads * 64]).  grid = (key chunks of the longest cache, n_heads / R, rows), 256 threads.  A workgroup takes ONE
// chunk of LDC_CHUNK keys - FIXED, cut from the row's own position - of one kv head and R query heads that share it.  K / V go
// straight to registers: a lane holds 8 of a key's 64 dims, 8 lanes a key, a wave 8 keys per load and 32 keys in all, every load
// issued before the first use.  The new row is rotated here by rope64_pairs - rope64_kernel's arithmetic on the same table
// entries, so the key a step writes is bit for bit the key a prefill writes for that token - and its key and value are written
// by the workgroup that owns the position's chunk, once per kv head.  Each workgroup leaves one (maximum, sum, 64 accumulators)
// partial per head - its four waves merged in wave order - and attn_dec_combine64_kernel merges a row's chunks in key order.
// A head's arithmetic does not depend on R (every per-head array is indexed by r alone, the merge is per head).
template <int R, bool BIAS>
__device__ __forceinline__ void attn_dec_cached64_body(const AttnDecCached128Args& p) {
  __shared__ float s_m[4][R], s_l[4][R];
  __shared__ __attribute__((aligned(16))) float s_acc[4][R][64];
  const int ch = blockIdx.x, h0 = blockIdx.y * R, b = blockIdx.z;
  int pos = p.pos[b];
  pos = pos < 0 ? 0 : (pos < p.P - 1 ? pos : p.P - 1);   // (the host keeps it inside the cache; the clamp keeps a bad word from faulting)
  const int key0 = ch * LDC_CHUNK;
  if (key0 > pos) return;                                 // uniform: this chunk lies beyond the row's keys
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kg = lane >> 3, c = lane & 7;
  const int G = p.n_heads / p.n_kv, kvh = h0 / G;
  const half_t* row = p.qkv + (size_t)b * p.ld;
  const int i0 = (c & 3) * 8;
  const bool hi = c >= 4;                                 // this lane's dims are in the second half of the head
  float co[8], si[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { co[j] = p.cos_t[(size_t)pos * 32 + i0 + j]; si[j] = p.sin_t[(size_t)pos * 32 + i0 + j]; }
  // this lane's 8 dims of rotated head hd (of q | k), rounded as rope64_kernel does
  auto rotated = [&](int hd) {
    half8 oa, ob;
    rope64_pairs<BIAS>(row + (size_t)hd * 64, BIAS ? p.bias + (size_t)hd * 64 : nullptr, i0, co, si, oa, ob);
    return hi ? ob : oa;
  };
  const half8 knew = rotated(p.n_heads + kvh);
  const size_t voff = (size_t)(p.n_heads + p.n_kv + kvh) * 64 + c * 8;
  half8 vnew = *(const half8*)(row + voff);
  if constexpr (BIAS) vnew = bias_v8(vnew, p.bias + voff);
  half_t* kbase = p.kc + ((size_t)b * p.n_kv + kvh) * p.P * 64 + c * 8;
  half_t* vbase = p.vc + ((size_t)b * p.n_kv + kvh) * p.P * 64 + c * 8;
  if (pos - key0 < LDC_CHUNK && h0 % G == 0 && wave == 0 && kg == 0) {   // the position's chunk, once per kv head
    *(half8*)(kbase + (size_t)pos * 64) = knew;
    *(half8*)(vbase + (size_t)pos * 64) = vnew;
  }
  const int wkey0 = key0 + wave * 32;
  float m_w[R], l_w[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m_w[r] = -1e30f; l_w[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
  }
  if (wkey0 <= pos) {                                     // wave-uniform
    half8 kf[4], vf[4];
    const int last_old = pos > 0 ? pos - 1 : 0;           // keys before the new one come from the cache
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = wkey0 + 8 * i + kg;
      const int idx = key < last_old ? key : last_old;
      kf[i] = *(const half8*)(kbase + (size_t)idx * 64);
      vf[i] = *(const half8*)(vbase + (size_t)idx * 64);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool is_new = wkey0 + 8 * i + kg >= pos;
      kf[i] = is_new ? knew : kf[i];
      vf[i] = is_new ? vnew : vf[i];
    }
    float s[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const half8 q = rotated(h0 + r);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = __builtin_fmaf((float)q[j], (float)kf[i][j], d);
        d = row8_sum_f(d) * p.scale_log2e;
        s[r][i] = wkey0 + 8 * i + kg <= pos ? d : -1e30f;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mx = s[r][0];
#pragma unroll
      for (int i = 1; i < 4; ++i) mx = fmaxf(mx, s[r][i]);
      mx = fmaxf(mx, __shfl_xor(mx, 8));
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pr = __builtin_amdgcn_exp2f(s[r][i] - mx);   // masked keys: exp2(-1e30) = 0
        sum += pr;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_fmaf(pr, (float)vf[i][j], acc[r][j]);
      }
      sum += __shfl_xor(sum, 8);
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        acc[r][j] += __shfl_xor(acc[r][j], 8);
        acc[r][j] += __shfl_xor(acc[r][j], 16);
        acc[r][j] += __shfl_xor(acc[r][j], 32);
      }
      m_w[r] = mx; l_w[r] = sum;
    }
  }
  if (kg == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      *(f32x4*)&s_acc[wave][r][c * 8] = f32x4{acc[r][0], acc[r][1], acc[r][2], acc[r][3]};
      *(f32x4*)&s_acc[wave][r][c * 8 + 4] = f32x4{acc[r][4], acc[r][5], acc[r][6], acc[r][7]};
      if (c == 0) { s_m[wave][r] = m_w[r]; s_l[wave][r] = l_w[r]; }
    }
  }
  __syncthreads();
  if (tid < 64) {                                         // the four waves' partials, merged in wave order
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float M = fmaxf(fmaxf(s_m[0][r], s_m[1][r]), fmaxf(s_m[2][r], s_m[3][r]));
      float L = 0.f, A = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float f = __builtin_amdgcn_exp2f(s_m[w][r] - M);
        L = __builtin_fmaf(s_l[w][r], f, L);
        A = __builtin_fmaf(s_acc[w][r][tid], f, A);
      }
      float* dst = p.part + (((size_t)b * p.n_heads + h0 + r) * p.nch + ch) * LDC64_PSTR;
      dst[tid] = A;
      if (tid == 0) { dst[64] = M; dst[65] = L; }
    }
  }
}

template <int R>
__global__ __launch_bounds__(256) void attn_dec_cached64_kernel(AttnDecCached128Args p) { attn_dec_cached64_body<R, false>(p); }
template <int R>
__global__ __launch_bounds__(256) void attn_dec_cached64_bias_kernel(AttnDecCached128Args p) { attn_dec_cached64_body<R, true>(p); }

// Merges the chunk partials of one (sequence, head) in key order and writes the fp16 context.  grid = (n_heads, rows), 64
// threads = the head's 64 dims.
__global__ __launch_bounds__(64) void attn_dec_combine64_kernel(AttnDecCached128Args p) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int pos = p.pos[b];
  pos = pos < 0 ? 0 : (pos < p.P - 1 ? pos : p.P - 1);
  const int n = pos / LDC_CHUNK + 1;
  const float* src = p.part + ((size_t)b * p.n_heads + h) * p.nch * LDC64_PSTR;
  float M = -1e30f;
  for (int k = 0; k < n; ++k) M = fmaxf(M, src[(size_t)k * LDC64_PSTR + 64]);
  float L = 0.f, A = 0.f;
  for (int k = 0; k < n; ++k) {
    const float f = __builtin_amdgcn_exp2f(src[(size_t)k * LDC64_PSTR + 64] - M);
    L = __builtin_fmaf(src[(size_t)k * LDC64_PSTR + 65], f, L);
    A = __builtin_fmaf(src[(size_t)k * LDC64_PSTR + d], f, A);
  }
  p.ctx[(size_t)b * p.n_heads * 64 + h * 64 + d] = f2h_sat(A / L);   // a row always sees its own key: L > 0
}
