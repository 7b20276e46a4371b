// Decoder-only (Llama family) kernels for gfx950: rotary position embedding and causal grouped-query attention with
// head_dim = 128 (every Llama-2/3 size), and the decode step against a K / V cache for head_dim = 128 and 64 (the rest of the
// 64-wide kernels: llama_kernels_hd64.h).  Everything else of the Llama forward - RMSNorm (folded), the QKV / O / gate-up /
// down projections (SwiGLU epilogue), the final-token head - runs on the kernels the T5 path already uses.
//
// Semantics restated from hf: models/llama/modeling_llama.py: apply_rotary_pos_emb :137-160 (rotate_half pairs element i
// with i + head_dim/2), eager_attention_forward :192-214 (scaling = head_dim**-0.5, causal mask, fp32 softmax),
// repeat_kv :180-189 (query head h reads kv head h / (n_heads / n_kv_heads)).
#pragma once
#include "common.h"
#include "xcd_map.h"

// The q / k / v projection bias of the Qwen2 family (hf: models/qwen2/modeling_qwen2.py: Qwen2Attention, q_proj / k_proj / v_proj
// with bias=True): fp32, added to the fp16 GEMM output.  It cannot be folded into the weights - the QKV GEMM multiplies its
// output by the folded RMSNorm's row factor, the bias comes after that - so it is added where the row is touched next: here (prefill)
// and in attn_dec_cached_kernel's row load (decode step), by THESE helpers, so that both form the same bits.
__device__ __forceinline__ void bias_add8(float (&x)[8], const half8 a, const float* __restrict__ b) {
  const f32x4 b0 = *(const f32x4*)b, b1 = *(const f32x4*)(b + 4);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = (float)a[j] + (j < 4 ? b0[j & 3] : b1[j & 3]);
}
__device__ __forceinline__ half8 bias_v8(const half8 a, const float* __restrict__ b) {   // a value row's 8 dims: one rounding
  float x[8];
  bias_add8(x, a, b);
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = f2h_sat(x[j]);
  return o;
}

// One rotated pair, in a FIXED form (no contraction left to the compiler): `fused` = both results as one fma over a rounded
// product, lo = fma(cos, x1, -(sin x2)) and up = fma(cos, x2, sin x1), else two rounded products and an add.  EVERY 128-wide caller,
// with and without the bias - the prefill's q and k, the step's new key and its queries, the drafting step's append - passes
// fused = (element 0 of the thread's eight), so a step rounds a row exactly as a prefill does: the cached key IS the prefill's key
// by construction, and a prefill with an all-zero bias gives the bias-free bits except the sign of a zero (-0 + 0.0f = +0: the
// bias-free kernels add nothing; tests/test_gpu_rope_forms.py asserts exactly that).  Why element 0: that is what a compiler once
// made of the bias-free rope128_kernel's plain expression (one v_fma_mix, seven packed multiplies + add), the bits the prefill
// always had.  The step kernels' copies of that expression had come out otherwise (up = fma(sin, x1, cos x2)), one fp16 ulp from
// the prefill's key on about 1.3e-4 of those elements: hence one form in source.
__device__ __forceinline__ void rope_rot(float x1, float x2, float co, float si, bool fused, float& lo, float& hi) {
#pragma clang fp contract(off)
  if (fused) { lo = __builtin_fmaf(co, x1, -(si * x2)); hi = __builtin_fmaf(co, x2, si * x1); }
  else { lo = co * x1 - si * x2; hi = co * x2 + si * x1; }
}
// ONE of rope_rot's two results, for a caller that keeps one half of the head (the step's lanes): with (u, w) = (x1, -x2) it is
// `lo`, with (x2, x1) it is `hi`, bit for bit - fl(si * -x2) = -fl(si * x2), and a - b is a + (-b) in IEEE arithmetic, zeros'
// signs included.  Half the multiplies of rope_rot for such a lane.
__device__ __forceinline__ float rope_rot_half(float u, float w, float co, float si, bool fused) {
#pragma clang fp contract(off)
  return fused ? __builtin_fmaf(co, u, si * w) : co * u + si * w;
}

// In place on the fused QKV buffer [T, ld]: the first n_rot heads of a row (all query heads, then all key heads) are
// rotated by the row's position.  cos / sin: [max_pos, 64] fp32 (the two halves of HF's table are equal).
// One workgroup per token; a thread takes 8 consecutive pairs of one head: 16-byte accesses.
// BIAS (Qwen2): bias [(n_rot + n_v) * 128] fp32 in q | k | v order is added to the fp16 GEMM output before the rotation - ONE
// fp16 rounding for q and k, after bias and rotation - and to the n_v value heads behind them (touched only here).  BIAS = false
// rotates the widened fp16 values by the same rope_rot calls: the bits the Llama kernel always gave, now written down.
template <bool BIAS>
__global__ __launch_bounds__(256) void rope128_kernel(half_t* __restrict__ qkv, const int* __restrict__ pos,
                                                      const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                      int ld, int n_rot, const float* __restrict__ bias, int n_v) {
  const int t = blockIdx.x;
  const int p = pos[t];
  half_t* row = qkv + (size_t)t * ld;
  const float* cr = cos_t + (size_t)p * 64;
  const float* sr = sin_t + (size_t)p * 64;
  for (int c = threadIdx.x; c < n_rot * 8; c += 256) {
    const int head = c >> 3, i0 = (c & 7) * 8;
    half_t* x = row + head * 128 + i0;
    const half8 a = *(const half8*)x, b = *(const half8*)(x + 64);
    half8 oa, ob;
    float xa[8], xb[8];
    if constexpr (BIAS) {
      bias_add8(xa, a, bias + head * 128 + i0);
      bias_add8(xb, b, bias + head * 128 + 64 + i0);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) { xa[j] = (float)a[j]; xb[j] = (float)b[j]; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {                    // q * cos + rotate_half(q) * sin: first half -x2, second half +x1
      float lo, hi;
      rope_rot(xa[j], xb[j], cr[i0 + j], sr[i0 + j], j == 0, lo, hi);
      oa[j] = f2h_sat(lo);
      ob[j] = f2h_sat(hi);
    }
    *(half8*)x = oa;
    *(half8*)(x + 64) = ob;
  }
  if constexpr (BIAS) {
    for (int c = threadIdx.x; c < n_v * 16; c += 256) {
      const int off = (n_rot + (c >> 4)) * 128 + (c & 15) * 8;
      *(half8*)(row + off) = bias_v8(*(const half8*)(row + off), bias + off);
    }
  }
}

struct AttnCausalArgs {
  const half_t* qkv;     // [T, ld]: q heads at column 0, k heads at n_heads*D, v heads at (n_heads + n_kv)*D (D = head_dim)
  half_t* ctx;           // [T, ldctx] (n_heads * D columns)
  const int* seq_off;    // [B+1]
  int ld, ldctx, n_heads, n_kv;
  float scale_log2e;     // head_dim**-0.5 * log2(e): the softmax runs in the log2 domain
  int n_seq, nqb;        // attn_causal_dma_kernel (1-D grid): sequences, query blocks of 32 NW of the longest sequence
  int ko;                // attn_causal_dma_kernel, measurement builds only (-DRK_MEASURE): timing knock-outs, see ATCD_KO
};
struct AttnCausalWinArgs : AttnCausalArgs {   // the windowed entries' arguments; the plain kernels' struct stays what it was
  int window;            // Mistral's sliding window: W > 0, query i sees keys max(0, i - W + 1) .. i
};
// The two prefill kernels below take WIN as a template parameter: WIN = 0 is the plain kernel over AttnCausalArgs, WIN = 1 the
// windowed entry over AttnCausalWinArgs.  The windowed form differs from the plain one in the 64-key tiles (chunks) it skips and
// the keys it masks, nothing else: the walk starts at the first tile that holds a visible key of the block's first query, a wave
// skips a tile that ends below its first query's bound, and a tile that starts below the bound of the wave's last query inside
// the sequence gets the lower mask - the causal edge's -1e30.  So a sequence no longer than W runs the very tile bodies the plain
// kernel runs and gets its bits.  (A lane whose keys of a tile are ALL below its bound - the tile is another lane's - forms
// weights exp2(0) = 1 against its maximum of -1e30; its own first visible tile comes later, moves the maximum to a real score and
// multiplies all of that by alpha = exp2(-1e30 - m) = 0, exactly.)
template <bool WIN> using AttnCausalArgsOf = std::conditional_t<WIN, AttnCausalWinArgs, AttnCausalArgs>;

// Flash-style causal attention staged through registers, D = head_dim (128 or 64): ONE kernel for every sequence length.  q heads
// at column 0, k heads at n_heads*D, v heads at (n_heads + n_kv)*D, ctx [T, ldctx] of n_heads*D columns.
// grid = (ceil(maxL / 128), n_heads, B); 256 threads = 4 waves x 32 queries.  Per 64-key tile: K rows and V TRANSPOSED are staged
// in LDS (17.5 KiB at D = 64); S^T = K Q^T by MFMA 32x32x16 (D / 16 k16 steps; A = K rows, B = Q^T) so a lane owns ONE query column
// and the online-softmax state is per-lane scalars; the fp16 probabilities are already in B-operand position for O^T = V^T P^T
// (D / 32 32-row d fragments).  Tiles above the diagonal are skipped, the diagonal tile is masked per lane.  A row's arithmetic
// depends on its own sequence only (its position, its keys in tiles of 64 in order): batch-independent.
#define ATC_KPAD 8     // sK row stride in halfs is D + 8 (144 / 272 B: 16-B aligned)
#define ATC_VSTR 68    // sVt row stride in halfs (136 B: 8-B aligned)
template <int D, bool WIN>
__global__ __launch_bounds__(256) void attn_causal_tile_kernel(AttnCausalArgsOf<WIN> p) {
  constexpr int KSTR = D + ATC_KPAD, C8 = D / 8;             // C8: the 16-byte pieces of a row
  __shared__ __attribute__((aligned(16))) half_t sK[64 * KSTR];
  __shared__ __attribute__((aligned(16))) half_t sVt[D * ATC_VSTR];
  const int b = blockIdx.z, h = blockIdx.y, qt = blockIdx.x;
  const int tok0 = p.seq_off[b];
  const int L = p.seq_off[b + 1] - tok0;
  if (qt * 128 >= L) return;   // uniform for the whole block
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hh = lane >> 5, l31 = lane & 31;
  const int kvh = h / (p.n_heads / p.n_kv);
  const half_t* kbase = p.qkv + (size_t)(p.n_heads + kvh) * D;
  const half_t* vbase = p.qkv + (size_t)(p.n_heads + p.n_kv + kvh) * D;
  const int q0 = qt * 128 + wave * 32;
  const bool wave_active = q0 < L;
  const int qpos = q0 + l31;
  const int qrow = qpos < L ? qpos : L - 1;
  half8 qf[D / 16];
  {
    const half_t* qptr = p.qkv + (size_t)(tok0 + qrow) * p.ld + h * D + 8 * hh;
#pragma unroll
    for (int s = 0; s < D / 16; ++s) qf[s] = *(const half8*)(qptr + 16 * s);
  }
  f32x16 o[D / 32];
#pragma unroll
  for (int f = 0; f < D / 32; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[f][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const int last_q = min(qt * 128 + 127, L - 1);
  const int nkt = (last_q >> 6) + 1;                 // key tiles this block of queries can see (causal)
  int window = 0, kt0 = 0, wlo = 0, wlo_last = 0;
  if constexpr (WIN) {
    window = p.window;
    kt0 = max(qt * 128 - window + 1, 0) >> 6;        // the first tile the block's first query sees
    wlo = q0 - window + 1;                           // lower bound of the wave's first query (its lowest)
    wlo_last = min(q0 + 31, L - 1) - window + 1;     // ... of its last query inside the sequence (its highest)
  }
  for (int kt = kt0; kt < nkt; ++kt) {
    __syncthreads();                                   // the previous tile's fragments are read
    // ---- stage K (row-major) and V^T (key pairs) of keys kt*64 .. kt*64+63; rows beyond L are clamped copies (masked) ----
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
      const int c = tid + 256 * i, row = c / C8, cc = c % C8;
      const int key = min(kt * 64 + row, L - 1);
      *(half8*)(sK + row * KSTR + cc * 8) = *(const half8*)(kbase + (size_t)(tok0 + key) * p.ld + cc * 8);
    }
#pragma unroll
    for (int i = 0; i < D / 64; ++i) {
      const int c = tid + 256 * i, kp = c / C8, cc = c % C8;
      const int k0 = min(kt * 64 + 2 * kp, L - 1), k1 = min(kt * 64 + 2 * kp + 1, L - 1);
      const half8 v0 = *(const half8*)(vbase + (size_t)(tok0 + k0) * p.ld + cc * 8);
      const half8 v1 = *(const half8*)(vbase + (size_t)(tok0 + k1) * p.ld + cc * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const half2v pr = {v0[j], v1[j]};
        *(half2v*)(sVt + (cc * 8 + j) * ATC_VSTR + 2 * kp) = pr;
      }
    }
    __syncthreads();
    if (!wave_active || kt * 64 > q0 + 31) continue;    // this wave's queries see none of these keys
    if (WIN && kt * 64 + 63 < wlo) continue;            // nor of these: the tile ends below the window of every one of them
    const bool need_low = WIN && kt * 64 < wlo_last;    // the tile starts below the window of the wave's last query
    f32x16 s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      const half8 k0 = *(const half8*)(sK + l31 * KSTR + 16 * s + 8 * hh);
      const half8 k1 = *(const half8*)(sK + (32 + l31) * KSTR + 16 * s + 8 * hh);
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
      if (need_low) {
        const int key0 = key_base + (r & 3) + 8 * (r >> 2), lo = qpos - window + 1;
        s0[r] = key0 >= lo ? s0[r] : -1e30f;
        s1[r] = key0 + 32 >= lo ? s1[r] : -1e30f;
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
    for (int f = 0; f < D / 32; ++f)
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
        for (int f = 0; f < D / 32; ++f) {
          const half_t* vr = sVt + (f * 32 + l31) * ATC_VSTR + kb;
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
    half_t* dst = p.ctx + (size_t)(tok0 + qpos) * p.ldctx + h * D;
#pragma unroll
    for (int f = 0; f < D / 32; ++f)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        half4 a;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = f2h_sat(o[f][4 * q + j] * inv);
        *(half4*)(dst + f * 32 + 8 * q + 4 * hh) = a;
      }
  }
}

// The same attention by the recipe of the long-sequence T5 kernel (attention.h: attn_enc_long_kernel), for d = 128 (round 5;
// engine option llama_attn_dma = 1, the default).  The kernel above stages every 64-key tile through registers - K row-major,
// V through sixteen 4-byte transposing LDS writes per thread - between two barriers that leave the memory pipe idle while the
// tile is computed: 220 TF/s on a 1 536-token prompt.  Here the K and V rows of a 64-key chunk arrive by LDS-DMA
// (global_load_lds_dwordx4) into one of two 32-KiB stages while the previous chunk is computed (ONE barrier per chunk, behind a
// wait that has had a whole chunk of compute to be satisfied); a 128-column row is kept as TWO 64-column images in the T5
// kernels' layout ([64 keys][64 halves], the eight 16-byte slots of a row permuted by ATTD_SWZ on the SOURCE address), so the K
// fragments are conflict-free ds_read_b128 and the V^T fragments come from ds_read_b64_tr_b16 (attd_issue_vt) - no transpose
// is ever written.  S^T = K Q^T as before (a lane owns one query column), log2-domain online softmax per chunk with the
// packed-fp32 / v_max3 helpers of attention.h, the two half-rows of a query (lane, lane ^ 32) exchanged by
// v_permlane32_swap; the 64 accumulator registers are rescaled only when some lane's running maximum moved (alpha == 1 for
// every lane otherwise: the same bits); context rows leave as 16-byte stores.  64 KiB of LDS, <= 256 VGPRs: two workgroups per
// CU.  grid = ceil(B n_kv / 8) x 8 x (n_heads / n_kv) x ceil(maxL / 128) workgroups (see the mapping below); 256 threads = 4 waves x 32 queries.
// A row's arithmetic depends on its own sequence only (its position, its keys in chunks of 64 in order): batch-independent.
// timing-only knock-outs (measurement builds: hipcc ... -DRK_MEASURE, loaded through RK_ENGINE_LIB; results are garbage):
// AttnCausalArgs::ko bit 0 no K / V DMA inside the chunk loop, 1 no score MFMAs, 2 no softmax (scale, maximum, exp, merge),
// 3 no P V, 4 no workgroup barrier per chunk, 5 no context stores, 6 return at once, 7 return after the prologue.  tools/llama_attn_ko.py
#ifdef RK_MEASURE
#define ATCD_KO(bit) ((p.ko >> (bit)) & 1)
#else
#define ATCD_KO(bit) 0
#endif
#define ATCD_KEYS 64
#define ATCD_IMG_HALFS (ATCD_KEYS * 64)            // one image: 8 KiB
#define ATCD_STAGE_HALFS (4 * ATCD_IMG_HALFS)      // K columns 0-63 | K columns 64-127 | V columns 0-63 | V columns 64-127
#define ATCD_LDS_BYTES (2 * ATCD_STAGE_HALFS * 2)
// NW waves x 32 queries per workgroup (4 or 8): a query row's arithmetic does not depend on NW - the same chunks of 64 keys in the
// same order, the same per-wave decisions - so the host may pick it freely (8: two waves per SIMD inside ONE workgroup, each
// K / V chunk fetched once for 256 queries; 4: twice the workgroups, shorter critical path of the last query block)
// The windowed form (WIN, see AttnCausalArgsOf above): the chunk walk starts at ch0 = the first chunk that holds a visible key of
// the block's first query: the prologue issues chunk ch0 into stage ch0 & 1 and drains it (vmcnt(0), barrier) exactly as the plain
// kernel does chunk 0, and the loop's accounting is unchanged - one chunk in flight, drained at the end of every iteration, stage
// = ch & 1.  The lower mask is a second compile-time flag of the chunk body (LOW), so a sequence no longer than W runs the very
// chunk bodies the plain kernel runs.  (The lane whose chunk is ALL below its bound: alpha = 0 != 1, so the accumulators are rescaled.)
template <int NW, bool WIN>
__global__ __launch_bounds__(64 * NW, 2) void attn_causal_dma_kernel(AttnCausalArgsOf<WIN> p) {
  constexpr int ATCD_QUERIES = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) unsigned char atcd_smem[];
  half_t* const sbuf = (half_t*)atcd_smem;
  // workgroup -> (sequence, head, query block), XCD-aware: consecutive workgroups go to the 8 XCDs in turn, each with its own
  // L2, so workgroup i belongs to the (sequence, kv head) group 8 (i / 8 / W) + i % 8 - all W = heads-per-group x query-blocks
  // workgroups that read one K / V pair (0.8 MB at 1.5k tokens) meet in ONE L2 instead of each XCD pulling every pair through the
  // fabric - and walks that group's query blocks from the last (most keys) to the first, the heads of a kv head side by side
  const int hpg = p.n_heads / p.n_kv, W = hpg * p.nqb;
  int grp, w;
  if (!xcd_decode((int)blockIdx.x, p.n_seq * p.n_kv, W, grp, w)) return;   // uniform for the whole block (xcd_map.h)
  const int b = grp / p.n_kv, kvh = grp % p.n_kv, h = kvh * hpg + w % hpg, qb = p.nqb - 1 - w / hpg;
  const int tok0 = p.seq_off[b];
  const int L = p.seq_off[b + 1] - tok0;
  const int Q0 = qb * ATCD_QUERIES;
  if (Q0 >= L) return;                                       // uniform for the whole block
  if (ATCD_KO(6)) return;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int q0 = Q0 + wave * 32;
  const bool active = q0 < L;                                // wave-uniform
  const half_t* const kbase = p.qkv + (size_t)(p.n_heads + kvh) * 128;
  const half_t* const vbase = p.qkv + (size_t)(p.n_heads + p.n_kv + kvh) * 128;
  const int last_q = min(Q0 + ATCD_QUERIES - 1, L - 1);
  const int nch = (last_q >> 6) + 1;                         // chunks this block of queries can see (causal)
  // (all of the window's values are formed HERE and only under WIN: inside a generic lambda p.window would be looked up for
  // WIN = 0 too, and even a dead min() outside this block moved the plain kernel's scalar prologue)
  int window = 0, ch0 = 0, wlo = 0, wlo_last = 0;
  if constexpr (WIN) {
    window = p.window;
    ch0 = max(Q0 - window + 1, 0) >> 6;                      // the first chunk the block's first query sees
    wlo = q0 - window + 1;                                   // lower bound of the wave's first query (its lowest)
    wlo_last = min(q0 + 31, L - 1) - window + 1;             // ... of its last query inside the sequence (its highest)
  }
  auto opaque_lane = [&]() {
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    return lane;
  };
  struct LaneCtx { int hh, l31, qpos, kfo0, vfo0; };
  auto lane_ctx = [&](int lane) {
    LaneCtx c;
    c.hh = lane >> 5; c.l31 = lane & 31; c.qpos = q0 + c.l31;
    c.kfo0 = c.l31 * 64 + ((c.hh ^ ATTD_SWZ(c.l31)) << 3);
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
    c.vfo0 = (4 * c.hh + (i16 >> 2)) * 64 + (((2 * g1 + ((i16 & 3) >> 1)) ^ ((((i16 >> 3) & 1) << 2) | c.hh)) << 3) + 4 * (i16 & 1);
    return c;
  };
  // chunk ch -> stage st: 32 pieces of 64 sixteen-byte slots (8 per image), 32 / NW per wave; keys beyond the sequence are
  // clamped copies of its last row (never visible to a valid query: causal)
  auto issue_chunk = [&](int lane, int ch, int st) {
#pragma unroll
    for (int k = 0; k < 32 / NW; ++k) {
      const int pid = wave + NW * k, img = pid >> 3, sub = pid & 7;
      const int slot = sub * 64 + lane, r = slot >> 3, c = slot & 7;
      int key = ch * ATCD_KEYS + r;
      key = key < L ? key : L - 1;
      const char* hb = (const char*)((img < 2 ? kbase : vbase) + (img & 1) * 64);
      const unsigned off = ((unsigned)(tok0 + key) * (unsigned)p.ld + ((c ^ ATTD_SWZ(r)) << 3)) * 2u;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(hb + off),
                                       (__attribute__((address_space(3))) void*)(sbuf + st * ATCD_STAGE_HALFS + img * ATCD_IMG_HALFS + sub * 512),
                                       16, 0, 0);
    }
  };

  // ---- prologue: this lane's Q fragments (8 k16 steps), chunk 0 ----
  half8 qf[8];
  {
    const LaneCtx c = lane_ctx(opaque_lane());
    const int qrow = c.qpos < L ? c.qpos : L - 1;
    const half_t* qptr = p.qkv + (size_t)(tok0 + qrow) * p.ld + h * 128 + 8 * c.hh;
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *(const half8*)(qptr + 16 * s);
  }
  issue_chunk(opaque_lane(), ch0, ch0 & 1);                  // (the stage of chunk ch is ch & 1 throughout)
  // (the Q fragments are "used" here so that the compiler's wait for these tracked loads sits in front of the chunk loop and
  // not at their first MFMA inside it, where it would drain the DMA queue of every chunk)
  asm volatile("" :: "v"(qf[0]), "v"(qf[1]), "v"(qf[2]), "v"(qf[3]), "v"(qf[4]), "v"(qf[5]), "v"(qf[6]), "v"(qf[7]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (ATCD_KO(7)) return;

  f32x16 o[4];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[f][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;                         // l_run: this lane's half of the row sum (the halves meet at the end)

  // scores of the chunk: 8 k16 steps (4 per image) x two 32-key halves; the K fragments of step i + 1 requested before the MFMAs of step i
  auto qk_chunk = [&](const LaneCtx& c, const half_t* kst, f32x16& s0, f32x16& s1) {
    const half_t* kb_ = kst + c.kfo0;
    half8 kf[2][2];
    auto fetch = [&](int i, half8 (&d)[2]) {
      const half_t* a = kb_ + (i >> 2) * ATCD_IMG_HALFS + ((c.kfo0 ^ ((i & 3) << 4)) - c.kfo0);
      d[0] = *(const half8*)a;
      d[1] = *(const half8*)(a + 32 * 64);
    };
    fetch(0, kf[0]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i + 1 < 8) fetch(i + 1, kf[(i + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
      if (i == 0) {
        f32x16 z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        s0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[0][0], qf[0], z, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[0][1], qf[0], z, 0, 0, 0);
      } else {
        s0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[i & 1][0], qf[i], s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[i & 1][1], qf[i], s1, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // O^T += V^T P^T for one 64-column image of the chunk's V rows (the T5 kernels' pv_tile: transposing reads a k16 step ahead
  // of their MFMAs, counted lgkmcnt); oa / ob: output columns 0-31 / 32-63 of the image
  auto pv_image = [&](const LaneCtx& c, const half_t* vimg, const unsigned (&pp)[16], f32x16& oa, f32x16& ob) {
    const unsigned vb0 = (unsigned)(size_t)(const __attribute__((address_space(3))) half_t*)vimg;
    unsigned va[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) va[i] = vb0 + 2u * (unsigned)(c.vfo0 ^ (16 * i));
    half4 v[2][4];
    auto step = [&](auto gc, half4 (&d)[4]) {
      constexpr int g = decltype(gc)::value, sub = g >> 1, sp = g & 1;
      const attd_u32x4 pu = {pp[8 * sub + 4 * sp], pp[8 * sub + 4 * sp + 1], pp[8 * sub + 4 * sp + 2], pp[8 * sub + 4 * sp + 3]};
      const half8 pf = __builtin_bit_cast(half8, pu);
      if constexpr (g < 3) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]));
      else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]));
      __builtin_amdgcn_sched_barrier(0);
      const half8 vf0 = {d[0][0], d[0][1], d[0][2], d[0][3], d[1][0], d[1][1], d[1][2], d[1][3]};
      const half8 vf1 = {d[2][0], d[2][1], d[2][2], d[2][3], d[3][0], d[3][1], d[3][2], d[3][3]};
      oa = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf0, pf, oa, 0, 0, 0);
      ob = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf1, pf, ob, 0, 0, 0);
    };
    using std::integral_constant;
    attd_issue_vt<0>(v[0], va);
    attd_issue_vt<1>(v[1], va);
    step(integral_constant<int, 0>{}, v[0]);
    attd_issue_vt<2>(v[0], va);
    step(integral_constant<int, 1>{}, v[1]);
    attd_issue_vt<3>(v[1], va);
    step(integral_constant<int, 2>{}, v[0]);
    step(integral_constant<int, 3>{}, v[1]);
  };

  // one chunk of a wave that sees some of its keys.  MASK: the chunk reaches past the wave's first query (the diagonal);
  // LOW (WIN only): the chunk starts below the window of the wave's last query
  auto chunk_body = [&](auto maskc, auto lowc, int ch, int st) {
    constexpr bool MASK = decltype(maskc)::value, LOW = decltype(lowc)::value;
    const half_t* kst = sbuf + st * ATCD_STAGE_HALFS;
    f32x16 s0, s1;
    if (!ATCD_KO(1)) qk_chunk(lane_ctx(opaque_lane()), kst, s0, s1);
    else {
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
      asm volatile("" : "+v"(s0), "+v"(s1));
    }
    __builtin_amdgcn_sched_barrier(0);
    float tmax = -1e30f;
    if (!ATCD_KO(2)) {
      const LaneCtx c1 = lane_ctx(opaque_lane());
      const int key_base = ch * ATCD_KEYS + 4 * c1.hh;       // register r <-> key key_base + (r & 3) + 8 (r >> 2) (+ 32 for s1)
      const f32x2 sc = {p.scale_log2e, p.scale_log2e};
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f32x2 t0 = f32x2{s0[r], s0[r + 1]} * sc, t1 = f32x2{s1[r], s1[r + 1]} * sc;
        s0[r] = t0[0]; s0[r + 1] = t0[1]; s1[r] = t1[0]; s1[r + 1] = t1[1];
        if (MASK) {
#pragma unroll
          for (int j = r; j < r + 2; ++j) {
            const int key0 = key_base + (j & 3) + 8 * (j >> 2);
            s0[j] = key0 <= c1.qpos ? s0[j] : -1e30f;
            s1[j] = key0 + 32 <= c1.qpos ? s1[j] : -1e30f;
          }
        }
        if (LOW) {
          const int lo = c1.qpos - window + 1;
#pragma unroll
          for (int j = r; j < r + 2; ++j) {
            const int key0 = key_base + (j & 3) + 8 * (j >> 2);
            s0[j] = key0 >= lo ? s0[j] : -1e30f;
            s1[j] = key0 + 32 >= lo ? s1[j] : -1e30f;
          }
        }
        tmax = attn_max3(tmax, s0[r], s1[r]);
        tmax = attn_max3(tmax, s0[r + 1], s1[r + 1]);
      }
    }
    // (without a window the chunk's first key is visible to every query of the wave, so the row maximum is a real score)
    const float m_c = attn_row_max(tmax);
    const float m_new = attn_max3(m_run, m_c, m_c);
    float psum = 0.f;
    if (!ATCD_KO(2)) attn_tile_exp(s0, s1, m_new, psum);
    unsigned pp[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const half2v a = {(half_t)s0[2 * i], (half_t)s0[2 * i + 1]};
      const half2v b2 = {(half_t)s1[2 * i], (half_t)s1[2 * i + 1]};
      pp[i] = __builtin_bit_cast(unsigned, a);
      pp[8 + i] = __builtin_bit_cast(unsigned, b2);
    }
    // online merge (m_run starts at -1e30: alpha = 0 and the zero accumulators stay zero on the first chunk); the 64 accumulator
    // registers are only touched when some lane's maximum moved - multiplying by 1.0f changes no bit
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    if (!ATCD_KO(2) && __builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
      const f32x2 a2 = {alpha, alpha};
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const f32x2 x = f32x2{o[f][r], o[f][r + 1]} * a2;
          o[f][r] = x[0]; o[f][r + 1] = x[1];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    const LaneCtx c3 = lane_ctx(opaque_lane());
    if (!ATCD_KO(3)) pv_image(c3, kst + 2 * ATCD_IMG_HALFS, pp, o[0], o[1]);
    __builtin_amdgcn_sched_barrier(0);
    if (!ATCD_KO(3)) pv_image(c3, kst + 3 * ATCD_IMG_HALFS, pp, o[2], o[3]);
    __builtin_amdgcn_sched_barrier(0);
  };

  using T = std::integral_constant<bool, true>; using F = std::integral_constant<bool, false>;
  for (int ch = ch0; ch < nch; ++ch) {
    const int st = ch & 1;
    // the next chunk travels while this one is computed: its stage was last read before the barrier that ended chunk ch - 1
    if (ch + 1 < nch && !ATCD_KO(0)) issue_chunk(opaque_lane(), ch + 1, st ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    // else: every key of the chunk lies after every query of this wave, or (WIN) before every window
    if (active && ch * ATCD_KEYS <= q0 + 31 && (!WIN || ch * ATCD_KEYS + ATCD_KEYS - 1 >= wlo)) {
      const bool mask = ch * ATCD_KEYS + ATCD_KEYS - 1 > q0, low = WIN && ch * ATCD_KEYS < wlo_last;
      if (mask) { if (low) chunk_body(T{}, T{}, ch, st); else chunk_body(T{}, F{}, ch, st); }
      else { if (low) chunk_body(F{}, T{}, ch, st); else chunk_body(F{}, F{}, ch, st); }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // chunk ch + 1 has landed (it had this whole chunk to do so)
    __builtin_amdgcn_s_waitcnt(0xc07f);                    // lgkmcnt(0): every LDS read of this chunk retired
    if (!ATCD_KO(4)) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  // ---- context rows: normalise, pack, 16-byte stores (v_permlane32_swap pairs the half-waves' quads into whole octets) ----
  if (active) {
    const float l_row = attn_row_sum(l_run);
    const float inv = 1.0f / l_row;                          // a query always sees its own key: l_row > 0
    const LaneCtx c4 = lane_ctx(opaque_lane());
    half_t* dst = p.ctx + (size_t)(tok0 + (c4.qpos < L ? c4.qpos : L - 1)) * p.ldctx + h * 128 + 16 * c4.hh;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      unsigned pk[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        half4 a;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = f2h_sat(o[f][4 * q + j] * inv);
        const auto au = __builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, a);
        pk[2 * q] = au[0]; pk[2 * q + 1] = au[1];
      }
      const auto x0 = __builtin_amdgcn_permlane32_swap(pk[0], pk[4], false, false);
      const auto x1 = __builtin_amdgcn_permlane32_swap(pk[1], pk[5], false, false);
      const auto y0 = __builtin_amdgcn_permlane32_swap(pk[2], pk[6], false, false);
      const auto y1 = __builtin_amdgcn_permlane32_swap(pk[3], pk[7], false, false);
      const attd_u32x4 lo = {x0[0], x1[0], x0[1], x1[1]};
      const attd_u32x4 hi = {y0[0], y1[0], y0[1], y1[1]};
      if (c4.qpos < L && !ATCD_KO(5)) {
        *(attd_u32x4*)(dst + 32 * f) = lo;
        *(attd_u32x4*)(dst + 32 * f + 8) = hi;
      }
    }
  }
}

// =========================== incremental decoding: one new row per sequence against a K / V cache ===========================
// ONE kernel family for both head widths, templated on D = head_dim (128, or 64 with llama_kernels_hd64.h included).
// rk_llama_generate keeps every layer's rotated keys and its values: per layer K [rows][n_kv][P][D] then V, fp16, the keys of one
// kv head contiguous (an FP8-cache engine, rk_llama_set_kv_fp8, keeps bytes and exponents instead: llama_kernels_kv8.h).  Who writes
// it: the step kernel's owning workgroup, and the fill and the append further down.

// the regions of one layer's cache (kv_layout.h): K and V planes - fp16, or bytes in mode 1, which adds the two exponent planes
// [rows][n_kv][pe]; ke / ve / pe are null / 0 in the fp16 layouts (modes 0 and 2)
struct Kv8Cache { half_t* kc; half_t* vc; int8_t* ke; int8_t* ve; int pe; };

struct LlamaDecAttnArgs {
  const half_t* qkv;     // [rows, ld]: the step's fused q | k | v rows, NOT yet rotated
  half_t* kc;            // this layer's key cache [rows][n_kv][P][D]; the new key is written at the row's position
  half_t* vc;            // value cache, same shape
  const int* pos;        // [rows] position of the new row (device: it advances inside the replayed step graph)
  const float* cos_t;    // rotary tables [max_pos, D / 2]
  const float* sin_t;
  float* part;           // [rows][n_heads][nch][ldc_pstr(D)]: per key chunk D accumulators, running maximum, sum
  half_t* ctx;           // [rows, n_heads * D]
  int ld, n_heads, n_kv, P, nch;
  float scale_log2e;     // head_dim**-0.5 * log2(e)
  const float* bias;     // Qwen2: this layer's q | k | v projection bias [(n_heads + 2 n_kv) * D] fp32, else null
  int window;            // the windowed kernels (Mistral's sliding window): W > 0, the row at pos sees keys max(0, pos - W + 1) .. pos
  const float* qkn = nullptr;   // Qwen3 (attn_dec_cached_qkn_kernel, llama_kernels_qknorm.h): this layer's q | k head-norm weights [2 * 128] fp32, else null
  float qkn_eps = 0.f;          // ... and the norm's eps
};
#define LDC_CHUNK 128    // keys per workgroup: FIXED, so the chunk boundaries of a sequence follow from its own position alone
constexpr int ldc_pstr(int D) { return D + 4; }   // floats per partial: D accumulators, maximum, sum, 2 unused (16-byte rows)

__device__ __forceinline__ float row8_sum_f(float v) {   // sum over an aligned group of 8 lanes, every lane gets it; fixed order
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

template <bool BIAS>   // llama_kernels_hd64.h
__device__ __forceinline__ void rope64_pairs(const half_t* __restrict__ head, const float* __restrict__ bias_head, int i0,
                                             const float (&co)[8], const float (&si)[8], half8& oa, half8& ob);

__device__ __forceinline__ half8 qkn_lane8(const half_t* row, const float* w, float eps, int n_heads, int hd, int i0, bool hi,
                                           const float (&co)[8], const float (&si)[8]);   // llama_kernels_qknorm.h

typedef unsigned kv8_u2 __attribute__((ext_vector_type(2)));   // a lane's 8 bytes of an FP8 cache vector
typedef unsigned kv8_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ half8 kv8_quant16(const half8 x, kv8_u2& q, int& e);   // llama_kernels_kv8.h
__device__ __forceinline__ half8 kv8_deq8(const kv8_u2 q, int e);

// The step's rotation of the new row, the one thing the two widths do differently: this lane's 8 dims (elements i0 .. i0 + 7 of
// the first half of the head, or with `hi` their partners in the second) of rotated head hd (of q | k) of `row`, rounded as the
// prefill's kernel of that width does, on the same table entries co / si.  D = 64: rope64_pairs, rope64_kernel's own form.
// D = 128: rope128_kernel's arithmetic - the same rope_rot calls, on the widened fp16 values or behind bias_add8.  HALF (bias-free
// 128 only; the cached step's body asks for it, the drafting step's kernels do not): the lane's own half by rope_rot_half, the same
// bits from half the multiplies.  Which of the two a kernel takes is a matter of time alone: with rope_rot the plain step's R = 4
// kernel needed 170 registers for the parent's 128 and Llama-3-8B's step at 4 slots ran 1.8 % slower; with rope_rot_half it is at
// the parent's, while the drafting step's kernels measured faster with rope_rot ("Where roundings part").
template <int D, bool BIAS, bool HALF = false>
__device__ __forceinline__ half8 rope_lane8(const half_t* row, const float* bias, int hd, int i0, bool hi,
                                            const float (&co)[8], const float (&si)[8]) {
  const half_t* head = row + (size_t)hd * D;
  if constexpr (D == 64) {
    half8 oa, ob;
    rope64_pairs<BIAS>(head, BIAS ? bias + (size_t)hd * 64 : nullptr, i0, co, si, oa, ob);
    return hi ? ob : oa;
  } else {
    const half8 a = *(const half8*)(head + i0), bb = *(const half8*)(head + 64 + i0);
    half8 o;
    if constexpr (BIAS) {
      float xa[8], xb[8];
      bias_add8(xa, a, bias + (size_t)hd * 128 + i0);
      bias_add8(xb, bb, bias + (size_t)hd * 128 + 64 + i0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float lo, up;
        rope_rot(xa[j], xb[j], co[j], si[j], j == 0, lo, up);
        o[j] = hi ? f2h_sat(up) : f2h_sat(lo);
      }
    } else if constexpr (HALF) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {                           // the lane's own half alone: (u, w) = (x1, -x2) or (x2, x1)
        const float x1 = (float)a[j], x2 = (float)bb[j];
        o[j] = f2h_sat(rope_rot_half(hi ? x2 : x1, hi ? x1 : -x2, co[j], si[j], j == 0));
      }
    } else {
      float xa[8], xb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { xa[j] = (float)a[j]; xb[j] = (float)bb[j]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float lo, up;
        rope_rot(xa[j], xb[j], co[j], si[j], j == 0, lo, up);
        o[j] = hi ? f2h_sat(up) : f2h_sat(lo);
      }
    }
    return o;
  }
}

// Single-token attention over the cache (hf: modeling_llama.py:130-214 at one query position: scaling head_dim**-0.5, fp32
// softmax, repeat_kv), d = D.  grid = (key chunks of the longest cache, n_heads / R, rows), 256 threads.  The contract, for both
// widths:
// * FIXED chunks.  A workgroup takes ONE chunk of LDC_CHUNK keys - cut from the row's own position, whatever P and whatever the
//   other rows hold - of one kv head and R query heads that share it: with R = n_heads / n_kv_heads (Llama-3-8B: 4) every K / V
//   byte is read once per kv head.  K / V go straight to registers (no LDS staging: each byte is used once): a lane holds 8 of a
//   key's D dims, D / 8 lanes a key, a wave 512 / D keys per load and 32 keys in all (D / 16 loads), every load issued before the
//   first use.
// * Who writes the cache.  The new row is rotated here by rope_lane8 - the arithmetic of the prefill's kernel of this width on the
//   same table entries - its key and value are used from registers and written to the cache by the workgroup that owns the
//   position's chunk, once per kv head.  BIAS (Qwen2): the row's q / k / v get the projection bias where they are loaded -
//   bias_add8 / bias_v8, the prefill kernel's arithmetic and rounding.  With and without it the key a step writes to the cache is
//   bit for bit the key a prefill writes for that token: at both widths both call one fixed source form (rope_rot), nothing is
//   left to what a compiler contracts in one instantiation and not in another.
// * The merge.  Each workgroup leaves one (maximum, sum, D accumulators) partial per head - its four waves merged in wave order -
//   and attn_dec_combine_kernel merges a row's chunks in key order: nobody waits on another workgroup.
// * Independence.  A row's context depends on its own position only, never on the batch, and a head's arithmetic does not depend
//   on R (every per-head array is indexed by r alone, the merge is per head).
// BIAS = false is the Llama kernel (its 128-wide rotation in rope_rot's form since the step and the prefill were found to round
// element 0's second half differently).  The sum over a key's lanes is what each width always used: row16_sum_f
// (DPP) at 128, the three shuffles of row8_sum_f at 64.
// (The kernel is an entry point around a body, `rotated` a lambda around rope_lane8 and the shuffles across a wave's keys are
// written out, because that is the form the compiler in use turns into the instructions these kernels always had; the T5 step's
// attn_dec_cached_kernel(AttnCachedArgs) in attention.h is another kernel.)
// WIN (Mistral's sliding window, LlamaDecAttnArgs::window = W > 0; the entries attn_dec_cached_win_kernel / attn_dec_combine_win_kernel):
// the row sees keys lo = max(0, pos - W + 1) .. pos.  A workgroup whose whole chunk lies below lo returns at once (uniform, like the
// chunk beyond pos) and leaves NO partial; a wave whose 32 keys lie below lo keeps its empty state, as a wave beyond pos does; the
// keys below lo inside a visible wave get the -1e30 of the keys beyond pos; the merge walks chunks lo / LDC_CHUNK .. pos / LDC_CHUNK
// only.  The cache keeps every position and the chunk that owns pos (always visible) still writes the new key and value.  With
// pos < W nothing is skipped or masked: the plain kernel's bits.  WIN = false is the kernel as it was.
// QKN (Qwen3's q / k head norm; the entry attn_dec_cached_qkn_kernel in llama_kernels_qknorm.h): the row transform is qkn_lane8 - norm,
// rotation, one rounding, the arithmetic of the prefill's rope128_qkn_kernel - instead of rope_lane8; nothing else differs.
// KEYS (a drafting session's step, LlamaDecAttnKeysArgs; the entries attn_dec_keys_*_kernel below): the step's rows are G1 per
// cache row - row b reads cache row b / G1 - and every key <= pos, the row's own included, is already in the cache
// (kv_cache_append_kernel ran in front): no new key is formed, none is selected and nothing is written.  The bytes the append left
// are the bytes `knew` / `vnew` hold in the plain form, so a row's context is the plain kernel's bit for bit.  KEYS = false is the
// kernel as it was.
// KV8 (an FP8-cache engine, rk_llama_set_kv_fp8; the entries and the format: llama_kernels_kv8.h; ARGS = LlamaDecAttnKv8Args): the
// cache's element type.  0: fp16, the kernel as it was.  1: one e4m3fn byte per value and one exponent per vector - a lane loads 8
// bytes of K and 8 of V, the wave its 32 keys' exponents as two 16-byte loads per plane, and kv8_deq8 turns each piece into the half8
// the fp16 kernel loads from the dequantised cache (exact), so everything behind the loads is the same text.  2: the fp16 cache
// holding dequantised values (option llama_kv_fp8 = 0).  1 and 2: the row's own key and value pass through kv8_quant16 before they
// are used and before they are stored - the row sees its key as every later step reads it back.
template <int D, int R, bool BIAS, bool WIN, bool QKN = false, bool KEYS = false, class ARGS = LlamaDecAttnArgs, int KV8 = 0>
__device__ __forceinline__ void attn_dec_cached_body(const ARGS& p) {
  static_assert(D == 128 || D == 64, "lanes per key 16 or 8");
  static_assert(KV8 == 0 || D == 128, "FP8 K / V cache: head_dim 128");
  constexpr int LK = D / 8, KL = 512 / D, NL = D / 16;   // lanes per key, keys per wave load, loads per wave
  __shared__ float s_m[4][R], s_l[4][R];
  __shared__ __attribute__((aligned(16))) float s_acc[4][R][D];
  const int ch = blockIdx.x, h0 = blockIdx.y * R, b = blockIdx.z;
  int pos = p.pos[b];
  pos = pos < 0 ? 0 : (pos < p.P - 1 ? pos : p.P - 1);   // (the host keeps it inside the cache; the clamp keeps a bad word from faulting)
  const int key0 = ch * LDC_CHUNK;
  if (key0 > pos) return;                                 // uniform: this chunk lies beyond the row's keys
  const int lo = WIN ? max(pos - p.window + 1, 0) : 0;    // the row's first visible key
  if (WIN && key0 + LDC_CHUNK - 1 < lo) return;           // uniform: ... or below its window
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kg = lane / LK, c = lane % LK;
  const int G = p.n_heads / p.n_kv, kvh = h0 / G;
  const half_t* row = p.qkv + (size_t)b * p.ld;
  const int i0 = (c % NL) * 8;
  const bool hi = c >= NL;                                // this lane's dims are in the second half of the head
  float co[8], si[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { co[j] = p.cos_t[(size_t)pos * (D / 2) + i0 + j]; si[j] = p.sin_t[(size_t)pos * (D / 2) + i0 + j]; }
  auto rotated = [&](int hd) {
    if constexpr (QKN) return qkn_lane8(row, p.qkn, p.qkn_eps, p.n_heads, hd, i0, hi, co, si);
    else return rope_lane8<D, BIAS, !KEYS>(row, p.bias, hd, i0, hi, co, si);
  };
  half8 knew, vnew;
  int crow = b;                                           // the row's cache row
  if constexpr (KEYS) crow = b / p.g1;
  else {
    knew = rotated(p.n_heads + kvh);
    const size_t voff = (size_t)(p.n_heads + p.n_kv + kvh) * D + c * 8;
    vnew = *(const half8*)(row + voff);
    if constexpr (BIAS) vnew = bias_v8(vnew, p.bias + voff);
  }
  [[maybe_unused]] kv8_u2 kq_new, vq_new;                 // KV8: the new vectors' bytes and exponents
  [[maybe_unused]] int ke_new = 0, ve_new = 0;
  if constexpr (KV8 != 0 && !KEYS) {                      // every lane of the workgroup is here: a key's 16 lanes reduce together
    knew = kv8_quant16(knew, kq_new, ke_new);
    vnew = kv8_quant16(vnew, vq_new, ve_new);
  }
  half_t* kbase = p.kc + ((size_t)crow * p.n_kv + kvh) * p.P * D + c * 8;
  half_t* vbase = p.vc + ((size_t)crow * p.n_kv + kvh) * p.P * D + c * 8;
  [[maybe_unused]] uint8_t *kb8 = nullptr, *vb8 = nullptr;   // KV8 = 1: p.kc / p.vc are byte planes, p.ke / p.ve the exponents [..][pe]
  [[maybe_unused]] int8_t *keb = nullptr, *veb = nullptr;
  if constexpr (KV8 == 1) {
    kb8 = (uint8_t*)p.kc + ((size_t)crow * p.n_kv + kvh) * p.P * D + c * 8;
    vb8 = (uint8_t*)p.vc + ((size_t)crow * p.n_kv + kvh) * p.P * D + c * 8;
    keb = p.ke + ((size_t)crow * p.n_kv + kvh) * p.pe;
    veb = p.ve + ((size_t)crow * p.n_kv + kvh) * p.pe;
  }
  if constexpr (!KEYS) {
    if (pos - key0 < LDC_CHUNK && h0 % G == 0 && wave == 0 && kg == 0) {   // the position's chunk, once per kv head
      if constexpr (KV8 == 1) {
        *(kv8_u2*)(kb8 + (size_t)pos * D) = kq_new;
        *(kv8_u2*)(vb8 + (size_t)pos * D) = vq_new;
        if (c == 0) { keb[pos] = (int8_t)ke_new; veb[pos] = (int8_t)ve_new; }
      } else {
        *(half8*)(kbase + (size_t)pos * D) = knew;
        *(half8*)(vbase + (size_t)pos * D) = vnew;
      }
    }
  }
  const int wkey0 = key0 + wave * 32;
  float m_w[R], l_w[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m_w[r] = -1e30f; l_w[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
  }
  if (wkey0 <= pos && (!WIN || wkey0 + 31 >= lo)) {       // wave-uniform
    half8 kf[NL], vf[NL];
    const int last_old = KEYS ? pos : (pos > 0 ? pos - 1 : 0);   // keys before the new one come from the cache (KEYS: all of them)
    if constexpr (KV8 == 1) {
      // the wave's 32 exponents per plane (wkey0 is a multiple of 32, pe too: aligned, inside the plane), every piece requested
      // before the first conversion.  Key wkey0 + 4 i + kg: byte kg of word i.  An exponent beyond the row's last written position
      // belongs to a key that is masked or replaced below; whatever the byte holds is clamped to the format's range, so the
      // masked product stays finite.
      kv8_u2 kq[NL], vq[NL];
      const kv8_u4 kew0 = *(const kv8_u4*)(keb + wkey0), kew1 = *(const kv8_u4*)(keb + wkey0 + 16);
      const kv8_u4 vew0 = *(const kv8_u4*)(veb + wkey0), vew1 = *(const kv8_u4*)(veb + wkey0 + 16);
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int key = wkey0 + KL * i + kg;
        const int idx = key < last_old ? key : last_old;
        kq[i] = *(const kv8_u2*)(kb8 + (size_t)idx * D);
        vq[i] = *(const kv8_u2*)(vb8 + (size_t)idx * D);
      }
      const int sh = 24 - 8 * kg;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const unsigned kw = i < 4 ? kew0[i & 3] : kew1[i & 3], vw = i < 4 ? vew0[i & 3] : vew1[i & 3];
        const int ek = (int)(kw << sh) >> 24, ev = (int)(vw << sh) >> 24;
        kf[i] = kv8_deq8(kq[i], min(max(ek, -15), 7));
        vf[i] = kv8_deq8(vq[i], min(max(ev, -15), 7));
      }
    } else {
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int key = wkey0 + KL * i + kg;
        const int idx = key < last_old ? key : last_old;
        kf[i] = *(const half8*)(kbase + (size_t)idx * D);
        vf[i] = *(const half8*)(vbase + (size_t)idx * D);
      }
    }
    if constexpr (!KEYS) {
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const bool is_new = wkey0 + KL * i + kg >= pos;
        kf[i] = is_new ? knew : kf[i];
        vf[i] = is_new ? vnew : vf[i];
      }
    }
    float s[R][NL];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const half8 q = rotated(h0 + r);
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = __builtin_fmaf((float)q[j], (float)kf[i][j], d);
        if constexpr (D == 128) d = row16_sum_f(d) * p.scale_log2e;
        else d = row8_sum_f(d) * p.scale_log2e;
        if constexpr (WIN) s[r][i] = wkey0 + KL * i + kg <= pos && wkey0 + KL * i + kg >= lo ? d : -1e30f;
        else s[r][i] = wkey0 + KL * i + kg <= pos ? d : -1e30f;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mx = s[r][0];
#pragma unroll
      for (int i = 1; i < NL; ++i) mx = fmaxf(mx, s[r][i]);
      if constexpr (LK == 8) mx = fmaxf(mx, __shfl_xor(mx, 8));   // across the wave's keys: lanes LK, 2 LK .. 32 apart, in that order
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const float pr = __builtin_amdgcn_exp2f(s[r][i] - mx);   // masked keys: exp2(-1e30) = 0
        sum += pr;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_fmaf(pr, (float)vf[i][j], acc[r][j]);
      }
      if constexpr (LK == 8) sum += __shfl_xor(sum, 8);
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if constexpr (LK == 8) acc[r][j] += __shfl_xor(acc[r][j], 8);
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
  if (tid < D) {                                          // the four waves' partials, merged in wave order
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
      float* dst = p.part + (((size_t)b * p.n_heads + h0 + r) * p.nch + ch) * ldc_pstr(D);
      dst[tid] = A;
      if (tid == 0) { dst[D] = M; dst[D + 1] = L; }
    }
  }
}

template <int D, int R, bool BIAS>
__global__ __launch_bounds__(256) void attn_dec_cached_kernel(LlamaDecAttnArgs p) { attn_dec_cached_body<D, R, BIAS, false>(p); }
template <int D, int R, bool BIAS>
__global__ __launch_bounds__(256) void attn_dec_cached_win_kernel(LlamaDecAttnArgs p) { attn_dec_cached_body<D, R, BIAS, true>(p); }

// ---- the cache's fill behind a prefill (the append in front of a drafting step: further down) ----
// How a vector enters the cache, in the cache's mode KV8: lane c (of the vector's D / 8) stores its 8 values x of the key or the
// value of (head = cache row * n_kv + kv head, position t) into that vector's plane (and exponent plane, rows of pe).  0: fp16 as
// it is.  1 and 2 (llama_kernels_kv8.h; the vector's 16 lanes are all here): through kv8_quant16 - 1 stores the bytes and, lane
// 0, the exponent; 2 the dequantised fp16 values.  Called once for the key and once for the value.  (The step kernel's owning
// workgroup and the append write the same way from vectors they hold already: their stores stay where they were - byte-identical kernels.)
template <int D, int KV8>
__device__ __forceinline__ void kv_cache_store8(half_t* plane, int8_t* eplane, int pe, size_t head, int P, int t, int c, half8 x) {
  static_assert(KV8 == 0 || D == 128, "FP8 K / V cache: head_dim 128");
  [[maybe_unused]] kv8_u2 q;
  [[maybe_unused]] int e;
  if constexpr (KV8 != 0) x = kv8_quant16(x, q, e);
  const size_t dst = (head * P + t) * D + c * 8;
  if constexpr (KV8 == 1) {
    *(kv8_u2*)((uint8_t*)plane + dst) = q;
    if (c == 0) eplane[head * pe + t] = (int8_t)e;
  } else *(half8*)(plane + dst) = x;
}

// kv_cache_fill_kernel copies the prompt's rows out of the prefill's fused QKV buffer (after rope128_kernel / rope64_kernel);
// grid = (longest prompt, n_seq), a thread moves one 16-byte piece of K and of V (D / 8 pieces per head).
// SLOTS is the decoding session's fill (rk_llama_session_admit): the same copy, but sequence b of the call goes to cache row
// slots[b] of a cache of n_slots rows that holds other, running rows - two 16-byte stores per thread, addresses from the slot map
// alone.  Without SLOTS sequence b goes to row b and slots / n_slots are null / 0.
// KV8 (the entries kv8_cache_fill_kernel: llama_kernels_kv8.h): the same grid, the same item per thread - a head's 16 pieces are
// 16 adjacent threads and the bound n_kv * 16 is a multiple of 16, so a vector's lanes enter and leave the loop together -
// through kv_cache_store8 in the cache's mode.
template <int D, bool SLOTS, int KV8>
__device__ __forceinline__ void kv_cache_fill_body(const half_t* __restrict__ qkv, const int* __restrict__ seq_off,
                                                   const int* __restrict__ slots, int n_slots, const Kv8Cache& cc, int ld,
                                                   int n_heads, int n_kv, int P) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int tok0 = seq_off[b], crow = SLOTS ? slots[b] : b;
  if (t >= seq_off[b + 1] - tok0 || t >= P || (SLOTS && (crow < 0 || crow >= n_slots))) return;
  const half_t* row = qkv + (size_t)(tok0 + t) * ld + (size_t)n_heads * D;
  for (int c = threadIdx.x; c < n_kv * (D / 8); c += 256) {
    const int h = c / (D / 8), piece = (c % (D / 8)) * 8;
    const size_t head = (size_t)crow * n_kv + h;
    kv_cache_store8<D, KV8>(cc.kc, cc.ke, cc.pe, head, P, t, c % (D / 8), *(const half8*)(row + h * D + piece));
    kv_cache_store8<D, KV8>(cc.vc, cc.ve, cc.pe, head, P, t, c % (D / 8), *(const half8*)(row + (size_t)(n_kv + h) * D + piece));
  }
}
template <int D, bool SLOTS>
__global__ __launch_bounds__(256) void kv_cache_fill_kernel(const half_t* __restrict__ qkv, const int* __restrict__ seq_off,
                                                            const int* __restrict__ slots, int n_slots,
                                                            half_t* __restrict__ kc, half_t* __restrict__ vc, int ld,
                                                            int n_heads, int n_kv, int P) {
  kv_cache_fill_body<D, SLOTS, 0>(qkv, seq_off, slots, n_slots, Kv8Cache{kc, vc, nullptr, nullptr, 0}, ld, n_heads, n_kv, P);
}

// ---- a drafting session's step (rk_llama_session_open_draft): G1 rows per cache row, the keys appended in front of the attention ----
struct LlamaDecAttnKeysArgs : LlamaDecAttnArgs {   // the drafting entries' arguments; the plain kernels' struct stays what it was
  int g1;                // rows per cache row: step row b belongs to cache row b / g1
  const int* live;       // [rows] kv_cache_append_kernel: 1 = the row's key and value go to the cache, 0 = a dead row, nothing is written
};
// The cache append of a drafting step, in front of each layer's attention: row b's rotated key and its value go to cache row
// b / g1 at the row's position - formed by the helpers the step kernel forms `knew` / `vnew` with (rope_lane8 / bias_v8 / qkn_lane8,
// on the lane mapping of attn_dec_cached_body: lane c of a key's D / 8 holds 8 dims), every one of them a fixed form in source, so
// the bytes are those a plain step writes (tests/test_gpu_rope_forms.py, tests/test_gpu_draft_attention.py: g1 plain steps leave
// the same cache, byte for byte).
// grid = rows; an item is (kv head, lane c).  A dead row (live[b] = 0) or a position outside the cache writes nothing.  QKN: the 8
// lanes of an aligned group hold the items of one half of ONE head (D / 8 = 16 items per head) and the bound n_kv * 16 is a multiple
// of 8, so a group enters and leaves the loop together and qkn_pairs' shuffles read active lanes only.
// (kv8_cache_append_kernel, llama_kernels_kv8.h, is this kernel plus the quantiser in front of the stores.  The two stay two
// kernels: merged into one body with the cache's mode as a policy, as the fill is, the fp16 instantiations came out with another
// schedule, and the bias one measured 2 % slower than the parent's - profiles/llama_step_dispatch_refactor.txt.)
template <int D, bool BIAS, bool QKN>
__global__ __launch_bounds__(256) void kv_cache_append_kernel(LlamaDecAttnKeysArgs p) {
  constexpr int LK = D / 8, NL = D / 16;
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
    const half8 knew = rotated(p.n_heads + kvh);
    const size_t voff = (size_t)(p.n_heads + p.n_kv + kvh) * D + c * 8;
    half8 vnew = *(const half8*)(row + voff);
    if constexpr (BIAS) vnew = bias_v8(vnew, p.bias + voff);
    const size_t dst = (((size_t)crow * p.n_kv + kvh) * p.P + pos) * D + c * 8;
    *(half8*)(p.kc + dst) = knew;
    *(half8*)(p.vc + dst) = vnew;
  }
}
template <int D, int R, bool BIAS>
__global__ __launch_bounds__(256) void attn_dec_keys_kernel(LlamaDecAttnKeysArgs p) { attn_dec_cached_body<D, R, BIAS, false, false, true>(p); }
template <int D, int R, bool BIAS>
__global__ __launch_bounds__(256) void attn_dec_keys_win_kernel(LlamaDecAttnKeysArgs p) { attn_dec_cached_body<D, R, BIAS, true, false, true>(p); }
template <int D, int R>
__global__ __launch_bounds__(256) void attn_dec_keys_qkn_kernel(LlamaDecAttnKeysArgs p) { attn_dec_cached_body<D, R, false, false, true, true>(p); }

// Merges the chunk partials of one (sequence, head) in key order and writes the fp16 context.  grid = (n_heads, rows), D
// threads = the head's D dims.
// WIN: the chunks that hold a visible key, lo / LDC_CHUNK .. pos / LDC_CHUNK - the ones below wrote no partial.
template <int D, bool WIN>
__device__ __forceinline__ void attn_dec_combine_body(const LlamaDecAttnArgs p) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int pos = p.pos[b];
  pos = pos < 0 ? 0 : (pos < p.P - 1 ? pos : p.P - 1);
  const int n = pos / LDC_CHUNK + 1;
  const int k0 = WIN ? max(pos - p.window + 1, 0) / LDC_CHUNK : 0;
  const float* src = p.part + ((size_t)b * p.n_heads + h) * p.nch * ldc_pstr(D);
  float M = -1e30f;
  for (int k = k0; k < n; ++k) M = fmaxf(M, src[(size_t)k * ldc_pstr(D) + D]);
  float L = 0.f, A = 0.f;
  for (int k = k0; k < n; ++k) {
    const float f = __builtin_amdgcn_exp2f(src[(size_t)k * ldc_pstr(D) + D] - M);
    L = __builtin_fmaf(src[(size_t)k * ldc_pstr(D) + D + 1], f, L);
    A = __builtin_fmaf(src[(size_t)k * ldc_pstr(D) + d], f, A);
  }
  p.ctx[(size_t)b * p.n_heads * D + h * D + d] = f2h_sat(A / L);   // a row always sees its own key: L > 0
}
template <int D>
__global__ __launch_bounds__(D) void attn_dec_combine_kernel(LlamaDecAttnArgs p) { attn_dec_combine_body<D, false>(p); }
template <int D>
__global__ __launch_bounds__(D) void attn_dec_combine_win_kernel(LlamaDecAttnArgs p) { attn_dec_combine_body<D, true>(p); }
