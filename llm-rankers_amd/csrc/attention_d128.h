// T5 encoder self-attention for gfx950 at d_kv = 128 (t5-3b, t5-11b: monoT5-3B, duoT5-3B).
//
// Semantics: the header of attention.h with 128-wide heads -
//   P = softmax(Q K^T + lut[h, clamp(j - i, +-128)]),  ctx = P V        (no scaling; hf: modeling_t5.py:144-173, :196-197)
// over the packed qkv rows (q | k | v at columns 0 | I | 2I, I = 128 H), ragged through seq_off.
//
// ONE kernel for every sequence length (no short / long split): attn_enc_kernel's S^T = K Q^T layout carried to 128 dims.
// grid = (ceil(maxL / 128), H, B), four waves of 32 queries.  Per 64-key tile the K rows (row-major) and the V rows
// (TRANSPOSED) are staged in LDS; S^T = K Q^T by MFMA 32x32x16 f16 in eight k16 steps (A = K rows, B = Q^T), so a lane owns ONE
// query column: running maximum, sum and rescale are per-lane scalars and the fp16 probabilities are already in B-operand
// position for O^T = V^T P^T (A = V^T rows, four f32x16 accumulators: d = 32 dq + ...).  Online softmax per 64-key tile for
// EVERY length, in the log2 domain with the pre-multiplied table - attn_tile_bias_max, attn_tile_exp, attn_row_max and
// attn_row_sum of attention.h, in attn_tile_softmax's order.  Probabilities are rounded to fp16 as the P V operand, sums are
// fp32.  Double-buffered tiles, one barrier per tile: the K rows of tile t + 1 travel through registers while the scores of
// tile t are formed, its V rows while softmax and P V run (never both at once: o, Q and the scores already hold 128 of the
// 256 registers a wave has at two workgroups per CU).  The context rows leave through LDS as whole 256-byte head rows.
//
// A sequence's bytes depend on its own tokens and length only: a wave's arithmetic reads its 32 query rows, the sequence's key
// tiles in order and the head's table - never the grid, the batch or the sequence's place in it.
//
// LDS: 2 x 17 408 (K) + 2 x 17 408 (V^T) + the table = 70 672 bytes, dynamic; two workgroups per CU.
#pragma once
#include "attention.h"

#define ATT128_KSTR 136   // sK row stride in halfs (272 B: 16-B aligned, conflict-free b128 reads)
#define ATT128_VSTR 68    // sVt row stride in halfs (136 B: 8-B aligned, conflict-free b64 reads)
#define ATT128_K_HALFS (64 * ATT128_KSTR)
#define ATT128_V_HALFS (128 * ATT128_VSTR)
#define ATT128_LDS_BYTES (2 * ATT128_K_HALFS * 2 + 2 * ATT128_V_HALFS * 2 + (RK_LUT_N + 3) * 4)

struct AttnEnc128Args {
  const half_t* qkv;     // [T, ld]: q at column 0, k at column I, v at column 2I
  half_t* ctx;           // [T, ldctx]
  const int* seq_off;    // [B+1] token offsets of the packed batch
  const float* bias_lut; // [H][RK_LUT_N]
  int ld, ldctx, I;
};

// attn_tile_softmax (attention.h) over four output accumulators: the same operations in the same order, in ONE form for
// every tile (the kernel holds 128 accumulator, Q and score registers; a specialised body per first / last / far tile made
// the register allocator spill).  The masked form on a tile that lies inside the sequence takes none of its selects (they are
// decided per group of eight keys on wave-uniform values).  The general step on tile 0 gives the first tile's bits: the
// running maximum starts at -1e30, below every score, so m_new = the tile's maximum, alpha = exp2(-1e30 - m_new) = 0,
// l = 0 * 0 + psum and the zero accumulators stay zero.
template <class BiasFn>
__device__ __forceinline__ void attn128_tile_softmax(f32x16& s0, f32x16& s1, f32x16 (&o)[4], float& m_run, float& l_run, int key_base, int L, BiasFn bias) {
  float tmax = -1e30f;
  attn_tile_bias_max<true, BiasFn, true>(s0, s1, tmax, key_base, L, bias);   // (chunked table reads: the register budget)
  tmax = attn_row_max(tmax);
  const float m_new = attn_max3(m_run, tmax, tmax);
  float psum = 0.f;
  attn_tile_exp(s0, s1, m_new, psum);
  psum = attn_row_sum(psum);
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
  l_run = l_run * alpha + psum;
#pragma unroll
  for (int dq = 0; dq < 4; ++dq)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dq][r] *= alpha;
  m_run = m_new;
}

#define ATT128_NW 4   // waves per workgroup: 128 queries share a staged key tile (two waves would re-stage every tile twice for
                      // the same four waves per CU: LDS holds two workgroups either way)
__global__ __launch_bounds__(64 * ATT128_NW, 2) void attn_enc128_kernel(AttnEnc128Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char att128_smem[];
  constexpr int NW = ATT128_NW, NT = 64 * NW, QB = 32 * NW;
  half_t* const sK = (half_t*)att128_smem;                 // [2][64 keys][ATT128_KSTR]
  half_t* const sVt = sK + 2 * ATT128_K_HALFS;             // [2][128 d][ATT128_VSTR]
  float* const sLut = (float*)(sVt + 2 * ATT128_V_HALFS);
  const int b = blockIdx.z, h = blockIdx.y, qt = blockIdx.x;
  const int tok0 = p.seq_off[b];
  const int L = p.seq_off[b + 1] - tok0;
  if (qt * QB >= L) return;   // uniform for the whole block
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hh = lane >> 5, l31 = lane & 31;
  for (int i = tid; i < RK_LUT_N; i += NT) sLut[i] = p.bias_lut[h * RK_LUT_N + i] * ATT_LOG2E;
  const int q0 = qt * QB + wave * 32;
  const bool wave_active = q0 < L;
  const int qpos = q0 + l31;
  const int qrow = qpos < L ? qpos : L - 1;
  half8 qf[8];
  {
    const half_t* qptr = p.qkv + (size_t)(tok0 + qrow) * p.ld + h * 128 + 8 * hh;
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *(const half8*)(qptr + 16 * s);
  }
  f32x16 o[4];
#pragma unroll
  for (int dq = 0; dq < 4; ++dq)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dq][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const int nkt = (L + 63) >> 6;
  // staging roles.  K: piece t = tid + i NT is row t >> 4, 16-byte chunk t & 15 (a row's 256 bytes by 16 adjacent lanes).
  // V: piece t is key pair (t >> 3) & 31, chunk (t & 7) | (t >> 8) << 3: a wave writes eight key pairs of eight d rows
  // at a time (the transposed image takes key PAIRS: ds_write_b32)
  constexpr int NKP = 1024 / NT, NVP = 512 / NT;
  half8 rk[NKP], rv[NVP][2];
  const half_t* const base = p.qkv + p.I + h * 128;
  auto load_k = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NKP; ++i) {
      const int t = tid + i * NT, row = min(kt * 64 + (t >> 4), L - 1);
      rk[i] = *(const half8*)(base + (size_t)(tok0 + row) * p.ld + (t & 15) * 8);
    }
  };
  auto load_v = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NVP; ++i) {
      const int t = tid + i * NT, pr = (t >> 3) & 31, ch = (t & 7) | ((t >> 8) << 3);
      const int va = min(kt * 64 + 2 * pr, L - 1), vb = min(kt * 64 + 2 * pr + 1, L - 1);
      rv[i][0] = *(const half8*)(base + p.I + (size_t)(tok0 + va) * p.ld + ch * 8);
      rv[i][1] = *(const half8*)(base + p.I + (size_t)(tok0 + vb) * p.ld + ch * 8);
    }
  };
  auto store_k = [&](int buf) {
    half_t* kb_ = sK + buf * ATT128_K_HALFS;
#pragma unroll
    for (int i = 0; i < NKP; ++i) {
      const int t = tid + i * NT;
      *(half8*)(kb_ + (t >> 4) * ATT128_KSTR + (t & 15) * 8) = rk[i];
    }
  };
  auto store_v = [&](int buf) {
    half_t* vb_ = sVt + buf * ATT128_V_HALFS;
#pragma unroll
    for (int i = 0; i < NVP; ++i) {
      const int t = tid + i * NT, pr = (t >> 3) & 31, ch = (t & 7) | ((t >> 8) << 3);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const half2v two = {rv[i][0][j], rv[i][1][j]};
        *(half2v*)(vb_ + (ch * 8 + j) * ATT128_VSTR + 2 * pr) = two;
      }
    }
  };
  load_k(0);
  load_v(0);
  store_k(0);
  store_v(0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nkt;
    const half_t* kbuf = sK + cur * ATT128_K_HALFS;
    const half_t* vbuf = sVt + cur * ATT128_V_HALFS;
    f32x16 s0, s1;
    if (more) load_k(kt + 1);                     // in flight while this tile's scores are formed
    if (wave_active) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
      // the K fragments of step s + 1 are requested before the MFMAs of step s (the sched_barriers pin that order and keep
      // the compiler from requesting all sixteen at once)
      half8 kf[2][2];
      auto fetch = [&](int s, half8 (&d)[2]) {
        d[0] = *(const half8*)(kbuf + l31 * ATT128_KSTR + 16 * s + 8 * hh);
        d[1] = *(const half8*)(kbuf + (32 + l31) * ATT128_KSTR + 16 * s + 8 * hh);
      };
      fetch(0, kf[0]);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        if (s + 1 < 8) fetch(s + 1, kf[(s + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        s0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[s & 1][0], qf[s], s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[s & 1][1], qf[s], s1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (more) { store_k(cur ^ 1); load_v(kt + 1); }   // buffer cur^1 was last read before the previous barrier; V: in flight during softmax and P V
    __builtin_amdgcn_sched_barrier(0);
    if (wave_active) {
      {
        const int key_base = kt * 64 + 4 * hh;
        attn128_tile_softmax(s0, s1, o, m_run, l_run, key_base, L, [&](int r, int sub) {
          int rel = key_base + (r & 3) + 8 * (r >> 2) + 32 * sub - qpos;
          rel = rel < -RK_LUT_R ? -RK_LUT_R : (rel > RK_LUT_R ? RK_LUT_R : rel);
          return sLut[rel + RK_LUT_R];
        });
      }
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          half8 pf;
#pragma unroll
          for (int i = 0; i < 8; ++i) pf[i] = (half_t)(sub == 0 ? s0[8 * sp + i] : s1[8 * sp + i]);
          const int kb = sub * 32 + 16 * sp + 4 * hh;   // keys kb..kb+3 and kb+8..kb+11 <-> regs 8sp..8sp+7
#pragma unroll
          for (int dq = 0; dq < 4; ++dq) {
            const half_t* vr = vbuf + (32 * dq + l31) * ATT128_VSTR + kb;
            const half4 v0 = *(const half4*)vr, v1 = *(const half4*)(vr + 8);
            const half8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            o[dq] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[dq], 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);          // one k16 step's eight V^T reads at a time
        }
      }
    }
    if (more) store_v(cur ^ 1);
    __syncthreads();
  }
  // all waves are past the last barrier: K buffer 0 turns per-lane 8-byte pieces into whole context rows
  // (NW x 16 rows of ATT128_KSTR halfs <= the buffer's 64 rows)
  if (wave_active) {
    const float inv = 1.0f / l_run;
    half_t* st = sK + wave * (16 * ATT128_KSTR);   // 2 passes of 16 query rows x 128 d per wave
#pragma unroll
    for (int half_i = 0; half_i < 2; ++half_i) {
      if ((l31 >> 4) == half_i) {
#pragma unroll
        for (int dq = 0; dq < 4; ++dq)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            half4 a;
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = f2h_sat(o[dq][4 * q + j] * inv);
            *(half4*)(st + (l31 & 15) * ATT128_KSTR + 32 * dq + 8 * q + 4 * hh) = a;
          }
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r0 = 0; r0 < 16; r0 += 4) {
        const int row = r0 + (lane >> 4), ch = lane & 15;
        const int qq = q0 + half_i * 16 + row;
        if (qq < L)
          *(half8*)(p.ctx + (size_t)(tok0 + qq) * p.ldctx + h * 128 + ch * 8) = *(const half8*)(st + row * ATT128_KSTR + ch * 8);
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
  }
}
