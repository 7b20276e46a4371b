// FP8 step weights (DESIGN.md section 3 "FP8 step weights"): the quantiser and the FP8 feed of the weight-streaming GEMM.
//
// Format of a matrix W [N][K] (fp16, K % 16): groups of 128 consecutive k of one row (the last may be shorter); per group one
// exponent e in [-15, 7], the smallest with absmax <= 448 * 2^e (all-zero group: -15); per weight one OCP e4m3fn byte
// q = rne_sat(w * 2^-e).  The dequantised weight q * 2^e is an fp16 number by construction (2^-9 * 2^-15 = the smallest fp16
// subnormal, 448 * 2^7 < 65 504), so the FP8 kernel - bytes -> f32 (v_cvt_pk_f32_fp8) -> f16 -> x 2^e, all exact - hands the
// MFMAs the very half8 fragments the fp16 kernel reads from the dequantised matrix: same bytes out (gemm_skinny.inc: one kernel text for both).
//
// Device order of the bytes: rows of ldq = K rounded up to 256 bytes; within a 256-k chunk (16 K steps) the 8 bytes lane half hh
// needs at step ws = w + 8 j (w = the wave that owns the step, j = 0 / 1: its two steps of the chunk) sit at
// 32 w + 16 hh + 8 j, so ONE 16-byte load holds a lane's fragments for two of its own K steps and a wave reads 32 contiguous
// bytes per row as the fp16 kernel does.  Exponents: int8 [N][lde], lde = groups rounded up to 4 - a wave's four steps in flight
// lie in four consecutive groups, one dword.
#pragma once
#include "gemm.h"

struct GemmW8 {
  const uint8_t* q;     // e4m3fn bytes in device order, row stride ldq
  const int8_t* exps;   // group exponents, row stride lde
  int ldq, lde;
};
inline int fp8_ldq(int K) { return (K + 255) & ~255; }
inline int fp8_groups(int K) { return (K + 127) / 128; }
inline int fp8_lde(int K) { return (fp8_groups(K) + 3) & ~3; }

// byte offset of weight k within its row of the device order
__host__ __device__ __forceinline__ int fp8_dev_offset(int k) {
  const int s = k >> 4, r = k & 15;
  return (s >> 4) * 256 + (s & 7) * 32 + (r >> 3) * 16 + ((s >> 3) & 1) * 8 + (r & 7);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// eight e4m3fn bytes (a = k 0..3, b = k 4..7) x 2^e -> the half8 fragment.  Exact at every stage: e4m3 -> f32 -> f16 (an e4m3
// number has four significant bits and lies in [2^-9, 448]), then x 2^e in fp16 (v_pk_mul_f16 by ldexp(1, e); 2^-15 is an fp16
// subnormal, fp16 denormals are never flushed on this target) - the product is an fp16 number by the format's construction, so the
// one rounding of the multiply does nothing.  Pairs stay pairs: one v_cvt_pk_f32_fp8, one v_cvt_pk_f16_f32 and one v_pk_mul_f16
// per two weights, two registers of temporaries.  (Scaling in f32 - v_pk_mul_f32 between the two conversions - is the same bits
// and cost 8 VGPRs of temporaries per step: the kernel then needed 64 / 80 / 94 VGPRs against the fp16 forms' 56 / 76 / 76.)
__device__ __forceinline__ half8 fp8_frag(unsigned a, unsigned b, int e) {
  const half_t sc = __builtin_ldexpf16((half_t)1.0f, e);
  const half2v sc2 = {sc, sc};
  const half2v h0 = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)a, false), half2v) * sc2;
  const half2v h1 = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)a, true), half2v) * sc2;
  const half2v h2 = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)b, false), half2v) * sc2;
  const half2v h3 = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)b, true), half2v) * sc2;
  const u32x4 v = {__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1), __builtin_bit_cast(unsigned, h2), __builtin_bit_cast(unsigned, h3)};
  return __builtin_bit_cast(half8, v);
}

// How a wave of the weight-streaming kernel obtains its MFMA A fragments from FP8 step weights.  The lane's rows are 32-bit byte
// offsets from the (uniform) bases - one VGPR each where the fp16 form holds a 64-bit pointer (plan: N * ldq < 4 GiB) - and they
// RUN: qcur / ecur point at the wave's next 32 K steps and the main loop advances them, so nothing but them stays live for the
// tail loop.  Main loop, s = wave + 32 i: steps s, s + 8 are the wave's two of chunk 2i (one 16-byte piece at qcur), s + 16,
// s + 24 those of chunk 2i + 1 (qcur + 256), and their groups 4i .. 4i + 3 are one aligned dword of exponents at ecur.
template <int NT>
struct SkinnyFeedFp8 {
  struct Raw { u32x4 q[2]; int e; };   // the four K steps of a trip: two 16-byte pieces (two steps each) and their four exponents
  const uint8_t* q; const int8_t* exps;
  unsigned qcur[NT], ecur[NT];
  __device__ __forceinline__ SkinnyFeedFp8(const GemmArgs& p, const GemmW8& w, int n0, int l31, int hh, int wave) : q(w.q), exps(w.exps) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      int n = n0 + t * 32 + l31;
      n = n < p.N ? n : p.N - 1;
      qcur[t] = (unsigned)n * (unsigned)w.ldq + 16u * hh + 32u * wave;
      ecur[t] = (unsigned)n * (unsigned)w.lde;
    }
  }
  // requested with the activation fragments (u = 0): the exponents and the first piece ...
  __device__ __forceinline__ void load(Raw& r, int t, int u) const {
    if (u == 0) {
      r.e = *(const int*)(exps + (size_t)ecur[t]);
      r.q[0] = *(const u32x4*)(q + (size_t)qcur[t]);
    }
  }
  // ... and the second piece behind the first step's MFMA: two steps' bytes live at a time, which is what the compiler makes of
  // the fp16 kernel's four loads too (two and two), and what lets this kernel fit the fp16 forms' registers (56 / 76 / 74 VGPRs
  // against 56 / 76 / 76).  With both pieces requested up front: 62 / 78 / 80.
  __device__ __forceinline__ half8 frag(Raw& r, int t, int u) const {
    if (u == 1) r.q[1] = *(const u32x4*)(q + (size_t)qcur[t] + 256);
    const u32x4 v = r.q[u >> 1];
    return fp8_frag(v[(u & 1) * 2], v[(u & 1) * 2 + 1], (int)((unsigned)r.e << (24 - 8 * u)) >> 24);
  }
  __device__ __forceinline__ void advance() {
#pragma unroll
    for (int t = 0; t < NT; ++t) { qcur[t] += 512u; ecur[t] += 4u; }
  }
  // one step alone (the tail loop): step s is number j = (s >> 3) & 3 of the 32 the next trip of the main loop would have taken
  __device__ __forceinline__ half8 step(int t, int s) const {
    const unsigned j = ((unsigned)s >> 3) & 3u;
    const int e = exps[(size_t)(ecur[t] + j)];
    const u32x2 v = *(const u32x2*)(q + (size_t)(qcur[t] + (j >> 1) * 256u + (j & 1u) * 8u));
    return fp8_frag(v[0], v[1], e);
  }
};

// gemm_skinny_fp8_kernel<EPI, NT>: the weight-streaming kernel on FP8 step weights - gemm_skinny_kernel's text (gemm_skinny.inc), its
// fragments from SkinnyFeedFp8.  One batch (blockIdx.y = 0; p.bsW = 0).
#define SKINNY_KERNEL gemm_skinny_fp8_kernel
#define SKINNY_FP8 1
#include "gemm_skinny.inc"
#undef SKINNY_KERNEL
#undef SKINNY_FP8

// ---- quantiser -------------------------------------------------------------------------------------------------------
struct QuantFp8Args {
  const half_t* W; int ldw;      // [N][K] fp16
  int N, K;
  uint8_t* q; int ldq;           // bytes, device order (null: not written)
  int8_t* exps; int lde;         // group exponents
  uint8_t* q_rm;                 // bytes row-major [N][K] (null: not written; the debug read-back)
  half_t* deq; int ldd;          // dequantised fp16 (null: not written; may be W itself)
};

// smallest e with a <= 448 * 2^e, clamped: a = m 2^x (1 <= m < 2), 448 = 1.75 * 2^8 -> e = x - 8 + (m > 1.75).  Integer arithmetic
// on the bits of a as f32 (every fp16 number, subnormals included, is a normal f32).
__device__ __forceinline__ int fp8_group_exp(float absmax) {
  const unsigned b = __builtin_bit_cast(unsigned, absmax);
  int e = (int)(b >> 23) - 127 - 8 + ((b & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  return e < -15 ? -15 : (e > 7 ? 7 : e);
}

// OCP e4m3fn byte of x, round to nearest even, saturating at 448 (written out: independent of any rounding-mode or overflow
// setting of the conversion instructions)
__device__ __forceinline__ unsigned fp8_encode(float x) {
  const unsigned sign = (__builtin_bit_cast(unsigned, x) >> 24) & 0x80u;
  float a = fabsf(x);
  a = a < 448.f ? a : 448.f;
  unsigned mag;
  if (a < 0.015625f) {                                   // below the smallest normal 2^-6: multiples of 2^-9
    mag = (unsigned)(int)rintf(a * 512.f);               // 0 .. 8 (8 = the encoding of 2^-6)
  } else {
    unsigned b = __builtin_bit_cast(unsigned, a);
    b += 0x7FFFFu + ((b >> 20) & 1u);                    // RNE at three mantissa bits
    mag = (b >> 20) - ((127u - 7u) << 3);
  }
  return sign | mag;
}
__device__ __forceinline__ float fp8_decode(unsigned byte) {
  const unsigned ex = (byte >> 3) & 15u, mant = byte & 7u;
  const float a = ex ? __builtin_bit_cast(float, ((ex + 120u) << 23) | (mant << 20)) : (float)mant * 0.001953125f;
  return (byte & 0x80u) ? -a : a;
}

// One wave per (row, group of 128 k), two weights per lane.  Deterministic: the group maximum through a fixed shuffle tree, the
// exponent in integers, no atomics.  deq may be W: a lane reads its pair before anything of the group is written (the shuffles).
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(QuantFp8Args p) {
  // grid: ceil(groups / 4) workgroups per row, rows folded into blockIdx.x (any N: no 65 535-row limit of a grid's y)
  const int groups = (p.K + 127) >> 7, per_row = (groups + 3) >> 2;
  const int lane = threadIdx.x & 63, n = blockIdx.x / per_row, g = (blockIdx.x - n * per_row) * 4 + (threadIdx.x >> 6);
  if (g >= groups) return;
  const int k = g * 128 + 2 * lane;
  const bool ok = k < p.K;                                // K % 16: a pair is inside or outside together
  half2v w = {(half_t)0.f, (half_t)0.f};
  if (ok) w = *(const half2v*)(p.W + (size_t)n * p.ldw + k);
  const float w0 = (float)w[0], w1 = (float)w[1];
  const float amax = wave_max(fmaxf(fabsf(w0), fabsf(w1)));
  const int e = fp8_group_exp(amax);
  if (lane == 0) p.exps[(size_t)n * p.lde + g] = (int8_t)e;
  if (!ok) return;
  const float down = __builtin_bit_cast(float, (127 - e) << 23), up = __builtin_bit_cast(float, (127 + e) << 23);
  const unsigned q0 = fp8_encode(w0 * down), q1 = fp8_encode(w1 * down);
  const unsigned short pair = (unsigned short)(q0 | (q1 << 8));
  if (p.q) *(unsigned short*)(p.q + (size_t)n * p.ldq + fp8_dev_offset(k)) = pair;
  if (p.q_rm) *(unsigned short*)(p.q_rm + (size_t)n * p.K + k) = pair;
  if (p.deq) *(half2v*)(p.deq + (size_t)n * p.ldd + k) = half2v{(half_t)(fp8_decode(q0) * up), (half_t)(fp8_decode(q1) * up)};
}
