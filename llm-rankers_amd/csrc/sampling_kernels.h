// sampling_kernels.h — the sampling head of the decoder-only path (rk_llama_generate_sampled, sampled decoding sessions).
//
// sample_rows_kernel draws one token per row from full-vocabulary fp32 logits, in HF's order of logits processors
// (hf: generation/logits_process.py TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, then softmax and one
// multinomial draw; generation/utils.py _sample).  One workgroup per row; a row of a 152k vocabulary (608 KB) does not fit in
// LDS, so every pass reads it again from L2.  Nothing is sorted:
//   keys       z_i = x_i / T (fp32, HF's division) mapped to an unsigned int that orders like the float
//   top-k      radix select over the keys, 8 bits per level, COUNTS per bucket, from the top: the min(k, V)-th largest key; every
//              key >= it is kept (ties at the threshold all stay, as in HF)
//   top-p      radix select over the keys of what top-k kept, MASS per bucket, from the bottom: the smallest key whose tail mass
//              (all kept keys <= it) exceeds (1 - p) Z; every key >= it is kept.  The largest key's tail is Z itself: always kept
//   weights    w_i = expf((x_i - max x) / T) in (0, 1], turned into 2^-40 fixed point (a 64-bit integer).  Every sum over
//              weights - bucket masses, Z, the running sums of the draw - is an INTEGER sum: exact, so its order does not matter
//              and the LDS atomics that build the histograms cannot make two runs differ.  What is left of the error is the
//              weights' own: expf and the division (a few ulp each) and 2^-40 of truncation per id
//   draw       u = (first word of Philox4x32-10 >> 8) 2^-24 with key = the row's 64-bit seed and counter = (token index, 0, 0, 0);
//              the token is the first kept id in vocabulary order whose running sum exceeds u Z: sums per 256-id segment, a scan
//              over the segments, then one wave walks the segment that holds the crossing
// A row's token is a function of its logit bits, (T, k, p), its seed and its token index: nothing else enters the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sampling {

constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int SEG = 256;              // ids per segment of the draw's first level: four coalesced loads of a wave
constexpr int MAX_SEGS = 4096;        // segment sums held in LDS; beyond 2^20 ids a segment grows by whole multiples of SEG
constexpr float FIX_ONE = 1099511627776.0f;   // 2^40: the fixed-point image of weight 1
constexpr int MAX_VOCAB = 1 << 23;            // ids per row: 2^23 weights of 1 are 2^63, the last sum that fits

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter c[4], key (k0, k1)
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// the unsigned image of a float: a < b as floats <=> key(a) < key(b); -0 is taken as +0 (they compare equal)
__device__ inline uint32_t order_key(float z) {
  if (z == 0.f) z = 0.f;
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline uint64_t fixed_weight(float x, float mx, float T) {
  const float w = expf((x - mx) / T);
  return w > 0.f ? (uint64_t)(w * FIX_ONE) : 0ull;       // (NaN: 0)
}

__device__ inline uint64_t shfl_up64(uint64_t v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t shfl_xor64(uint64_t v, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t wave_scan(uint64_t v, int lane) {   // inclusive, lanes in order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = shfl_up64(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ inline uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor64(v, o);
  return v;
}
// inclusive scan over the workgroup's threads in order; *total = the sum over all.  wtot: WAVES words of LDS, free on return
__device__ inline uint64_t block_scan(uint64_t v, uint64_t* wtot, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t incl = wave_scan(v, lane);
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  uint64_t below = 0, all = 0;
  for (int w = 0; w < WAVES; ++w) { const uint64_t t = wtot[w]; if (w < wave) below += t; all += t; }
  __syncthreads();
  *total = all;
  return incl + below;
}

// f(i, x[i]) for every id of the row, the workgroup's threads striding over it; eight independent loads are issued before the first
// is used (one workgroup has a whole row to itself: what it waits for is the latency of L2, not its bandwidth).  The order in which
// ids are visited carries no weight: every accumulation behind f is a maximum or an integer sum.
template <class F>
__device__ inline void for_each_logit(const float* __restrict__ x, int V, F&& f) {
  constexpr int U = 8;
  for (int i0 = threadIdx.x; i0 < V; i0 += THREADS * U) {
    float v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) { const int i = i0 + j * THREADS; v[j] = i < V ? x[i] : 0.f; }
#pragma unroll
    for (int j = 0; j < U; ++j) { const int i = i0 + j * THREADS; if (i < V) f(i, v[j]); }
  }
}

// One level of a radix select: hist[256] holds, per value of the key's next 8 bits, the count or mass of the candidates.  Walks
// the buckets from the top (down) or the bottom and picks the one in which the running sum first exceeds thr - *base (what the
// buckets passed at the levels above held); *base grows by what was passed here.  Returns the bucket, or -1: thr is not below
// the total.  sh: 2 words of LDS.
__device__ inline int pick_bucket(const uint64_t* hist, bool down, uint64_t thr, uint64_t* base, uint64_t* wtot, uint64_t* sh) {
  const int tid = threadIdx.x;
  if (tid == 0) { sh[0] = ~0ull; sh[1] = 0; }
  const int b = down ? 255 - tid : tid;
  uint64_t total;
  const uint64_t incl = block_scan(tid < 256 ? hist[b] : 0ull, wtot, &total);   // (its barriers order the write above)
  const uint64_t v = tid < 256 ? hist[b] : 0ull, excl = incl - v;
  if (tid < 256 && v && *base + excl <= thr && thr < *base + incl) { sh[0] = (uint64_t)b; sh[1] = excl; }
  __syncthreads();
  const uint64_t got = sh[0];
  *base += sh[1];
  __syncthreads();
  return got == ~0ull ? -1 : (int)got;
}

}  // namespace sampling

// logits [n_logit_rows][ldl] fp32: row r reads row r % n_logit_rows (the engine passes its row count; rk_debug_sample draws many
// (seed, index) pairs from a few rows).  seeds[seed_map ? seed_map[r] : r]; the token index is pos[pos_map ? pos_map[r] : r] +
// pos_add: the decoders keep the position of the LAST token of every row on the device (pos_add = 1), so a replayed graph moves
// along the Philox stream with no host write.  temperature > 0; top_k <= 0 or >= V: off; top_p >= 1: off.
// out[r] = the token; kept (optional) [rows][2] = ids kept after top-k, after top-p.
__global__ __launch_bounds__(sampling::THREADS) void sample_rows_kernel(const float* __restrict__ logits, int n_logit_rows, long ldl, int V,
                                                                        float T, int top_k, float top_p,
                                                                        const unsigned long long* __restrict__ seeds, const int* __restrict__ seed_map,
                                                                        const int* __restrict__ pos, const int* __restrict__ pos_map, int pos_add,
                                                                        int* __restrict__ out, int* __restrict__ kept) {
  using namespace sampling;
  __shared__ uint64_t hist[256];
  __shared__ uint64_t segs[MAX_SEGS];
  __shared__ uint64_t wtot[WAVES];
  __shared__ uint64_t sh[4];
  __shared__ float wmax[WAVES];
  __shared__ int wcnt[2 * WAVES];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (size_t)(row % n_logit_rows) * ldl;

  // ---- the largest key and its first id (the token if no weight survives), the largest logit ----
  uint64_t best = 0;
  float mx = -INFINITY;
  for_each_logit(x, V, [&](int i, float v) {
    const uint64_t c = ((uint64_t)order_key(v / T) << 32) | (uint32_t)~(uint32_t)i;
    best = c > best ? c : best;
    mx = fmaxf(mx, v);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t ob = shfl_xor64(best, o);
    best = ob > best ? ob : best;
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  if (lane == 0) { wtot[wave] = best; wmax[wave] = mx; }
  __syncthreads();
  for (int w = 0; w < WAVES; ++w) { best = wtot[w] > best ? wtot[w] : best; mx = fmaxf(mx, wmax[w]); }
  __syncthreads();
  const uint32_t key_max = (uint32_t)(best >> 32);
  const int first_max = (int)~(uint32_t)best;

  // ---- top-k: the min(k, V)-th largest key ----
  uint32_t key_k = 0;
  if (top_k > 0 && top_k < V) {
    uint64_t base = 0;
    uint32_t prefix = 0;
    for (int level = 0; level < 4; ++level) {
      const int shift = 24 - 8 * level;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for_each_logit(x, V, [&](int, float v) {
        const uint32_t key = order_key(v / T);
        if (level == 0 || (key >> (shift + 8)) == prefix) atomicAdd((unsigned long long*)&hist[(key >> shift) & 255], 1ull);
      });
      __syncthreads();
      const int b = pick_bucket(hist, true, (uint64_t)top_k - 1, &base, wtot, sh);
      prefix = (prefix << 8) | (uint32_t)(b < 0 ? 0 : b);
    }
    key_k = prefix;
  }

  // ---- top-p over what top-k kept: the smallest key whose tail mass exceeds (1 - p) Z ----
  uint32_t key_p = 0;
  if (top_p < 1.f) {
    uint64_t base = 0, thr = 0;
    uint32_t prefix = 0;
    bool found = true;
    for (int level = 0; level < 4 && found; ++level) {
      const int shift = 24 - 8 * level;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for_each_logit(x, V, [&](int, float v) {
        const uint32_t key = order_key(v / T);
        if (key >= key_k && (level == 0 || (key >> (shift + 8)) == prefix)) {
          const uint64_t q = fixed_weight(v, mx, T);
          if (q) atomicAdd((unsigned long long*)&hist[(key >> shift) & 255], (unsigned long long)q);
        }
      });
      __syncthreads();
      if (level == 0) {                                   // Z of what top-k kept: the sum of the first level's buckets
        uint64_t z;
        block_scan(tid < 256 ? hist[tid] : 0ull, wtot, &z);
        thr = (uint64_t)((1.0 - (double)top_p) * (double)z);   // a running sum s (an integer) exceeds (1 - p) Z <=> s > floor
      }
      const int b = pick_bucket(hist, false, thr, &base, wtot, sh);
      found = b >= 0;
      prefix = (prefix << 8) | (uint32_t)(found ? b : 0);
    }
    key_p = found ? prefix : key_max;                     // no weight at all (every logit -inf or NaN): the largest alone
  }
  const uint32_t key_f = key_k > key_p ? key_k : key_p;

  // ---- the draw, level 1: the kept weight of every segment of seg_len consecutive ids (and the two kept counts) ----
  const int per_seg = (int)(((long)V + (long)SEG * MAX_SEGS - 1) / ((long)SEG * MAX_SEGS));   // wave loads of 256 ids per segment: 1 up to 2^20 ids
  const long seg_len = (long)SEG * per_seg;
  const int n_segs = (int)((V + seg_len - 1) / seg_len);
  int cnt_k = 0, cnt_p = 0;
  for (int s = wave; s < n_segs; s += WAVES) {
    uint64_t sum = 0;
    for (int jj = 0; jj < per_seg; ++jj) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { const long i = s * seg_len + (long)(4 * jj + j) * 64 + lane; v[j] = i < V ? x[i] : 0.f; }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long i = s * seg_len + (long)(4 * jj + j) * 64 + lane;
        if (i < V) {
          const uint32_t key = order_key(v[j] / T);
          cnt_k += key >= key_k;
          if (key >= key_f) { ++cnt_p; sum += fixed_weight(v[j], mx, T); }
        }
      }
    }
    sum = wave_sum(sum);
    if (lane == 0) segs[s] = sum;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { cnt_k += __shfl_xor(cnt_k, o); cnt_p += __shfl_xor(cnt_p, o); }
  if (lane == 0) { wcnt[wave] = cnt_k; wcnt[WAVES + wave] = cnt_p; }
  if (tid == 0) { sh[2] = ~0ull; sh[3] = 0; }
  __syncthreads();
  if (kept && tid == 0) {
    int a = 0, b = 0;
    for (int w = 0; w < WAVES; ++w) { a += wcnt[w]; b += wcnt[WAVES + w]; }
    kept[2 * row] = a; kept[2 * row + 1] = b;
  }

  // ---- level 2: Z, the target u Z, the segment in which the running sum first exceeds it ----
  uint32_t ctr[4] = {(uint32_t)(pos[pos_map ? pos_map[row] : row] + pos_add), 0u, 0u, 0u};
  const unsigned long long seed = seeds[seed_map ? seed_map[row] : row];
  philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t u24 = ctr[0] >> 8;
  uint64_t mine[4], local = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { const int s = 4 * tid + j; mine[j] = s < n_segs ? segs[s] : 0ull; local += mine[j]; }
  uint64_t Z;
  const uint64_t incl = block_scan(local, wtot, &Z);
  // floor(u24 Z / 2^24) from the 88-bit product: a running sum (an integer) exceeds u Z <=> it exceeds the floor
  const uint64_t target = (__umul64hi(Z, u24) << 40) | ((Z * u24) >> 24);
  if (local && incl - local <= target && target < incl) {
    uint64_t run = incl - local;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (mine[j] && run <= target && target < run + mine[j]) { sh[2] = (uint64_t)(4 * tid + j); sh[3] = run; }
      run += mine[j];
    }
  }
  __syncthreads();

  // ---- level 3: one wave walks the segment, 64 ids at a time in vocabulary order ----
  if (wave != 0) return;
  if (sh[2] == ~0ull) {                                    // Z = 0: no weight survived
    if (lane == 0) out[row] = first_max;
    return;
  }
  const long s0 = (long)sh[2] * seg_len;
  uint64_t run = sh[3];
  for (int j = 0; j < 4 * per_seg; ++j) {
    const long i = s0 + (long)j * 64 + lane;
    uint64_t q = 0;
    if (i < V) {
      const float v = x[i];
      if (order_key(v / T) >= key_f) q = fixed_weight(v, mx, T);
    }
    const uint64_t sc = wave_scan(q, lane);
    if (q && run + sc - q <= target && target < run + sc) out[row] = (int)i;
    run += shfl64(sc, 63);
    if (run > target) return;
  }
}
