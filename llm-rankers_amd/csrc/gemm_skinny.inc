// The weight-streaming kernel, compiled once per weight format (gemm.h, gemm_fp8.h):
//   SKINNY_KERNEL  the kernel's name
//   SKINNY_FP8     0: W is the fp16 matrix, a fragment is one 16-byte load (GemmArgs p)
//                  1: FP8 step weights (GemmArgs p, GemmW8 w8): SkinnyFeedFp8 loads bytes and exponents and converts them to the half8
//                     fragment the fp16 form would have read from the dequantised matrix
// Everything outside the `#if SKINNY_FP8` blocks - K order, MFMA calls, reduction tree, epilogues - is one text, so the two
// forms produce the same bytes from the same fragments.
template <int EPI, int NT>
#if SKINNY_FP8
// (waves per SIMD asked of the scheduler: 8 / 6 / 6 are what the fp16 store / residual / SwiGLU forms reach at 56 / 76 / 76 VGPRs.
// With the target the FP8 forms take 56 / 76 / 74; without it the scheduler converts several steps' bytes up front and they take more)
__global__ __launch_bounds__(SKINNY_THREADS, (EPI == EPI_STORE_F16 ? 8 : 6)) void SKINNY_KERNEL(GemmArgs p, GemmW8 w8) {
#else
__global__ __launch_bounds__(SKINNY_THREADS) void SKINNY_KERNEL(GemmArgs p) {
#endif
  __shared__ float red[4 * NT * 1024];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int l31 = lane & 31, hh = lane >> 5;
  const int n0 = blockIdx.x * 32 * NT;
  const int nsteps = p.K >> 4;
  const int mrow0 = blockIdx.z * 32;          // more than 32 rows: one workgroup per 32-row slab (weights re-read via L2)
  const int m = mrow0 + l31 < p.M ? mrow0 + l31 : p.M - 1;
  p.A += (size_t)blockIdx.y * p.bsA;          // batched form: one small GEMM per blockIdx.y (e.g. per attention head)
  p.W += (size_t)blockIdx.y * p.bsW;
  p.C = (char*)p.C + (size_t)blockIdx.y * p.bsC * ((EPI == EPI_RESID_F32 || EPI == EPI_STORE_F32 || EPI == EPI_ARGMAX_F32) ? 4 : 2);
  const half_t* arow = p.A + (size_t)m * p.lda + 8 * hh;
#if SKINNY_FP8
  SkinnyFeedFp8<NT> feed(p, w8, n0, l31, hh, wave);
#else
  const half_t* wrow[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int n = n0 + t * 32 + l31;
    n = n < p.N ? n : p.N - 1;
    wrow[t] = p.W + (size_t)n * p.ldw + 8 * hh;
  }
#endif
  f32x16 acc[NT][1];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][0][r] = 0.f;
  // Wave 0 writes the result: what its epilogue reads besides the accumulators is requested now and travels under the
  // weight stream - the old fp32 rows of a residual add (registers), the block sums of squares of a folded RMSNorm (DMA
  // straight into LDS: no registers held across the main loop, the occupancy of this kernel is what hides its latency).
  __shared__ f32x4 sqs[8 * 64];                 // [instruction][lane]: float4 2i + (lane >> 5) of row (lane & 31)
  f32x4 old[EPI == EPI_RESID_F32 ? 4 : 1];
  float rowfac = 1.f;
  const bool row_ok = mrow0 + l31 < p.M;
  const bool sq_here = p.ssq_in && !p.rowscale;
  const bool sq_dma = sq_here && (p.nb_in & 3) == 0 && p.nb_in <= 64;
  if (wave == 0) {
    if constexpr (EPI == EPI_RESID_F32) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + 8 * q + 4 * hh;
        old[q] = (row_ok && n < p.N) ? *(const f32x4*)((const float*)p.C + (size_t)m * p.ldc + n) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if (p.rowscale) rowfac = p.rowscale[m];
    else if (sq_dma) {
      const int nq = p.nb_in >> 2;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (2 * i < nq) {
          const int j = 2 * i + hh < nq ? 2 * i + hh : nq - 1;
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.ssq_in + (size_t)m * p.nb_in + 4 * j),
                                           (__attribute__((address_space(3))) void*)(sqs + i * 64), 16, 0, 0);
        }
      }
    }
  }
  int s = wave;
  for (; s + 24 < nsteps; s += 32) {
#if SKINNY_FP8
    half8 bf[4];
    typename SkinnyFeedFp8<NT>::Raw raw[NT];
#define SKINNY_LOAD(u, t, k) feed.load(raw[t], t, u)
#define SKINNY_FRAG(u, t) feed.frag(raw[t], t, u)
#else
    half8 bf[4], wf[4][NT];
#define SKINNY_LOAD(u, t, k) wf[u][t] = *(const half8*)(wrow[t] + k)
#define SKINNY_FRAG(u, t) wf[u][t]
#endif
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = (s + 8 * u) << 4;
      bf[u] = *(const half8*)(arow + k);
#pragma unroll
      for (int t = 0; t < NT; ++t) SKINNY_LOAD(u, t, k);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(SKINNY_FRAG(u, t), bf[u], acc[t][0], 0, 0, 0);
#undef SKINNY_LOAD
#undef SKINNY_FRAG
#if SKINNY_FP8
    feed.advance();
#endif
  }
  for (; s < nsteps; s += 8) {
    const int k = s << 4;
    const half8 bf = *(const half8*)(arow + k);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#if SKINNY_FP8
      const half8 wf = feed.step(t, s);
#else
      const half8 wf = *(const half8*)(wrow[t] + k);
#endif
      acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, bf, acc[t][0], 0, 0, 0);
    }
  }
  // fixed reduction tree: (w, w+4) -> w ; (w, w+2) -> w ; (0, 1) -> 0
#pragma unroll
  for (int half_n = 4; half_n >= 1; half_n >>= 1) {
    if (wave >= half_n && wave < 2 * half_n) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[((wave - half_n) * NT + t) * 1024 + r * 64 + lane] = acc[t][0][r];
    }
    __syncthreads();
    if (wave < half_n) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][0][r] += red[(wave * NT + t) * 1024 + r * 64 + lane];
    }
    __syncthreads();
  }
  if (wave != 0) return;
  if (sq_here) {
    // blocks added in increasing order, whatever the path (the DMA landed long ago: every barrier above drained vmcnt)
    float ssum = 0.f;
    if (sq_dma) {
      const int nq = p.nb_in >> 2;
      for (int j = 0; j < nq; ++j) {
        const f32x4 v = sqs[(j >> 1) * 64 + (j & 1) * 32 + l31];
        ssum += v[0]; ssum += v[1]; ssum += v[2]; ssum += v[3];
      }
    } else {
      for (int j = 0; j < p.nb_in; ++j) ssum += p.ssq_in[(size_t)m * p.nb_in + j];
    }
    rowfac = rsqrtf(ssum / (float)p.K + p.eps_in) / p.xs;
  }
  if constexpr (EPI == EPI_RESID_F32) {
    // C += acc (old rows prefetched above); with p.xraw also the fp16 copy of the new row and the sum of squares of this
    // workgroup's 32 columns (producer side of the next folded norm): a lane holds 16 of them, its partner (lane ^ 32) the rest
    const float sc = p.scale * rowfac;
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + 8 * q + 4 * hh;
      const bool ok = row_ok && n < p.N;
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = old[q][j] + acc[0][0][4 * q + j] * sc;
      if (ok) {
        *(f32x4*)((float*)p.C + (size_t)m * p.ldc + n) = o;
        if (p.xraw) {
#pragma unroll
          for (int j = 0; j < 4; ++j) ss = __builtin_fmaf(o[j], o[j], ss);
          const half4 xr = {f2h_sat(o[0] * p.xs), f2h_sat(o[1] * p.xs), f2h_sat(o[2] * p.xs), f2h_sat(o[3] * p.xs)};
          *(half4*)(p.xraw + (size_t)m * p.ldx + n) = xr;
        }
      }
    }
    if (p.xraw) {
      ss += __shfl_xor(ss, 32);
      if (hh == 0 && row_ok) p.ssq[(size_t)m * p.nb + (n0 >> 5)] = ss;
    }
  } else if constexpr (EPI == EPI_ARGMAX_F32) {
    // the logits of this block never reach memory: largest value and its FIRST column (torch.argmax tie rule) among the
    // workgroup's 32 columns; argmax_blocks_kernel finishes the row
    const float sc = p.scale * rowfac;
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + 8 * q + 4 * hh + j;
        const float v = acc[0][0][4 * q + j] * sc;
        if (n < p.N && (v > best || (v == best && n < bi))) { best = v; bi = n; }
      }
    const float ov = __shfl_xor(best, 32);
    const int oi = __shfl_xor(bi, 32);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    if (hh == 0 && row_ok) {
      ((float*)p.C)[(size_t)m * p.ldc + blockIdx.x] = best;
      p.amax_idx[(size_t)m * p.ldc + blockIdx.x] = bi;
    }
  } else {
    gemm_epilogue<EPI, NT, 1>(p, acc, mrow0, n0, l31, hh, rowfac);
  }
}

