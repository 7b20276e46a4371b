// HBM-bound helper kernels (embedding gather, RMSNorm, head rows, pair verdict, argmax, cross-entropy) for gfx950.
// One wave (64 lanes) per row, 16-byte vector accesses, shuffle reductions.
#pragma once
#include "common.h"
#include "decode_ints.h"

// hf: modeling_t5.py:644,678 (embed_tokens): hidden[t][:] = (fp32) E[ids[t]][:]; no scaling, dropout = identity.
// Folded-norm form of the encoder (xraw != nullptr): the row also goes out as fp16 x xs (A operand of the first QKV GEMM)
// with its RMSNorm row factor rsqrt(mean(x^2) + eps) / xs (GemmArgs::rowscale).
__global__ __launch_bounds__(256) void embed_gather_kernel(const int* __restrict__ ids, const half_t* __restrict__ table,
                                                           float* __restrict__ out, int n_rows, int d, int vocab,
                                                           half_t* __restrict__ xraw, float* __restrict__ rowscale,
                                                           float xs, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);   // host validates; clamp keeps a bad id from faulting
  const half_t* src = table + (size_t)id * d;
  float* dst = out + (size_t)row * d;
  float ss = 0.f;
  for (int c = lane * 8; c < d; c += 64 * 8) {
    const half8 v = *(const half8*)(src + c);
    f32x4 a = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    f32x4 b = {(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
    *(f32x4*)(dst + c) = a;
    *(f32x4*)(dst + c + 4) = b;
    if (xraw) {
      half8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float x = (float)v[j]; ss += x * x; o[j] = f2h_sat(x * xs); }
      *(half8*)(xraw + (size_t)row * d + c) = o;
    }
  }
  if (xraw) {
    ss = wave_sum(ss);
    if (lane == 0) rowscale[row] = rsqrtf(ss / (float)d + eps) / xs;
  }
}

// Folded RMSNorm, statistics step: the fp32-residual GEMM epilogue left the sums of squares of every new row per
// 64-column block in ssq [n_rows, nb] (gemm.h); rowscale[m] = rsqrt(sum_j ssq[m][j] / d + eps) / xs, blocks added in
// increasing order.  hf: modeling_t5.py:59-72 computes the same fp32 mean of squares.
__global__ __launch_bounds__(256) void rowscale_kernel(const float* __restrict__ ssq, float* __restrict__ rowscale,
                                                       int n_rows, int nb, int d, float eps, float xs) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  rowscale[row] = rk_row_factor(ssq + (size_t)row * nb, nb, d, eps, xs);
}

// hf: modeling_t5.py:59-72 (T5LayerNorm): y = w * x * rsqrt(mean(x^2) + eps); fp32 statistics, fp16 result
// (the GEMM input).  row_map (optional) gathers source rows: out row r reads x row row_map[r].
// One wave per row; the row (d <= 64*4*NV floats) stays in registers so HBM is read exactly once.
template <int NV>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      half_t* __restrict__ out, const int* __restrict__ row_map,
                                                      int n_rows, int d, float eps, float out_scale) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const float* src = x + (size_t)(row_map ? row_map[row] : row) * d;
  f32x4 v[NV];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane * 4 + i * 256;
    if (c < d) {
      v[i] = *(const f32x4*)(src + c);
      ss += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    }
  }
  ss = wave_sum(ss);
  const float rs = rsqrtf(ss / (float)d + eps) * out_scale;
  half_t* dst = out + (size_t)row * d;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane * 4 + i * 256;
    if (c < d) {
      const f32x4 g = *(const f32x4*)(w + c);
      half4 o = {f2h_sat(v[i][0] * rs * g[0]), f2h_sat(v[i][1] * rs * g[1]), f2h_sat(v[i][2] * rs * g[2]),
                 f2h_sat(v[i][3] * rs * g[3])};
      *(half4*)(dst + c) = o;
    }
  }
}

// dot(x row, head row) by one wave: 8 halves per lane and 512-column step, eight sequential fp32 adds per step, then the
// wave's butterfly sum.  The one order of additions behind every label logit (head_rows_kernel, pair_verdict_kernel).
__device__ __forceinline__ float head_row_dot(const half_t* __restrict__ xr, const half_t* __restrict__ hr, int d, int lane) {
  float s = 0.f;
  for (int c = lane * 8; c < d; c += 512) {
    const half8 a = *(const half8*)(xr + c);
    const half8 w = *(const half8*)(hr + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += (float)a[e] * (float)w[e];
  }
  return wave_sum(s);
}

// Final-token logit extraction for the label / yes-no rows only (hf: modeling_t5.py:1044-1047 lm_head, but
// just the n_out vocabulary rows the rankers read: ref pointwise.py:120-121, setwise.py:186).
// out[b][j] = dot(x[b], head[out_ids[j]]); one wave per (b, j).
__global__ __launch_bounds__(256) void head_rows_kernel(const half_t* __restrict__ x, const half_t* __restrict__ head,
                                                        const int* __restrict__ out_ids, float* __restrict__ out,
                                                        int n_seq, int n_out, int d) {
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (idx >= n_seq * n_out) return;
  const int b = idx / n_out, j = idx % n_out;
  const float s = head_row_dot(x + (size_t)b * d, head + (size_t)out_ids[j] * d, d, lane);
  if (lane == 0) out[idx] = s;
}

// The tail of a duoT5 compare (ref: llmrankers/pairwise.py:330-343) on the device: pair p = sequences 2p (the A/B prompt) and
// 2p + 1 (the B/A prompt).  One workgroup per pair; wave w computes the logit of sequence 2p + (w >> 1) for the id `false`
// (w even) or `true` (w odd) with head_rows_kernel's own dot product, so the logits are the ones rk_t5_score gives bit for
// bit.  The four sums meet in LDS and one thread takes, per ordering, the max-subtracted two-way softmax (torch's and
// _softmax_first's form; expf and IEEE division, no fast-math intrinsic) and the strict verdict P(true)[0] > P(true)[1].
// out: [0, 2 n_seq) logits [n_seq][2] = (false, true), rk_t5_score's place and layout for out ids {false, true};
//      [2 n_seq, 3 n_seq) P(true) per sequence;  [3 n_seq, 3 n_seq + n_seq / 2) the verdict per pair as 1.0f / 0.0f.
__global__ __launch_bounds__(256) void pair_verdict_kernel(const half_t* __restrict__ x, const half_t* __restrict__ head,
                                                           int false_id, int true_id, float* __restrict__ out,
                                                           int n_seq, int d) {
  __shared__ float sums[4];   // (false, true) logits of sequence 2p, then of 2p + 1
  const int p = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (2 * p + 1 >= n_seq) return;                      // (uniform per workgroup: no barrier is skipped by part of one)
  const int b = 2 * p + (wave >> 1);
  const float s = head_row_dot(x + (size_t)b * d, head + (size_t)((wave & 1) ? true_id : false_id) * d, d, lane);
  if (lane == 0) sums[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float pt[2];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const float f = sums[2 * o], t = sums[2 * o + 1];
      const float m = fmaxf(f, t);
      const float ef = expf(f - m), et = expf(t - m);
      pt[o] = et / (ef + et);
      out[(size_t)(2 * p + o) * 2] = f;
      out[(size_t)(2 * p + o) * 2 + 1] = t;
      out[(size_t)2 * n_seq + 2 * p + o] = pt[o];
    }
    out[(size_t)3 * n_seq + p] = pt[0] > pt[1] ? 1.0f : 0.0f;
  }
}

// Greedy decoding step, second half of the fused head: the weight-streaming head GEMM (EPI_ARGMAX_F32) left, per 32-column
// block, the row maximum and its first column; one workgroup per row picks the first index of the overall maximum
// (torch.argmax tie rule; hf: generation/utils.py greedy).
__global__ __launch_bounds__(256) void argmax_blocks_kernel(const float* __restrict__ bval, const int* __restrict__ bidx,
                                                            int n_blocks, int* __restrict__ out) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = tid; c < n_blocks; c += 256) {
    const float v = bval[(size_t)row * n_blocks + c];
    const int i = bidx[(size_t)row * n_blocks + c];
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { sv[wave] = best; si[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
    out[row] = bi;
  }
}

// Token feedback of rk_t5_generate's step graph, after argmax_blocks_kernel: the decoder just ran input position t = st[0].
// Prefix positions (t + 1 < dec_len) are forced: the next input is prefix[t + 1].  Otherwise column n = t + 1 - dec_len of the
// output gets the row's arg-max, or pad once the row has finished (hf: generation/utils.py greedy: finished rows emit pad); EOS
// finishes a row; the token is the row's next input.  st[1] (0 until then) becomes the number of columns the recompute loop of
// rk_t5_greedy would have produced: n + 1 at the column where the last row finished, or max_new.  The position advances, held
// at the cache's last row: a step enqueued after the end writes nothing but pads over pads.  One workgroup.
// st = {t, finished step, eos, pad}
__global__ __launch_bounds__(256) void greedy_advance_kernel(const int* __restrict__ argmax, int* st, const int* __restrict__ prefix,
                                                             int* done, int* out, int* next_ids, int n_seq, int dec_len, int max_new) {
  __shared__ int s_all;
  const int tid = threadIdx.x, t = st[0], eos = st[2], pad = st[3], n = t + 1 - dec_len;
  if (tid == 0) s_all = 1;
  __syncthreads();
  for (int b = tid; b < n_seq; b += 256) {
    int next = pad;
    if (n < 0) next = prefix[t + 1];
    else if (n < max_new) {
      const int tok = done[b] ? pad : argmax[b];
      out[(size_t)b * max_new + n] = tok;
      if (tok == eos) done[b] = 1;
      next = tok;
    }
    next_ids[b] = next;
    if (!done[b]) s_all = 0;
  }
  __syncthreads();
  if (tid == 0) {
    if (n >= 0 && n < max_new && st[1] == 0 && (s_all || n == max_new - 1)) st[1] = n + 1;
    st[0] = t + 1 < dec_len + max_new - 1 ? t + 1 : dec_len + max_new - 1;
  }
}

// Token feedback of rk_llama_generate, the sibling of greedy_advance_kernel for a decoder-only model: a SET of EOS ids and a limit
// on a row's total length.  st = the block's head, GenWord and the EOS ids from INTS_EOS0 on (decode_ints.h): column n = st[GEN_N] of the output gets
// the row's arg-max, or pad once the row has finished (hf: generation/utils.py greedy); a row finishes at one of the EOS ids or,
// with max_total > 0, once prompt + new tokens == max_total (hf: MaxLengthCriteria).  The token is the row's next input at
// position len[b] + n, held inside the cache.  st[GEN_FINISHED] (0 until then) becomes n + 1 at the column where the last row finished, or
// max_new.  A step enqueued after that writes pads over pads (every row has finished) or nothing (n == max_new).  One workgroup.
__global__ __launch_bounds__(256) void llama_advance_kernel(const int* __restrict__ argmax, int* st, const int* __restrict__ len,
                                                            int* done, int* pos, int* out, int* next_ids, int n_seq) {
  __shared__ int s_all;
  const int tid = threadIdx.x, n = st[GEN_N], pad = st[GEN_PAD], n_eos = st[GEN_N_EOS], max_new = st[GEN_MAX_NEW], max_total = st[GEN_MAX_TOTAL], P = st[GEN_P];
  if (n >= max_new) return;
  if (tid == 0) s_all = 1;
  __syncthreads();
  for (int b = tid; b < n_seq; b += 256) {
    const int tok = done[b] ? pad : argmax[b];
    out[(size_t)b * max_new + n] = tok;
    if (!done[b]) {
      bool fin = max_total > 0 && len[b] + n + 1 >= max_total;
      for (int k = 0; k < n_eos; ++k) fin = fin || tok == st[INTS_EOS0 + k];
      if (fin) done[b] = 1;
    }
    next_ids[b] = tok;
    const int p = len[b] + n;
    pos[b] = p < P - 1 ? p : P - 1;
    if (!done[b]) s_all = 0;
  }
  __syncthreads();
  if (tid == 0) {
    if (st[GEN_FINISHED] == 0 && (s_all || n == max_new - 1)) st[GEN_FINISHED] = n + 1;
    st[GEN_N] = n + 1;
  }
}

// Token feedback of a decoding session (rk_llama_session_*), the sibling of llama_advance_kernel for rows that start and end on
// their own: every cache slot has its prompt length, its own column counter, its own max_new and a done flag (1: idle or
// finished).  st = the block's head, SesWord and the EOS ids from INTS_EOS0 on (decode_ints.h).  An active slot's column col[b] gets its
// arg-max; the slot finishes at one of the EOS ids or at its max_new-th token; the token is its next input at position
// len[b] + col[b], held inside the cache.  A slot that is idle or done emits nothing, keeps its position, feeds pad and is not
// counted again: the step queued behind a finish changes nothing for that slot.  st[SES_FINISHES], the session word, is the running number
// of finishes (the host compares it with what it has seen).
// admit != null (rk_llama_session_admit, behind the prefill's head; admit = slot[n] | len[n] | max_new[n]): row r of argmax belongs
// to slot admit[r], which starts here with that prompt length and max_new; only those slots are touched.  One workgroup.
__global__ __launch_bounds__(256) void llama_session_advance_kernel(const int* __restrict__ argmax, int* st, int* len, int* col,
                                                                    int* max_new, int* done, int* pos, int* out, int* next_ids,
                                                                    int n_slots, const int* __restrict__ admit, int n_admit) {
  __shared__ int s_fin;
  const int tid = threadIdx.x, pad = st[SES_PAD], n_eos = st[SES_N_EOS], max_len = st[SES_MAX_LEN], cap = st[SES_CAP];
  if (tid == 0) s_fin = 0;
  __syncthreads();
  const int rows = admit ? n_admit : n_slots;
  for (int r = tid; r < rows; r += 256) {
    int b = r;
    if (admit) {
      b = admit[r];
      if (b < 0 || b >= n_slots) continue;
      len[b] = admit[n_admit + r]; max_new[b] = admit[2 * n_admit + r]; col[b] = 0; done[b] = 0;
    }
    if (done[b]) { next_ids[b] = pad; continue; }
    const int tok = argmax[r], c = col[b];
    bool fin = c + 1 >= max_new[b] || c + 1 >= cap;
    for (int k = 0; k < n_eos; ++k) fin = fin || tok == st[INTS_EOS0 + k];
    if (c < cap) out[(size_t)b * cap + c] = tok;
    next_ids[b] = tok;
    const int p = len[b] + c;
    pos[b] = p < max_len - 1 ? p : max_len - 1;
    col[b] = c + 1;
    if (fin) { done[b] = 1; atomicAdd(&s_fin, 1); }
  }
  __syncthreads();
  if (tid == 0 && s_fin) st[SES_FINISHES] += s_fin;
}

// Token feedback of a DRAFTING session (rk_llama_session_open_draft): llama_session_advance_kernel's state machine over g1 = Kd + 1
// rows per slot.  Row (s, 0) fed the slot's last accepted token, row (s, j) the draft token d_j = rnext[s g1 + j] at the next
// positions; dlen[s] of the extra rows are live.  t_0 = argmax(row 0) is always accepted; t_j = argmax(row j) is accepted while
// d_j == t_{j-1} and no accepted token has ended the slot (an EOS id, its max_new-th token, cap).  Accepted tokens go to the slot's
// output columns and to its history hist[s][len + column] (the prompt in front: what draft_lookup_kernel searches); col advances by
// the number accepted.  nstep[s] counts the steps the slot's request was active in.  st as above, with SES_NGRAM_MIN / SES_NGRAM_MAX.
// admit != null: row r of argmax is the prefill's last row of slot admit[r]; the slot starts here, its prompt tokens[seq_off[r] ..]
// is copied to its history and t_0 is its column 0.  One workgroup; rnext / dlen are written by draft_lookup_kernel behind this.
__global__ __launch_bounds__(256) void llama_session_advance_draft_kernel(const int* __restrict__ argmax, int* st, int* len, int* col,
                                                                          int* max_new, int* done, int* out, int n_slots,
                                                                          const int* __restrict__ admit, int n_admit, int g1,
                                                                          const int* __restrict__ rnext, const int* __restrict__ dlen,
                                                                          int* hist, int* nstep, const int* __restrict__ tokens,
                                                                          const int* __restrict__ seq_off) {
  __shared__ int s_fin;
  const int tid = threadIdx.x, n_eos = st[SES_N_EOS], max_len = st[SES_MAX_LEN], cap = st[SES_CAP];
  if (tid == 0) s_fin = 0;
  if (admit) {                                             // the prompts into the histories, every thread
    for (int r = 0; r < n_admit; ++r) {
      const int b = admit[r], L = admit[n_admit + r], t0 = seq_off[r];
      if (b < 0 || b >= n_slots) continue;
      for (int t = tid; t < L && t < max_len; t += 256) hist[(size_t)b * max_len + t] = tokens[t0 + t];
    }
  }
  __syncthreads();
  const int rows = admit ? n_admit : n_slots;
  for (int r = tid; r < rows; r += 256) {
    int b = r;
    if (admit) {
      b = admit[r];
      if (b < 0 || b >= n_slots) continue;
      len[b] = admit[n_admit + r]; max_new[b] = admit[2 * n_admit + r]; col[b] = 0; done[b] = 0; nstep[b] = 0;
    }
    if (done[b]) continue;
    const int row0 = admit ? r : b * g1, dl = admit ? 0 : dlen[b], L = len[b], mn = max_new[b];
    int c = col[b], prev = 0;
    bool fin = false;
    for (int j = 0; j <= dl && j < g1 && !fin; ++j) {
      const int tok = argmax[row0 + j];
      if (j > 0 && rnext[b * g1 + j] != prev) break;       // the draft fed to row j was not the token row j - 1 chose
      if (c < cap) out[(size_t)b * cap + c] = tok;
      if (L + c < max_len) hist[(size_t)b * max_len + L + c] = tok;
      ++c;
      prev = tok;
      fin = c >= mn || c >= cap;
      for (int k = 0; k < n_eos; ++k) fin = fin || tok == st[INTS_EOS0 + k];
    }
    col[b] = c;
    if (!admit) nstep[b] += 1;
    if (fin) { done[b] = 1; atomicAdd(&s_fin, 1); }
  }
  __syncthreads();
  if (tid == 0 && s_fin) st[SES_FINISHES] += s_fin;
}

// The proposer of a drafting session, one workgroup per slot, behind llama_session_advance_draft_kernel: the next step's g1 rows of
// the slot.  Row 0 feeds the last accepted token h[n - 1] at position n - 1 (n = len + col, the history's length).  The drafts:
// for N from ngram_max down to ngram_min the LARGEST i with h[i, i + N) == h[n - N, n) and i + N < n (a max-reduction over the
// candidates: the same answer whatever the thread order) proposes h[i + N, min(i + N + Kd, n)) - prompt lookup (hf: generation/
// candidate_generator.py PromptLookupCandidateGenerator; vLLM's [ngram] mode).  tabn[s] >= 0 (rk_debug_session_drafts): the drafts
// come from the caller's table instead, d_j = tab[s][col + j - 1].  They are clipped so that no live row lies beyond position
// max_len - 1 or beyond the slot's remaining max_new / cap.  Row j <= dlen: id d_j, position n - 1 + j, live; the others are dead:
// pad, position 0, not live (no cache write, results ignored).  An idle or done slot: no drafts, row 0 feeds pad at the position
// it has (llama_session_advance_kernel's rule).
__global__ __launch_bounds__(256) void draft_lookup_kernel(const int* __restrict__ st, const int* __restrict__ len, const int* __restrict__ col,
                                                           const int* __restrict__ max_new, const int* __restrict__ done, int g1,
                                                           int* rnext, int* rpos, int* rlive, int* dlen, const int* __restrict__ hist,
                                                           const int* __restrict__ tab, const int* __restrict__ tabn) {
  __shared__ int s_best;
  const int s = blockIdx.x, tid = threadIdx.x, Kd = g1 - 1;
  const int pad = st[SES_PAD], max_len = st[SES_MAX_LEN], cap = st[SES_CAP], nmin = st[SES_NGRAM_MIN], nmax = st[SES_NGRAM_MAX];
  int* nx = rnext + (size_t)s * g1; int* ps = rpos + (size_t)s * g1; int* lv = rlive + (size_t)s * g1;
  if (done[s]) {                                           // uniform
    if (tid == 0) { nx[0] = pad; lv[0] = 1; dlen[s] = 0; }
    if (tid >= 1 && tid < g1) { nx[tid] = pad; ps[tid] = 0; lv[tid] = 0; }
    return;
  }
  const int c = col[s], n = len[s] + c;
  const int* h = hist + (size_t)s * max_len;
  int lim = min(min(Kd, max_len - n), min(max_new[s], cap) - c - 1);
  lim = lim > 0 ? lim : 0;
  int dl = 0, src = 0;                                     // drafts d_j = from[src + j - 1]
  const int* from = h;
  if (tabn[s] >= 0) {
    from = tab + (size_t)s * cap; src = c;
    dl = min(lim, tabn[s] - c);
    dl = dl > 0 ? dl : 0;
  } else if (lim > 0) {
    for (int N = nmax; N >= nmin; --N) {
      if (N > n - 1) continue;                             // uniform
      if (tid == 0) s_best = -1;
      __syncthreads();
      int best = -1;
      for (int i = tid; i + N < n; i += 256) {
        bool eq = true;
        for (int k = 0; k < N; ++k) eq = eq && h[i + k] == h[n - N + k];
        if (eq) best = i;
      }
      if (best >= 0) atomicMax(&s_best, best);
      __syncthreads();
      best = s_best;
      __syncthreads();
      if (best >= 0) { src = best + N; dl = min(lim, n - src); break; }   // uniform
    }
  }
  if (tid == 0) { nx[0] = h[n - 1]; ps[0] = n - 1 < max_len - 1 ? n - 1 : max_len - 1; lv[0] = 1; dlen[s] = dl; }
  if (tid >= 1 && tid < g1) {
    const bool on = tid <= dl;
    nx[tid] = on ? from[src + tid - 1] : pad; ps[tid] = on ? n - 1 + tid : 0; lv[tid] = on ? 1 : 0;
  }
}

// QLM score (ref: llmrankers/pointwise.py:77-79) from the fused head (gemm.h: EPI_LSE_F32): stats [rows, nblk] = (block max, sum exp(x - block max)), xlab [rows] =
// the label's logit.  out[b] = -sum_t ( logsumexp_t - xlab[b, t] ), logsumexp_t = M + log(sum_blocks s * exp(m - M)).
// One block per sequence; the blocks of a position are merged in a fixed order, the positions summed in order (deterministic).
// row_off (rk_t5_qlm_many): the rows of sequence b are row_off[b] .. row_off[b + 1] - 1 instead of n_pos per sequence; out_idx:
// its score goes to out[out_idx[b]] (the caller's order of sequences that were sorted for the pass).
__global__ __launch_bounds__(256) void qlm_lse_kernel(const float2* __restrict__ stats, int nblk, const float* __restrict__ xlab,
                                                      int n_pos, const int* __restrict__ row_off, const int* __restrict__ out_idx,
                                                      float* __restrict__ out) {
  __shared__ float sred[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t row0 = row_off ? (size_t)row_off[b] : (size_t)b * n_pos;
  if (row_off) n_pos = row_off[b + 1] - row_off[b];
  float total = 0.f;
  for (int t = 0; t < n_pos; ++t) {
    const size_t row = row0 + t;
    const float2* src = stats + row * nblk;
    float mx = -INFINITY;
    for (int c = tid; c < nblk; c += 256) mx = fmaxf(mx, src[c].x);
    mx = wave_max(mx);
    if (lane == 0) sred[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
    __syncthreads();
    float se = 0.f;
    for (int c = tid; c < nblk; c += 256) { const float2 v = src[c]; se += v.y * expf(v.x - mx); }
    se = wave_sum(se);
    if (lane == 0) sred[wave] = se;
    __syncthreads();
    se = sred[0] + sred[1] + sred[2] + sred[3];
    __syncthreads();
    total += (mx + logf(se)) - xlab[row];
  }
  if (tid == 0) out[out_idx ? out_idx[b] : b] = -total;
}
