// The device int block of the Llama decoders: ONE owner of its format.  rk_llama_generate's block and a decoding session's block
// are a head of INTS_HEAD words (the state words below, the EOS ids from INTS_EOS0 on) and the arrays behind it.  The advance
// kernels (misc_kernels.h) read the head words by these names; the host takes every offset, the total and the block's initial
// contents from the layouts.  Plain C++17, no HIP: a CPU program includes this header too (tests/test_decode_ints_host.py).
#pragma once
#include <cstddef>
#include <vector>

enum { INTS_EOS0 = 8, INTS_HEAD = 16, INTS_MAX_EOS = INTS_HEAD - INTS_EOS0 };
// rk_llama_generate: the column to write, the step at which the last row finished (0: none yet), ...
enum GenWord { GEN_N, GEN_FINISHED, GEN_PAD, GEN_N_EOS, GEN_MAX_NEW, GEN_MAX_TOTAL, GEN_P };
// a session: the running number of finishes (the session word), ...; the n-gram lengths of a drafting session's lookup
enum SesWord { SES_FINISHES, SES_PAD, SES_N_EOS, SES_MAX_LEN, SES_CAP, SES_NGRAM_MIN, SES_NGRAM_MAX };

struct IntSpan { size_t off = 0, n = 0; };                 // an array's first int in the block and its length (n = 0: not there)

// rk_llama_generate's block: head | len[S] | done[S] | pos[S] | next[S] | out[n_seq][max_new]   (S = the engine's max_seqs)
struct GenInts { int *st, *len, *done, *pos, *next, *out; };
struct GenLayout {
  IntSpan len, done, pos, next, out;
  size_t total = INTS_HEAD;
  int n_seq, max_new;
  GenLayout(int S, int n_seq, int max_new) : n_seq(n_seq), max_new(max_new) {
    for (IntSpan* a : {&len, &done, &pos, &next, &out}) { *a = {total, a == &out ? (size_t)n_seq * max_new : (size_t)S}; total += a->n; }
  }
  GenInts bind(int* g) const { return GenInts{g, g + len.off, g + done.off, g + pos.off, g + next.off, g + out.off}; }
  // nothing has finished, column 0 is next; row b holds the seq_offsets[b] .. seq_offsets[b + 1] prompt tokens; the output is all pad
  std::vector<int> initial(const int* seq_offsets, int max_total, int P, const int* eos_ids, int n_eos, int pad) const {
    std::vector<int> v(total, 0);
    v[GEN_PAD] = pad; v[GEN_N_EOS] = n_eos; v[GEN_MAX_NEW] = max_new; v[GEN_MAX_TOTAL] = max_total; v[GEN_P] = P;
    for (int k = 0; k < n_eos; ++k) v[INTS_EOS0 + k] = eos_ids[k];
    for (int b = 0; b < n_seq; ++b) v[len.off + b] = seq_offsets[b + 1] - seq_offsets[b];
    for (size_t k = 0; k < out.n; ++k) v[out.off + k] = pad;
    return v;
  }
};

// a session's block: head | len[S] | col[S] | max_new[S] | done[S] | pos[S] | next[S] | admit[3 S] | out[S][cap], and with
// draft = Kd > 0 (R = S (Kd + 1) step rows): | rnext[R] | rpos[R] | rlive[R] | dlen[S] | nstep[S] | tabn[S] | tab[S][cap] | hist[S][max_len]
struct SessionInts { int *st, *len, *col, *max_new, *done, *pos, *next, *admit, *out, *rnext, *rpos, *rlive, *dlen, *nstep, *tabn, *tab, *hist; };
struct SessionLayout {
  IntSpan len, col, max_new, done, pos, next, admit, out, rnext, rpos, rlive, dlen, nstep, tabn, tab, hist;
  size_t total = INTS_HEAD;
  int cap, max_len, g1;                                    // g1: step rows per slot
  SessionLayout(int n_slots, int cap, int max_len, int draft) : cap(cap), max_len(max_len), g1(draft + 1) {
    const size_t S = (size_t)n_slots;
    auto take = [&](IntSpan& a, size_t n) { a = {total, n}; total += n; };
    for (IntSpan* a : {&len, &col, &max_new, &done, &pos, &next}) take(*a, S);
    take(admit, 3 * S); take(out, S * cap);
    if (!draft) return;
    for (IntSpan* a : {&rnext, &rpos, &rlive}) take(*a, S * g1);
    for (IntSpan* a : {&dlen, &nstep, &tabn}) take(*a, S);
    take(tab, S * cap); take(hist, S * max_len);
  }
  SessionInts bind(int* g) const {
    auto at = [&](const IntSpan& a) { return a.n ? g + a.off : nullptr; };
    return SessionInts{g, at(len), at(col), at(max_new), at(done), at(pos), at(next), at(admit), at(out),
                       at(rnext), at(rpos), at(rlive), at(dlen), at(nstep), at(tabn), at(tab), at(hist)};
  }
  // every slot idle: done, position 0, pad as its next id and all over its output; a drafting session: every row feeds pad at
  // position 0, row 0 of a slot is live, no caller's table, pad all over the tables and the histories
  std::vector<int> initial(const int* eos_ids, int n_eos, int pad, int ngram_min, int ngram_max) const {
    std::vector<int> v(total, 0);
    auto fill = [&](const IntSpan& a, int x) { for (size_t k = 0; k < a.n; ++k) v[a.off + k] = x; };
    v[SES_PAD] = pad; v[SES_N_EOS] = n_eos; v[SES_MAX_LEN] = max_len; v[SES_CAP] = cap;
    for (int k = 0; k < n_eos; ++k) v[INTS_EOS0 + k] = eos_ids[k];
    fill(done, 1); fill(next, pad); fill(out, pad);
    if (rnext.n) {
      v[SES_NGRAM_MIN] = ngram_min; v[SES_NGRAM_MAX] = ngram_max;
      fill(rnext, pad); fill(tabn, -1); fill(tab, pad); fill(hist, pad);
      for (size_t r = 0; r < rlive.n; r += g1) v[rlive.off + r] = 1;
    }
    return v;
  }
};
