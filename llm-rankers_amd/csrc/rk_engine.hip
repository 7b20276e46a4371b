// librk_engine.so — host side of the MI355X reranking engine: C ABI (include/rk_engine.h), weight repacking,
// workspace management and the launch sequence of the T5 encoder-decoder forward.
//
// What it replaces in the reference: T5ForConditionalGeneration.from_pretrained + .forward + .generate as
// called from llmrankers/pointwise.py:20-24,73-75,117-119 and llmrankers/setwise.py:46-59,93-95,184.
// The arithmetic restated here lives in hf: transformers/models/t5/modeling_t5.py (cited per kernel).
//
// gfx950 only; no CPU fallback, no CUDA/HIP dual paths.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is dlopen'ed on first use (rk_comm_*), never linked

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/rk_engine.h"
#pragma GCC visibility push(hidden)   // (its inline functions are no exports of the library)
#include "decode_ints.h"
#include "kv_layout.h"
#pragma GCC visibility pop
#include "attention.h"
#include "attention_d128.h"
#include "decoder_kernels.h"
#include "gemm.h"
#include "gemm_fp8.h"
#include "gemv_rows.h"
#include "llama_kernels.h"
#include "llama_kernels_hd64.h"
#include "llama_kernels_qknorm.h"
#include "llama_kernels_kv8.h"
#include "misc_kernels.h"
#include "sampling_kernels.h"

namespace {

thread_local std::string g_create_error;

enum ProfClass {
  PC_ENC_GEMM_QKV = 0, PC_ENC_GEMM_O, PC_ENC_GEMM_FFN_IN, PC_ENC_GEMM_FFN_OUT, PC_ENC_ATTN, PC_GEMM_CROSS_KV,
  PC_NORM, PC_EMBED, PC_DEC_GEMM, PC_DEC_ATTN, PC_HEAD, PC_OTHER,
  PC_COUNT
};
const char* kProfNames[PC_COUNT] = {"enc_gemm_qkv", "enc_gemm_o", "enc_gemm_ffn_in", "enc_gemm_ffn_out", "enc_attn",
                                    "gemm_cross_kv", "norm", "embed", "dec_gemm", "dec_attn", "head", "other"};

struct HostTensor {
  std::vector<half_t> h;   // 2-D matrices (fp16, the reference's accelerator dtype)
  std::vector<float> f;    // 1-D norm weights and the relative-attention tables (kept fp32)
  std::vector<int64_t> shape;
};

struct EncLayerW {
  half_t *qkv = nullptr, *o = nullptr, *ffn_in = nullptr, *ffn_out = nullptr; float *ln0 = nullptr, *ln1 = nullptr;
  half_t *qkv_f = nullptr, *ffn_in_f = nullptr;   // the same with the RMSNorm weight folded into the columns (W[n][k] * ln[k])
};
struct DecLayerW {
  half_t *qkv = nullptr, *o = nullptr, *cq = nullptr, *co = nullptr, *ffn_in = nullptr, *ffn_out = nullptr;
  half_t* ckT = nullptr;    // cross-attention W_k regrouped per head and transposed: [H][d_model][64] (direct path)
  half_t* ov = nullptr;     // self-attention W_o W_v [d_model, d_model]: the whole sub-layer at L_d = 1
  float *ln0 = nullptr, *ln1 = nullptr, *ln2 = nullptr;
  half_t *qkv_f = nullptr, *ov_f = nullptr, *cq_f = nullptr, *ffn_in_f = nullptr;   // norm weight folded in (W[n][k] * ln[k]), as in the encoder
};

// Llama-family decoder layer (hf: modeling_llama.py:291-330): fused q|k|v and interleaved gate|up carry the RMSNorm weights
// qkv8 .. down8: the four matrices a second time as FP8 step weights (rk_llama_set_weight_fp8; the fp16 matrices then hold the dequantised values)
struct LlamaLayerW { half_t *qkv_f = nullptr, *o = nullptr, *gu_f = nullptr, *down = nullptr; float* qkv_bias = nullptr; float* qk_norm = nullptr;
                     GemmW8 qkv8{nullptr, nullptr, 0, 0}, o8{nullptr, nullptr, 0, 0}, gu8{nullptr, nullptr, 0, 0}, down8{nullptr, nullptr, 0, 0}; };   // qkv_bias: Qwen2 only (rk_llama_set_qkv_bias), fp32 [Q + 2 KV], NOT scaled by the norm weight; qk_norm: Qwen3 only (rk_llama_set_qk_norm), fp32 q | k head-norm weights [2 * 128]

struct ProfRec { hipEvent_t a, b; int cls; };

struct Gemm;

// The residual stream of ONE chain (encoder, T5 decoder, Llama prefill, Llama step) and the protocol of its RMSNorms.
// Folded (the default): the GEMMs that follow a norm read the un-normalised stream as fp16 (written by the producer of the
// stream: embedding / residual epilogue), their weights carry the norm weight, and their epilogue applies the row factor - the
// norm kernels (re-reading the fp32 stream) are gone.  Unfolded: rmsnorm writes xn in front of every consumer.
// The buffers live as long as their owner (Slot, rk_engine::LlamaStep); a chain works on a copy, whose state begin() resets.
struct NormStream {
  float* hidden = nullptr;                 // the fp32 stream [rows, d_model]
  half_t* xraw[2] = {nullptr, nullptr};    // its fp16 copy x RK_XRAW_SCALE.  Two that alternate where a producer reads the stream it
                                           // replaces (T5 decoder: a producer never writes the buffer a workgroup of the same launch
                                           // may still read); else one
  float* ssq[2] = {nullptr, nullptr};      // block sums of squares per row left by the producer, one buffer per xraw
  float* factors = nullptr;                // row factors: written by the embedding or by rowscale_kernel
  half_t* xn = nullptr;                    // unfolded: the normed copy (chains that never run unfolded have none)
  int rows = 0; bool fold = false;
  int cur = 0, nb = 0;                     // the current xraw / ssq; block sums per row of the last producer (its plan; 0: the
                                           // embedding wrote the row factors)
  void begin(rk_engine* e, hipStream_t st, const int* ids, int rows_, bool fold_);   // the embedding launch
  const half_t* x() const { return fold ? xraw[cur] : xn; }                          // what the GEMMs behind a norm read
  Gemm consumer(rk_engine* e, hipStream_t st, const float* ln, Gemm c, bool own_factors) const;
  int producer(rk_engine* e, hipStream_t st, Gemm c, bool stats = true);
};

// A device buffer that grows between calls (never inside a capture).  reserve: nothing if n elements fit; else everything in
// flight is awaited, the buffer is replaced (contents lost) and *gen - part of the key of every graph that captured the
// address - is bumped.  Freed with its owner.
template <class T>
struct Grown {
  T* p = nullptr; size_t cap = 0;
  Grown() = default;
  Grown(const Grown&) = delete;
  Grown& operator=(const Grown&) = delete;
  ~Grown() { if (p) hipFree(p); }
  int reserve(rk_engine* e, size_t n, int* gen = nullptr);
};

// The decoder-side index buffers of a slot and the ONLY host code that writes them.  Every T5 entry point leaves its ids, row
// maps and labels here, and a later call may skip an upload because of what an earlier one left: so what the device holds is
// recorded here, as a consequence of WHICH buffer a write went to, never by the caller.
//   put     content-compared: nothing happens (no synchronisation, no copy) if the buffer holds exactly these ints, else one
//           pinned asynchronous copy on st (buffers below IX_N_CACHED: a pinned staging slot each)
//   write   plain synchronous copies (the big or always-changing arrays) after ONE synchronisation of st; what put knew of
//           those buffers is forgotten
//   tree    rk_t5_greedy2's five arrays: written only if `sig` differs from the last tree's or anything was written since
// The Llama family has IX_LAST_ROWS and IX_OUT_IDS only: llama_prefill writes the former through write(), rk_llama_last_logits copies
// the latter on its stream itself (its one writer, nothing is ever skipped there).  rk_llama_qlm adds IX_ROW_MAP (the stream rows its
// labels are predicted from), IX_ROW_LABEL and IX_ROW_OFF, allocated at its first call (ensure_llama_qlm) and written through
// write() in front of the prefill.  rk_t5_generate's greedy_advance_kernel writes IX_DEC_IDS on the device, behind the write()
// that forgot its content.
enum DecBuf { IX_DEC_IDS, IX_OUT_IDS, IX_LAST_ROWS, IX_N_CACHED, IX_ROW_LABEL = IX_N_CACHED, IX_ROW_OFF, IX_OUT_IDX, IX_ROW_SEQ, IX_TREE_KEYS, IX_TREE_POS, IX_ROW_MAP, IX_COUNT };
struct DecIndex {
  struct Src { DecBuf b; const std::vector<int>& v; };
  int* d[IX_COUNT] = {nullptr};
  int* pin = nullptr;                                          // pinned staging: IX_N_CACHED slots of PIN_INTS
  static constexpr int PIN_INTS = 8192;
  int put(rk_engine* e, hipStream_t st, DecBuf b, const int* src, int n);
  int write(rk_engine* e, hipStream_t st, std::initializer_list<Src> srcs);
  int tree(rk_engine* e, hipStream_t st, std::vector<int>& sig, std::initializer_list<Src> srcs);
 private:
  std::vector<int> held[IX_N_CACHED], tree_sig;                // what put / tree left on the device (empty: unknown)
  unsigned long epoch = 0, tree_epoch = ~0ul;                  // epoch counts the writes that reached the device
};

}  // namespace

#define RK_SLOTS 2

// Everything that belongs to ONE batch in flight: own activation workspace and own pair of HIP streams.  Two slots
// let (a) the latency-bound decoder chain of one batch hide under the MFMA-bound encoder of the next and (b) the
// encoder kernels of both batches co-run, so workgroups of one fill the tile-quantisation tail of the other
// (1104 GEMM tiles on 512 resident slots is 3 rounds alone but 2.16 rounds of work).
//
// Who touches what (T5; a launch = one encoder chain on se, then one decoder pass or several on sd).  Everything on one stream is
// ordered by the stream; the table is about the other stream and the host.
//   buffer                               written by                                read by
//   stg_tokens[g], stg_seq_off[g]        host, stage_slot (generation g)           encoder chain of the launches staged in g
//   enc, qkv, ctx, ffh                   encoder chain, from its first kernel      encoder chain only
//   dec_seq_off                          encoder chain, copy behind the layers     decoder: cross-attention
//   enc_out                              encoder chain, final rmsnorm              decoder: query-side cross-attention
//   cross_kv                             encoder chain, last GEMM (if needed)      decoder: cross-attention over materialised K / V
//   idx.*                                decoder stream (DecIndex copies); the HOST     decoder, head
//                                        waits for that stream first whenever the ints change (below)
//   dec, dqkv .. dlast, x*, d_argmax, d_scores   decoder stream (kernels)          decoder, head, verdict, gathers
//   h_scores                             decoder stream (copy behind the head)     host, behind ev_dec
// So the decoder of the slot's PREVIOUS launch reads dec_seq_off, enc_out and cross_kv and nothing else an encoder writes: the next
// encoder chain waits for ev_dec in front of its dec_seq_off copy (run_encoder: wait_prev_decoder), never earlier - its layers run
// beside that decoder.  The staged arrays are read by encoder chains alone, so staging waits for an encoder (ev_enc of the
// generation it writes), never for a decoder.  A new entry point that lets a decoder read another encoder-written buffer adds a row
// here and moves that buffer's first write behind wait_prev_decoder.
// One host wait for a decoder remains, in the LAUNCH and not in the staging: DecIndex::put / write reuse one pinned staging slot per
// buffer and synchronise the decoder stream before they overwrite it.  put compares first, so a launch whose decoder ids, last rows
// and output ids equal the slot's previous launch (same n_seq, dec_len, ids: the steady state of a stream of full calls) never
// waits; one that differs blocks the host until the slot's earlier decoders are through (include/rk_engine.h says so).
struct Slot {
  hipStream_t se = nullptr, sd = nullptr;   // this slot's encoder chain (MFMA-bound) | decoder chain (latency-bound)
  NormStream enc;                                              // the encoder's residual stream (Llama: the prefill's)
  half_t *qkv = nullptr, *ctx = nullptr, *ffh = nullptr, *enc_out = nullptr;
  int* d_tokens = nullptr; int* d_seq_off = nullptr;           // Llama only: the staged batch (llama_prefill writes and reads it on one stream)
  int* dec_seq_off = nullptr;                                  // T5 only: the DECODER's copy of the sequence offsets (the table above)
  // T5: two generations of the staged batch.  stage_slot writes the one no enqueued launch reads: the other one once a launch has
  // taken the current (gen_launched), else the current again.  stage_no counts the stagings, off_of is the one dec_seq_off holds.
  int *stg_tokens[2] = {nullptr, nullptr}, *stg_seq_off[2] = {nullptr, nullptr};
  int gen = 0; bool gen_launched = false; unsigned stage_no = 0, off_of = 0;
  int n_seq = 0, T = 0, maxL = 0, minL = 0; bool staged = false; int last_floats = 0;   // what the slot's last score / compare call left in its score buffer
  half_t* cross_kv = nullptr;                                  // [n_dec][max_tokens][2I] encoder -> decoder hand-off
  DecIndex idx; int* d_argmax = nullptr;                       // decoder ids, row maps, labels (see DecIndex) | the greedy head's result
  NormStream dec;                                              // the decoder's (run_decoder); rk_t5_qlm's final norm writes dec.xn
  half_t *dqkv = nullptr, *dctx = nullptr, *dq = nullptr, *dffh = nullptr, *dlast = nullptr;
  float* dssq_few[2] = {nullptr, nullptr};   // dec.ssq for the few-row GEMV family (gemv_rows.h): one partial per producing workgroup
  half_t *xqk = nullptr, *xctx = nullptr;                      // direct cross-attention: [32][H*d] each
  float *xpart = nullptr, *xstat = nullptr; bool have_cross_kv = false;
  float* d_scores = nullptr; float* h_scores = nullptr;
  // ev_enc[g]: the last encoder chain that read generation g is done (hand-off to the decoder; staging g again waits for it);
  // enc_gen: the generation of the last chain enqueued (-1: none).  ev_dec: the slot's last launch is done.
  hipEvent_t ev_enc[2] = {nullptr, nullptr}, ev_dec = nullptr; int enc_gen = -1; bool dec_pending = false;
};

struct rk_engine {
  rk_model_desc d{};
  int dev = 0;
  std::string err;
  bool finalized = false;
  int inner = 0;
  std::map<std::string, HostTensor> host;
  std::vector<void*> allocs;
  // weights
  half_t *emb = nullptr, *lm_head = nullptr, *cross_kv_w = nullptr;
  std::vector<EncLayerW> enc;
  std::vector<DecLayerW> dec;
  float *enc_final_ln = nullptr, *dec_final_ln = nullptr, *lut_enc = nullptr, *lut_dec = nullptr;
  Grown<float> logits; int logits_gen = 0;                     // qlm head: per-block (max, sum exp) pairs [rows, vocab/32] + label logits [rows]; slot 0 only.
                                                               // Llama sampling head: the step's fp32 logits [rows, vocab] (logits_gen counts the moves)
  Grown<float> amax_val; Grown<int> amax_idx; int amax_gen = 0;   // greedy head: per-row block maxima / first columns
  // rk_t5_generate: self-attention K / V cache [n_dec_layers][n_seq][P][2 inner] (kv_gen counts the moves) and the per-call int
  // block on the device (state, prefix, finished rows, output, tree arrays); decode_loop: pinned read-back of the finished step
  Grown<half_t> kv_cache; int kv_gen = 0;
  Grown<int> gen_buf; int* gen_pin = nullptr; hipEvent_t ev_gen[2] = {nullptr, nullptr};
  size_t scores_cap = 0;
  Slot slots[RK_SLOTS];
  // options / measurement
  // Engine options (rk_engine_set_option; table kOptions below: key, range, meaning).  Every option selects between TESTED
  // implementations of the same arithmetic - the on-device cross-check of a default path (tests/test_gpu_kernels.py compares them
  // bit for bit or within the stated tolerance) - or is a measurement knob of tools/; none is an unfinished experiment.
  struct Options {
    int glds = 1, skinny = 0x3F, overlap = 1, gemm_variant = 0, attn_short = 5, xattn_direct = 1, attn_heads_per_wg = 0, attn_ko = 0,
        gemm_persistent = 1, fold_norm = 1, s64_stages = 0, dec_fold_norm = 1, greedy_spec = 160, consumer_stats = 1, xattn_mfma = 1,
        dec_ffn_tiled = 1, gemm_split = 1, dec_fuse = 1, dec_fuse_rows = 0, dec_attn_seq = 1, attn_long = 1, attn_long_nw = 0,
        llama_attn_dma = 1, attn_long_xcd = 1, llama_attn_nw = 0, dec_graph = 1, gemm_sk = 1, dec_cross_mfma = 1, dec_gemv = 1, dec_gemv_rows = 4,
        dec_cached_attn = 1, llama_dec_r = 0, enc_serial = 0, llama_step_fp8 = 1, llama_kv_fp8 = 1;
  } opt;
  float* attn_trace = nullptr;   // measurement builds only (option attn_trace)
  int n_cu = 256;
  // K-split ping-pong GEMM (gemm.h: SPLIT): partial-tile slabs and arrival tickets, one set per stream (launches on different
  // streams overlap)
  struct SkWs { hipStream_t st = nullptr; float* slabs = nullptr; int* cnt = nullptr; };
  SkWs sk_ws[2 * RK_SLOTS];
  hipEvent_t t0 = nullptr, t1 = nullptr, t_tmp = nullptr;
  bool prof_on = false;
  std::vector<ProfRec> prof_recs; size_t prof_used = 0;
  double prof_flops[PC_COUNT] = {0}, prof_bytes[PC_COUNT] = {0}; int64_t prof_n[PC_COUNT] = {0};
  // decoder-only family (rk_llama_*): family 1 reuses `d` for the shared fields (vocab, d_model = hidden, d_ff =
  // intermediate, eps, capacities) so that the helpers below serve both families
  int family = 0; rk_llama_desc ld{};
  float rope_factor = 0.f, rope_low = 1.f, rope_high = 4.f; int rope_orig = 0;   // rope type llama3 when rope_factor > 0
  bool qkv_bias = false;                                                          // Qwen2 family: q / k / v projections carry a bias
  bool qk_norm = false;                                                           // Qwen3 family: RMSNorm over head_dim on every q and k head (rk_llama_set_qk_norm)
  bool weight_fp8 = false;                                                        // rk_llama_set_weight_fp8: the step's four projections also kept as FP8 step weights
  bool kv_fp8 = false;                                                            // rk_llama_set_kv_fp8: the decoding step's K / V cache in FP8 (llama_kernels_kv8.h)
  int window = 0;                                                                 // Mistral family: sliding window W (rk_llama_set_sliding_window), 0 = none
  std::vector<LlamaLayerW> ll; float *l_final_ln = nullptr, *rope_cos = nullptr, *rope_sin = nullptr; int* d_pos = nullptr;
  // rk_llama_set_sampling: temperature 0 = off (every entry point is greedy); d_seeds: one Philox key per row / session slot
  // (max_seqs of them, allocated once: no graph ever sees it move)
  struct Sampling { float T = 0.f; int k = 0; float p = 1.f; bool on() const { return T > 0.f; } } samp;
  unsigned long long* d_seeds = nullptr;
  // rk_llama_generate: K / V cache [n_layers][2][n_seq][n_kv][P][head_dim], the attention partials and the call's int block (grown
  // between calls; lkv_gen counts the moves and is part of the step graph's key), and the step's activation rows (max_seqs each).
  // An FP8-cache engine (kv_fp8) keeps bytes and exponents in lkv instead, as raw bytes: llama_kv_layer.
  Grown<half_t> lkv; Grown<float> lpart; Grown<int> lints; int lkv_gen = 0;
  struct LlamaStep { NormStream stream; half_t *qkv = nullptr, *ctx = nullptr, *ffh = nullptr; } lg;
  Grown<half_t> lqlm_x;                                                           // rk_llama_qlm: the final-normed label-predicting rows [rows][hidden]
  // rk_llama_session_*: the one open decoding session.  It lives in lkv / lpart / lints (rk_llama_generate is refused meanwhile)
  // and mirrors on the host what the device's int block said at the last read-back: no step is ever in flight between two calls.
  struct LlamaSession {
    bool open = false; int n_slots = 0, max_len = 0, cap = 0, seen = 0;   // seen: the session word at the last read-back
    std::vector<int> busy, told, len, max_new, col, done;                 // per slot; told: its finish was returned by a run
    bool sampled = false; std::vector<unsigned long long> seeds;          // latched at open: the sampling head; every slot's seed
    int draft = 0, ngram_min = 1, ngram_max = 3;                          // rk_llama_session_open_draft: Kd extra rows per slot (0: none)
    long long steps = 0, tokens = 0;                                      // rk_llama_session_stats: steps issued, tokens they emitted
    SessionLayout lay{0, 0, 0, 0};                                        // its int block in lints (decode_ints.h), set at the open
  } ls;
  // decoder chains as HIP graphs: key = everything the launch parameters of a chain depend on; at most RK_GRAPH_CACHE_KEYS keys
  // (run_graphed); graph_count: what run_graphed did since the engine was created (rk_debug_graph_stats)
  struct GraphEntry { int seen = 0; bool failed = false; hipGraphExec_t exec = nullptr; };
  std::map<std::vector<int>, GraphEntry> graphs; int opt_epoch = 0;
  struct GraphCount { int64_t eager = 0, captures = 0, replays = 0, failed = 0, evictions = 0; } graph_count;
  // score collection across GPUs (K9): one RCCL communicator per engine = per process = per GPU
  ncclComm_t comm = nullptr; int comm_rank = 0, comm_world = 1;
  float* d_gather[RK_SLOTS] = {nullptr}; float* h_gather[RK_SLOTS] = {nullptr}; size_t gather_cap = 0;
  hipEvent_t ev_gather[RK_SLOTS] = {nullptr}; bool gather_pending[RK_SLOTS] = {false}; int gather_n[RK_SLOTS] = {0};
  // appended form (a rank's share scored in several engine calls): send buffer [gather_cap], result [world][gather_cap]
  float *d_gsend = nullptr, *d_gall = nullptr, *h_gall = nullptr, *h_gstage = nullptr;
  hipEvent_t ev_gall = nullptr, ev_append = nullptr; bool gall_pending = false, append_foreign = false; int gall_n = 0;
};

namespace {

int fail(rk_engine* e, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e) e->err = buf; else g_create_error = buf;
  return code;
}

#define HIPCHK(E, call)                                                                              \
  do {                                                                                               \
    hipError_t _s = (call);                                                                          \
    if (_s != hipSuccess) return fail((E), RK_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_s)); \
  } while (0)
#define RC(x) do { rc = (x); if (rc) return rc; } while (0)   // (needs an int rc in scope)

template <class T>
int dalloc(rk_engine* e, T** p, size_t n) {
  void* q = nullptr;
  HIPCHK(e, hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
  e->allocs.push_back(q);
  *p = (T*)q;
  return RK_OK;
}

template <class T>
int upload(rk_engine* e, T** p, const T* src, size_t n) {
  int rc = dalloc(e, p, n);
  if (rc) return rc;
  HIPCHK(e, hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return RK_OK;
}

// ---- profiling-aware launch bracket ---------------------------------------------------------------------
struct Bracket {
  rk_engine* e; hipStream_t st; int idx = -1;
  Bracket(rk_engine* e_, hipStream_t st_, int cls, double flops, double bytes) : e(e_), st(st_) {
    if (!e->prof_on) return;
    if (e->prof_used == e->prof_recs.size()) {
      ProfRec r{};
      if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
      e->prof_recs.push_back(r);
    }
    idx = (int)e->prof_used++;
    e->prof_recs[idx].cls = cls;
    e->prof_flops[cls] += flops; e->prof_bytes[cls] += bytes; e->prof_n[cls]++;
    hipEventRecord(e->prof_recs[idx].a, st);
  }
  ~Bracket() { if (idx >= 0) hipEventRecord(e->prof_recs[idx].b, st); }
};

// overlap = 0 puts every launch of every slot on ONE stream (serial timeline, used for per-kernel event timing)
// encoders alternate between TWO streams however many slots there are (more concurrent GEMM chains only thrash)
hipStream_t enc_stream(rk_engine* e, Slot& sl) { return e->opt.overlap ? e->slots[(&sl - e->slots) & 1].se : e->slots[0].se; }
hipStream_t dec_stream(rk_engine* e, Slot& sl) { return e->opt.overlap ? sl.sd : e->slots[0].se; }

// ---- kernel launch helpers ------------------------------------------------------------------------------
// Launches kernel K with `lds` bytes of dynamic LDS.  More than 64 KiB needs hipFuncSetAttribute (opt_in bytes; 0: none), which
// applies per DEVICE: done once per (kernel, device), whichever engine / thread launches it there first (engines on different GPUs
// may live in one process).
template <auto K, class Args>
void launch_lds(hipStream_t st, dim3 grid, dim3 block, int lds, int opt_in, const Args& a) {
  static std::atomic<uint64_t> done{0};
  if (opt_in > 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
      hipError_t rc = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, opt_in);
      if (rc != hipSuccess) fprintf(stderr, "[rk_engine] hipFuncSetAttribute(%d B LDS) failed: %s\n", opt_in, hipGetErrorString(rc));
      done.fetch_or(bit, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(K, grid, block, lds, st, a);
}

template <int EPI, int WM, int WN, int MI, int NI>
void launch_v2(hipStream_t st, const GemmArgs& a) {
  constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
  constexpr int smem_stages = 2 * (BM + BN) * 64 * 2, smem_epi = WM * WN * 32 * (NI * 32 * 4 + 16);
  constexpr int smem = smem_stages > smem_epi ? smem_stages : smem_epi;
  const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
  launch_lds<gemm_v2_kernel<EPI, WM, WN, MI, NI>>(st, dim3(tiles), dim3(WM * WN * 64), smem, smem, a);
}

#define KSPLIT_MAX_SLABS 256      // partial tiles (256 x 256 fp32 = 256 KiB each) per stream: 64 MiB

template <int EPI, int KO = 0, bool RS = false, bool SPLIT = false>
void launch_pp2(hipStream_t st, const GemmArgs& a, int max_wgs) {
  constexpr int smem = 2 * 4 * 128 * 64 * 2 + 32768;   // 8 half-tile buffers + 32 KiB epilogue staging = all 160 KiB
  const int tiles = ((a.M + 255) / 256) * ((a.N + 255) / 256) * (SPLIT ? a.ksplit : 1);
  // persistent: one workgroup per CU walks the tiles (max_wgs = CUs rounded down to a multiple of 8 keeps the tile -> XCD
  // association); max_wgs <= 0: one workgroup per tile
  // (measured, r03: trimming the grid to the fewest workgroups with the same number of rounds - 232 instead of 256 for the
  // 920 tiles of O / FFN-out, to leave 24 CUs to the decoder stream for the whole GEMM - changes nothing: 7350-7370 against
  // 7367-7376 passages/s; the decoder kernels are not waiting for CUs, they share the memory system.  Likewise starting the
  // workgroups that walk one tile less 12 / 20 / 28 us late, so that their read-modify-write epilogues fall into the others'
  // MFMA phases at no cost to the critical path: o 0.496 -> 0.484 ms per step in the serial profile, 7302-7340 against
  // 7338-7376 passages/s in the pipeline - the epilogue's cost is not a shared-HBM burst that de-phasing would spread)
  const int grid = max_wgs > 0 && tiles > max_wgs ? max_wgs : tiles;
  launch_lds<gemm_pp2_kernel<EPI, KO, RS, SPLIT>>(st, dim3(grid), dim3(512), smem, smem, a);
}

// Tile-shape choice.  variant: 0 = auto, 1 = 128x128 (v1, two workgroups per CU), 2 = 256x256, 3 = 256x192,
// 4 = 256x128 (v2 kernels, one workgroup per CU), 5 = 256x256 ping-pong (v3).  auto = cheapest under a measured model:
// time ~ rounds over the resident slots x the variant's time for one round of K = 1024 (us, MI355X, tools/gemm_bench.py
// at M = 736 .. 23552, profiles/r01c_gemm_bench.txt, r01e_gemm_pingpong.txt).  All variants sum K in the same order, so
// the choice never changes a result bit.  GEGLU pairs gate/up inside 64-row wave tiles: no 192-wide tile for it.
// K split of the ping-pong kernel (gemm.h: SPLIT): the fp32 epilogues, TWO ways - and by option only (gemm_sk = 2: the hand-off tests,
// measurement).  The default (gemm_sk = 1) never splits.  The split rounds differently from the unsplit sum, and the one rule that
// ever paid - at most half as many 256 x 256 tiles as the chip has CUs and K >= 6 144 (profiles/r06_gemm_ksplit.txt, M = 1 536,
// N = 4 096: K = 14 336 281.6 -> 212.0 us, K = 8 192 155.9 -> 123.6 us; three / four ways lose) - reads the TILE COUNT of the launch,
// i.e. how many tokens share the call: a sequence alone, in a call of 1 537 .. 4 096 tokens and in a larger one got different last
// bits of `down`, and behind a whole ping-pong round (plan_gemm: m_pp2) even by its place in the batch - while a sequence's logits,
// scores and tokens are promised not to depend on what shares its call (include/rk_engine.h), on T5 as on Llama.  First seen on t5-3b
// (FFN-out N = 1 024, K = 16 384: tests/test_gpu_t5_d128.py), then at the plan lines of the Llama prefill
// (tests/test_gpu_llama_plan_lines.py, which also sweeps this rule over the served widths); what it cost: profiles/llama_ksplit_rule.txt.
// A rule that splits again has to read (N, K, family, options, CU count) alone, AND every kernel a call of other size may take at
// that (N, K) - the 64x64 variant, the launches with more tiles - has to sum K in the split's order.  Needs the workspace of the
// launch's stream (plan_gemm).
int choose_ksplit(const rk_engine* e, int epi, int M, int N, int K) {
  if (e->opt.gemm_sk != 2 || !(epi == EPI_RESID_F32 || epi == EPI_STORE_F32) || K % 64) return 1;
  const long tiles = (long)((M + 255) / 256) * ((N + 255) / 256);
  return (K / 64 >= 4 && tiles * 2 <= KSPLIT_MAX_SLABS) ? 2 : 1;    // two ways wherever they fit
}

int choose_variant(const rk_engine* e, int epi, int M, int N, int K, bool fold_producer, double* cost_out) {
  *cost_out = 0;
  if (e->opt.gemm_variant) return (e->opt.gemm_variant == 3 && (EPI_IS_GATED(epi) || fold_producer)) ? 2 : e->opt.gemm_variant;
  struct V { int id, bm, bn, slots; double round_us; };
  static const V vs[5] = {{5, 256, 256, 256, 25.5}, {2, 256, 256, 256, 29.8}, {3, 256, 192, 256, 24.7}, {4, 256, 128, 256, 19.0}, {1, 128, 128, 512, 17.3}};
  // 64x64 tiles (variant 6) win only while the larger tiles leave most of the chip idle (tools/gemm_bench.py, r02: O / FFN-out
  // of one or two setwise prompts, M = 1450 / 2900: 12.7 / 15.0 us against 15.7 / 17.4 us on 128x128 tiles; from M = 5888 on,
  // or for the wide QKV / FFN-in outputs, they lose): at most 192 tiles of 128x128
  if ((long)((M + 127) / 128) * ((N + 127) / 128) <= 192 && K >= 64) { *cost_out = 15.0; return 6; }
  double best = 1e30; int bv = 1;
  for (const V& v : vs) {
    if (v.id == 3 && (EPI_IS_GATED(epi) || fold_producer)) continue;   // (the folded-norm producer needs 64-column wave tiles)
    if (v.id == 5 && K < 128) continue;
    const long tiles = (long)((M + v.bm - 1) / v.bm) * ((N + v.bn - 1) / v.bn);
    double cost = (double)((tiles + v.slots - 1) / v.slots) * v.round_us;
    if (cost < best - 1e-9) { best = cost; bv = v.id; }
  }
  *cost_out = best;
  return bv;
}

// Folded RMSNorm hooks of one GEMM launch (GemmArgs): consumer side = rowscale or ssq_in / nb_in, producer side = xraw + ssq.
#define RK_XRAW_SCALE 0.0625f   // the fp16 copy of the fp32 residual stream is stored x 2^-4: head-room for the outlier
                                // channels of real T5 checkpoints (fp16 max 65504 -> 1.0e6), exact (power of two)
struct GemmFold { const float* rowscale = nullptr; half_t* xraw = nullptr; float* ssq = nullptr; const float* ssq_in = nullptr; int nb_in = 0; };

// Kernel family.  It follows from the CALLER's regime, never from M: a row's result must not depend on how many other rows share
// the launch (the families sum K in different orders).  GEMV: the few-row decoder pass (gemv_rows.h; run_decoder decides from the
// pass's rows / positions), one wave per output column over all CUs.  STREAM: weight-streaming (gemm_skinny_kernel) - the decoder,
// per-head batches, the greedy head.  TILED: the MFMA tile kernels.
enum GemmFamily { GEMM_NONE = -1, GEMM_TILED, GEMM_STREAM, GEMM_GEMV };
constexpr bool gemv_has(int E) { return E == EPI_STORE_F16 || E == EPI_RESID_F32 || E == EPI_GEGLU_F16 || E == EPI_RELU_F16 || E == EPI_STORE_F32; }
constexpr bool stream_has(int E) { return E != EPI_LSE_F32; }
constexpr bool tiled_has(int E) { return E != EPI_ARGMAX_F32; }
constexpr bool fp8_has(int E) { return E == EPI_STORE_F16 || E == EPI_RESID_F32 || E == EPI_SWIGLU_F16; }   // gemm_skinny_fp8_kernel: what the step needs
// the rows and K the GEMV kernel takes: all rows staged in LDS, K in 16-byte pieces, at most GEMV_MAX_PIECES per lane
inline bool gemv_fits(int M, int K) { return M <= GEMV_MAX_ROWS && K % 8 == 0 && K <= 512 * GEMV_MAX_PIECES; }

// One GEMM call, C = epilogue(A [M, K] x W [N, K]^T): the fields every call has in the constructor, the rare ones by name.
struct Gemm {
  int cls, epi; const half_t* A; int lda; const half_t* W; int ldw; void* C; int ldc, M, N, K;
  int n_split = 0; long split_stride = 0;       // GemmArgs::n_split (the stacked cross-attention K / V projection)
  int batch = 1; long bsA = 0, bsW = 0, bsC = 0;  // per-head GEMMs: `batch` blockIdx.y batches, element strides between them
  GemmFamily family = GEMM_TILED;
  GemmFold fold;
  const int* lse_labels = nullptr; float* lse_xlab = nullptr;   // EPI_LSE_F32: the label of every row, where its logit goes
  int* amax_idx = nullptr;                        // EPI_ARGMAX_F32: the first column of every block maximum, laid out like C
  GemmW8 fp8{nullptr, nullptr, 0, 0};             // W a second time as FP8 step weights (gemm_fp8.h): the stream family reads these
  Gemm(int cls_, int epi_, const half_t* A_, int lda_, const half_t* W_, int ldw_, void* C_, int ldc_, int M_, int N_, int K_)
      : cls(cls_), epi(epi_), A(A_), lda(lda_), W(W_), ldw(ldw_), C(C_), ldc(ldc_), M(M_), N(N_), K(K_) {}
  Gemm& heads(int b, long sA, long sW, long sC) { batch = b; bsA = sA; bsW = sW; bsC = sC; return *this; }
  Gemm& split(int n, long stride) { n_split = n; split_stride = stride; return *this; }
  Gemm& on(GemmFamily f) { family = f; return *this; }
  Gemm& with(const GemmFold& f) { fold = f; return *this; }
  Gemm& lse(const int* labels, float* xlab) { lse_labels = labels; lse_xlab = xlab; return *this; }
  Gemm& argmax(int* idx) { amax_idx = idx; return *this; }
  Gemm& w8(const GemmW8& w) { fp8 = w; return *this; }
};

// Launch plan of one GEMM call: everything gemm() launches, decided here and nowhere else.
struct GemmPlan {
  GemmFamily family = GEMM_NONE;   // NONE: no kernel runs the call as described (gemm() fails)
  const char* why = "no kernel of the family has the epilogue";   // NONE: what the call breaks (gemm_contract)
  int nb = 0;        // partial sums of squares per row the launch writes to fold.ssq: the nb_in of the GEMMs that read them
  // TILED: rows [0, m_pp2) on the persistent ping-pong kernel in whole rounds over the CUs (K split ks_pp2), the rest on `variant`
  // (1 = 128x128, 2..4 = 256-row v2 tiles, 5 = ping-pong, 6 = 64x64 with `stages` LDS stages; K split `ksplit` on variant 5)
  int m_pp2 = 0, ks_pp2 = 1, variant = 0, ksplit = 1, stages = 0;
  int wgs = 0;       // ping-pong grid: persistent workgroups (<= 0: one per tile)
  bool w8 = false;   // STREAM: gemm_skinny_fp8_kernel on the call's FP8 bytes (Gemm::w8), same bits as the fp16 kernel on W
  int ko = 0;        // measurement builds: ping-pong knock-out mask (gemm_variant 80 + mask)
  const rk_engine::SkWs* ks_ws = nullptr;   // the stream's K-split workspace
  // rows on the persistent ping-pong kernel?  A folded-norm consumer there takes its row factors ready-made (rowscale_kernel in
  // front of it); every other kernel forms them from the producer's block sums itself.
  bool pp2() const { return family == GEMM_TILED && (m_pp2 > 0 || variant == 5); }
};

// The CONTRACT of the kernel families (DESIGN.md "GEMM contract and how it is tested"): what the kernels require of a call, read off
// their loads and stores - not what the engine's dimension checks happen to guarantee.  Returns nullptr when family `fam` runs the
// call as described, else the reason; plan_gemm refuses (GEMM_NONE -> gemm() fails with RK_ERR_STATE) whatever breaks it, nothing
// is launched.  tests/test_gpu_gemm_epilogues.py asserts both directions through rk_debug_gemm_ex.
//   all       lda, ldw multiples of 8 halfs and >= K, A / W 16-byte aligned (16-byte operand pieces); ldc >= the output width
//   TILED     K % 64 (whole K tiles).  gemm_epilogue_staged writes 16-byte pieces: fp16 outputs 8 columns (N % 8, ldc % 8, n_split
//             % 8; N = 8j + 4 would put four halfs past column N - into the next row, or past C), fp32 outputs 4.  The folded-norm
//             consumer exists for the fp16 epilogues only (the residual epilogues with prefetched old rows and the ping-pong kernel's
//             fp32 / LSE instantiations never read the row factors); n_split not with the residual, gated or LSE epilogues (their
//             old-row prefetch / block layout ignores it); producer statistics need 64-column wave tiles (never the 192-wide tile:
//             choose_variant) and no n_split.  One launch: batch > 1 always goes to the weight-streaming kernel.
//   STREAM    K % 16 (k16 steps), 4-column pieces (N % 4, ldc % 4) except argmax blocks; no n_split (plan_gemm sends such a call to
//             the tiles); batches share neither fold buffers nor the argmax index buffer (not offset per batch)
//             FP8 bytes (Gemm::w8): store / residual / SwiGLU epilogues, one batch, rows of the device order (ldq >= K rounded up
//             to 256, 16-byte aligned), exponent rows of whole dwords
//   GEMV      M <= 16, K % 8, K <= 3072 (gemv_fits), scalar stores: any N, any ldc
//   gated     N % 64 everywhere: gate / up rows interleaved in groups of 32, a 64-row weight tile = 32 output columns
const char* gemm_contract(const Gemm& c, GemmFamily fam) {
  const int epi = c.epi;
  const bool gated = EPI_IS_GATED(epi), f16 = epi == EPI_STORE_F16 || epi == EPI_RELU_F16 || gated;
  const bool blocks = epi == EPI_ARGMAX_F32 || epi == EPI_LSE_F32;
  const bool consumer = c.fold.rowscale || c.fold.ssq_in, producer = c.fold.xraw || c.fold.ssq;
  if (c.N <= 0 || c.K <= 0 || c.batch < 1 || c.n_split < 0) return "empty or negative shape";
  if (c.lda < c.K || c.ldw < c.K || c.lda % 8 || c.ldw % 8 || c.bsA % 8 || c.bsW % 8 || ((uintptr_t)c.A | (uintptr_t)c.W) % 16)
    return "A / W rows must be 16-byte aligned and at least K long";
  if (gated && c.N % 64) return "gated epilogues pair gate / up rows in groups of 32: N % 64";
  const int width = blocks ? (c.N + 31) / 32 : (c.n_split > 0 ? c.n_split : (gated ? c.N / 2 : c.N));
  if (c.ldc < width) return "ldc smaller than the output width";
  if (epi == EPI_LSE_F32 && !(c.lse_labels && c.lse_xlab)) return "LSE epilogue without row labels and label-logit buffer";
  if (epi == EPI_ARGMAX_F32 && !c.amax_idx) return "argmax epilogue without index buffer";
  if (producer && (epi != EPI_RESID_F32 || !c.fold.xraw || !c.fold.ssq || c.n_split || c.batch > 1))
    return "producer statistics: fp32 residual epilogue, one batch, no n_split, xraw and ssq together";
  if (c.fold.ssq_in && c.fold.nb_in <= 0) return "ssq_in without nb_in";
  if (consumer && c.batch > 1) return "folded-norm consumer: one batch";
  if (fam == GEMM_GEMV) return nullptr;              // (gemv_fits, batch and n_split: plan_gemm)
  const int piece = fam == GEMM_TILED && f16 ? 8 : 4;        // columns per store
  const size_t cbytes = f16 ? 2 : 4;
  if (!blocks) {
    if (c.N % piece || c.ldc % piece || c.n_split % piece || c.split_stride % piece || c.bsC % piece || (uintptr_t)c.C % (piece * cbytes))
      return fam == GEMM_TILED && f16 ? "tiled fp16 outputs are written in 8-column pieces: N, ldc, n_split % 8, C 16-byte aligned"
                                      : "outputs are written in 4-column pieces: N, ldc, n_split % 4, C aligned to a piece";
    if (c.n_split > 0 && c.N % c.n_split) return "n_split must divide N";
  }
  if (fam == GEMM_STREAM) {
    if (c.K % 16) return "weight-streaming kernel: K % 16";
    if (c.batch > 1 && epi == EPI_ARGMAX_F32) return "argmax blocks: one batch";
    if (c.fp8.q) {
      if (!fp8_has(epi) || c.batch > 1) return "FP8 step weights: store, residual and SwiGLU epilogues, one batch";
      if (!c.fp8.exps || c.fp8.ldq < fp8_ldq(c.K) || c.fp8.ldq % 16 || c.fp8.lde < fp8_lde(c.K) || c.fp8.lde % 4 ||
          (uintptr_t)c.fp8.q % 16 || (uintptr_t)c.fp8.exps % 4)
        return "FP8 step weights: byte rows of K rounded up to 256 (16-byte aligned), exponent rows of whole dwords";
      if ((double)c.N * c.fp8.ldq >= 4294967296.0) return "FP8 step weights: the kernel addresses the bytes with 32-bit offsets (N * ldq < 4 GiB)";
    }
    return nullptr;
  }
  if (c.batch > 1) return "tiled kernels: one batch (a batch with n_split has no kernel)";
  if (c.K % 64) return "tiled kernels: K % 64";
  if (consumer && !f16) return "tiled kernels: folded-norm consumer for the fp16 epilogues only";
  if (c.n_split > 0 && (epi == EPI_RESID_F32 || gated || blocks)) return "tiled kernels: n_split for plain stores only";
  return nullptr;
}

// Tiled family: the ping-pong kernel pays a full round for a partial one: the 100 passages of one query (M = 18 400: 72 row panels)
// are 288 tiles of the O / FFN-out projections = 1.1 rounds paid as 2, 864 of QKV = 3.4 as 4.  All tile variants produce the same
// bits (K order, epilogue statistics: tests), so the rows beyond the last whole round go to the cheapest fill-in variant as a second
// launch - same model as choose_variant.  The grouped bench launches (M = 58 880) keep one launch: their last round is 60-98 % full
// and the model says so.
// A function of the call, the options and the CU count; its one stream-dependent input is the K split, which needs a workspace
// of the launch's stream (rk_engine::sk_ws: the slot streams have one).
GemmPlan plan_gemm(const rk_engine* e, const Gemm& c, hipStream_t st) {
  GemmPlan p;
  const int epi = c.epi, M = c.M, N = c.N, K = c.K;
  if (c.family == GEMM_GEMV) {                   // marked few-row by the caller: this kernel or none
    if (!gemv_has(epi)) return p;
    if (!(gemv_fits(M, K) && c.batch == 1 && c.n_split == 0)) { p.why = "few-row GEMV: M <= 16, K % 8, K <= 3072, one batch, no n_split"; return p; }
    if ((p.why = gemm_contract(c, GEMM_GEMV)) == nullptr) {
      p.family = GEMM_GEMV;
      p.nb = gemv_grid(N, e->n_cu);              // producer: one partial sum of squares per workgroup
    }
    return p;
  }
  if ((c.family == GEMM_STREAM || c.batch > 1) && c.n_split == 0 && (((e->opt.skinny >> epi) & 1) || c.batch > 1 || epi == EPI_ARGMAX_F32)) {
    if (stream_has(epi) && (p.why = gemm_contract(c, GEMM_STREAM)) == nullptr) { p.family = GEMM_STREAM; p.nb = (N + 31) / 32; p.w8 = c.fp8.q != nullptr; }   // producer blocks of 32 columns
    return p;
  }
  if (!tiled_has(epi)) return p;
  if ((p.why = gemm_contract(c, GEMM_TILED)) != nullptr) return p;
  p.family = GEMM_TILED;
  p.nb = (N + 63) / 64;                          // producer blocks of 64 columns
  p.wgs = e->opt.gemm_persistent == 1 ? (e->n_cu & ~7) : (e->opt.gemm_persistent & ~7);
  for (const auto& w : e->sk_ws) if (!p.ks_ws && w.st == st && w.slabs) p.ks_ws = &w;
  auto ksplit = [&](int rows) { return e->opt.gemm_persistent == 1 && p.ks_ws ? choose_ksplit(e, epi, rows, N, K) : 1; };
  const bool fold_producer = c.fold.xraw != nullptr;
  double whole = 0;
  p.variant = choose_variant(e, epi, M, N, K, fold_producer, &whole);
  if (e->opt.gemm_split && !e->opt.gemm_variant && K >= 128 && e->opt.gemm_persistent == 1 &&
      (epi == EPI_STORE_F16 || epi == EPI_RESID_F32 || EPI_IS_GATED(epi) || epi == EPI_RELU_F16)) {   // (the heads index rows from 0)
    const int tiles_n = (N + 255) / 256, tiles_m = (M + 255) / 256;
    const long rounds = (long)tiles_m * tiles_n / p.wgs;
    const int panels = (int)(rounds * p.wgs / tiles_n);          // whole row panels inside the whole rounds
    if (rounds >= 1 && (long)tiles_m * tiles_n % p.wgs != 0 && panels >= 1 && panels < tiles_m) {
      const long used = (long)panels * tiles_n;
      double rest = 0;
      const int v_rest = choose_variant(e, epi, M - panels * 256, N, K, fold_producer, &rest);
      if ((double)((used + p.wgs - 1) / p.wgs) * 25.5 + rest + 1.5 < whole - 1e-9) {   // (+ 1.5: a kernel boundary)
        p.m_pp2 = panels * 256; p.ks_pp2 = ksplit(p.m_pp2); p.variant = v_rest;
      }
    }
  }
#ifdef RK_MEASURE
  if (epi == EPI_STORE_F16 && p.variant > 80 && p.variant <= 96 && K >= 128) { p.ko = p.variant - 80; p.variant = 5; return p; }
#endif
  if (p.variant > 6) p.variant = 5;
  if (p.variant == 5 && K < 128) p.variant = 2;                   // the ping-pong kernel needs two K tiles
  if (p.variant == 5) p.ksplit = ksplit(M - p.m_pp2);
  if (p.variant == 6) {
    // stages: as many as keep every tile resident at once (4 -> 2 workgroups per CU, 3 -> 3, 2 -> 4)
    const int tiles = ((M - p.m_pp2 + 63) / 64) * ((N + 63) / 64);
    p.stages = e->opt.s64_stages;
    if (p.stages < 2 || p.stages > 4) p.stages = tiles <= 2 * e->n_cu ? 4 : (tiles <= 3 * e->n_cu ? 3 : 2);
  }
  if (p.pp2()) {
    // the ping-pong kernel addresses its panels with 32-bit byte offsets and takes ready-made row factors only
    if ((double)M * c.lda * 2 >= 4294967296.0 || (double)N * c.ldw * 2 >= 4294967296.0) { p.family = GEMM_NONE; p.why = "ping-pong kernel: an operand panel beyond 4 GiB"; }
    else if (c.fold.ssq_in && !c.fold.rowscale) { p.family = GEMM_NONE; p.why = "ping-pong kernel: row factors ready-made (rowscale), not ssq_in"; }
  }
  return p;
}

template <int EPI, int NST>
void launch_s64(hipStream_t st, const GemmArgs& a) {
  constexpr int smem = NST * 16384;
  launch_lds<gemm_s64_kernel<EPI, NST>>(st, dim3(((a.M + 63) / 64) * ((a.N + 63) / 64)), dim3(128), smem, smem, a);
}

// one ping-pong launch of the plan with K split ks
template <int EPI>
void launch_pp2_plan(hipStream_t st, GemmArgs a, const GemmPlan& p, int ks) {
#ifdef RK_MEASURE
  if constexpr (EPI == EPI_STORE_F16) {                              // timing-only knock-outs
    switch (p.ko) {
      case 0: break;
      case 8: launch_pp2<EPI, 8>(st, a, p.wgs); return;              // no W-panel DMA
      case 16: launch_pp2<EPI, 16>(st, a, p.wgs); return;            // no A-panel DMA
      case 1: launch_pp2<EPI, 1>(st, a, p.wgs); return;
      case 2: launch_pp2<EPI, 2>(st, a, p.wgs); return;
      case 3: launch_pp2<EPI, 3>(st, a, p.wgs); return;
      case 4: launch_pp2<EPI, 4>(st, a, p.wgs); return;
      case 5: launch_pp2<EPI, 5>(st, a, p.wgs); return;
      default: launch_pp2<EPI, 6>(st, a, p.wgs); return;
    }
  }
#endif
  if constexpr (EPI == EPI_STORE_F16 || EPI_IS_GATED(EPI) || EPI == EPI_RELU_F16) {
    if (a.rowscale) { launch_pp2<EPI, 0, true>(st, a, p.wgs); return; }   // consumer side of the folded RMSNorm
  }
  if constexpr (EPI == EPI_RESID_F32 || EPI == EPI_STORE_F32) {
    if (ks > 1) { a.ksplit = ks; a.ks_slabs = p.ks_ws->slabs; a.ks_cnt = p.ks_ws->cnt; launch_pp2<EPI, 0, false, true>(st, a, p.wgs); return; }
  }
  launch_pp2<EPI>(st, a, p.wgs);
}

template <int EPI>
void launch_tiled(const rk_engine* e, hipStream_t st, GemmArgs a, const GemmPlan& p) {
  if (p.m_pp2 > 0) {
    // whole rounds on the ping-pong kernel, then the remaining rows on the fill-in variant (row-offset arguments)
    GemmArgs head = a;
    head.M = p.m_pp2;
    launch_pp2_plan<EPI>(st, head, p, p.ks_pp2);
    const size_t r = (size_t)p.m_pp2;
    constexpr size_t celt = (EPI == EPI_RESID_F32 || EPI == EPI_STORE_F32) ? 4 : 2;
    a.A += r * a.lda;
    a.C = (char*)a.C + r * (size_t)a.ldc * celt;
    if (a.rowscale) a.rowscale += r;
    if (a.xraw) a.xraw += r * a.ldx;
    if (a.ssq) a.ssq += r * a.nb;
    if (a.ssq_in) a.ssq_in += r * a.nb_in;
    a.M -= p.m_pp2;
  }
  switch (p.variant) {
    case 6:
      if (p.stages == 4) launch_s64<EPI, 4>(st, a);
      else if (p.stages == 3) launch_s64<EPI, 3>(st, a);
      else launch_s64<EPI, 2>(st, a);
      return;
    case 5: launch_pp2_plan<EPI>(st, a, p, p.ksplit); return;
    case 2: launch_v2<EPI, 2, 4, 4, 2>(st, a); return;
    case 3: if constexpr (!EPI_IS_GATED(EPI)) { launch_v2<EPI, 4, 2, 2, 3>(st, a); return; } break;
    case 4: launch_v2<EPI, 4, 2, 2, 2>(st, a); return;
  }
  // (a 16-wave 256x256 form, launch_v2<EPI, 4, 4, 2, 2>, measured 3-9 % slower than the 8-wave one: not instantiated)
  const int tiles = ((a.M + GEMM_BM - 1) / GEMM_BM) * ((a.N + GEMM_BN - 1) / GEMM_BN);
  if (e->opt.glds)
    hipLaunchKernelGGL((gemm_f16_kernel<EPI, true>), dim3(tiles), dim3(256), GEMM_LDS_BYTES, st, a);
  else
    hipLaunchKernelGGL((gemm_f16_kernel<EPI, false>), dim3(tiles), dim3(256), GEMM_LDS_BYTES, st, a);
}

template <int EPI, int MR>
void launch_gemv(const rk_engine* e, hipStream_t st, const GemmArgs& a) {
  const int smem = MR * a.K * 2 + (GEMV_MAX_ROWS + 4 * GEMV_MAX_ROWS) * 4;
  launch_lds<gemv_rows_kernel<EPI, MR>>(st, dim3(gemv_grid(EPI_IS_GATED(EPI) ? a.N / 2 : a.N, e->n_cu)), dim3(256), smem, smem > 65536 ? 160 * 1024 : 0, a);
}

template <int EPI>
void launch_stream(hipStream_t st, const GemmArgs& a, int batch, const GemmW8* w8 = nullptr) {
  // (a form where one workgroup takes up to 8 row slabs - 8x fewer, fatter workgroups - was bit-identical but made
  // the step 6 % slower: what the decoder costs the concurrent encoder GEMMs is the serial LENGTH of its chain, every
  // kernel delaying some tile of the GEMM in flight, not its CU-time; so: many short workgroups)
  // (tried and dropped, round 3: a 1-D launch that runs all row slabs of a column block on ONE XCD, so that a weight row is
  // fetched into one L2 only - dec_gemm 0.337 vs 0.328 ms per step at 320 rows: the slabs are not bound by weight traffic)
  constexpr int NT = EPI_IS_GATED(EPI) ? 2 : 1;                    // gated: the gate and up blocks of 32 columns together
  if constexpr (fp8_has(EPI)) {
    if (w8) { hipLaunchKernelGGL((gemm_skinny_fp8_kernel<EPI, NT>), dim3((a.N + 32 * NT - 1) / (32 * NT), 1, (a.M + 31) / 32), dim3(SKINNY_THREADS), 0, st, a, *w8); return; }
  }
  hipLaunchKernelGGL((gemm_skinny_kernel<EPI, NT>), dim3((a.N + 32 * NT - 1) / (32 * NT), batch, (a.M + 31) / 32), dim3(SKINNY_THREADS), 0, st, a);
}

// f(std::integral_constant<int, epi>): the one map from the runtime epilogue kind (0 .. EPI_LSE_F32) to the kernel templates
template <int E = 0, class F>
void with_epi(int epi, F&& f) {
  if (epi == E) f(std::integral_constant<int, E>());
  else if constexpr (E < EPI_LSE_F32) with_epi<E + 1>(epi, f);
}

// f(std::integral_constant<int, head width>): the one map from a decoder-only engine's head width (64, else 128) to the
// width-templated decode kernels
template <class F>
void with_width(int hd, F&& f) {
  if (hd == 64) f(std::integral_constant<int, 64>());
  else f(std::integral_constant<int, 128>());
}
// f(std::integral_constant<int, V>) for the V of Vs that v equals: a runtime value of a closed set to a template argument; a value
// outside the set is a host bug
template <int... Vs, class F>
void with_int(int v, F&& f) {
  if (!((v == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...)) abort();
}

// Runs plan_gemm's plan of the call.  *nb (optional): the plan's statistics layout, for the GEMMs that read what this one produced.
int gemm(rk_engine* e, hipStream_t st, const Gemm& c, int* nb = nullptr) {
  if (c.M <= 0) return RK_OK;
  const GemmPlan p = plan_gemm(e, c, st);
  if (p.family == GEMM_NONE)
    return fail(e, RK_ERR_STATE, "no kernel of family %d takes the GEMM M=%d N=%d K=%d (epilogue %d, batch %d): %s", (int)c.family, c.M, c.N, c.K, c.epi, c.batch, p.why ? p.why : "");
  if (nb) *nb = p.nb;
  GemmArgs a{c.A, c.W, c.C, c.lda, c.ldw, c.ldc, c.M, c.N, c.K, c.n_split, c.split_stride, 1.f, c.bsA, c.bsW, c.bsC};
  a.rowscale = c.fold.rowscale; a.xraw = c.fold.xraw; a.ssq = c.fold.ssq; a.ldx = c.N; a.nb = p.nb; a.xs = RK_XRAW_SCALE;
  a.ssq_in = c.fold.ssq_in; a.nb_in = c.fold.nb_in; a.eps_in = e->d.eps;
  a.group_n = GEMM_GROUP_N;
  a.amax_idx = c.amax_idx; a.lse_labels = c.lse_labels; a.lse_xlab = c.lse_xlab;
  const double flops = 2.0 * c.M * (double)c.N * c.K * c.batch;
  const double out_elems = EPI_IS_GATED(c.epi) ? (double)c.M * c.N / 2 : (double)c.M * c.N;
  const double bytes = 2.0 * (double)c.M * c.K + (p.w8 ? 1.0 : 2.0) * (double)c.N * c.K +
                       out_elems * (c.epi == EPI_RESID_F32 ? 8.0 : (c.epi == EPI_STORE_F32 ? 4.0 : 2.0));
  Bracket br(e, st, c.cls, flops, bytes);
  with_epi(c.epi, [&](auto E) {
    constexpr int EPI = decltype(E)::value;
    if constexpr (gemv_has(EPI)) {
      if (p.family == GEMM_GEMV) {
        if (a.M <= 2) launch_gemv<EPI, 2>(e, st, a);            // rows staged per workgroup
        else if (a.M <= 4) launch_gemv<EPI, 4>(e, st, a);
        else if (a.M <= 8) launch_gemv<EPI, 8>(e, st, a);
        else launch_gemv<EPI, 16>(e, st, a);
        return;
      }
    }
    if constexpr (stream_has(EPI)) { if (p.family == GEMM_STREAM) { launch_stream<EPI>(st, a, c.batch, p.w8 ? &c.fp8 : nullptr); return; } }
    if constexpr (tiled_has(EPI)) { if (p.family == GEMM_TILED) launch_tiled<EPI>(e, st, a, p); }
  });
  return RK_OK;
}

// ---- launchers of the row kernels and the device state machines (misc_kernels.h, llama_kernels*.h) ----
// Each takes what its kernel takes and holds the grid rule and the choice of template parameter / width: the production call sites
// and rk_debug_rows both launch through these, so the debug entry has no launch code of its own.
int rmsnorm_nv(int d) { return d <= 1024 ? 4 : (d <= 2048 ? 8 : 16); }   // rmsnorm_kernel<NV> holds 256 NV columns: d <= 4096
dim3 grid_waves(int items) { return dim3((items + 3) / 4); }             // one wave per row or dot product, four to a workgroup
dim3 grid_rowscale(int rows) { return dim3((rows + 255) / 256); }        // one thread per row
dim3 grid_pairs(int n_seq) { return dim3(n_seq / 2); }                   // one workgroup per pair; an unpaired last sequence gets none
dim3 grid_kv_fill(int maxL, int n_seq) { return dim3(maxL, n_seq); }     // one workgroup per (position, sequence)
void launch_rmsnorm(hipStream_t st, const float* x, const float* w, half_t* out, const int* row_map, int rows, int d, float eps, float scale) {
  const dim3 g = grid_waves(rows), b(256);
  if (d <= 1024) hipLaunchKernelGGL(rmsnorm_kernel<4>, g, b, 0, st, x, w, out, row_map, rows, d, eps, scale);
  else if (d <= 2048) hipLaunchKernelGGL(rmsnorm_kernel<8>, g, b, 0, st, x, w, out, row_map, rows, d, eps, scale);
  else hipLaunchKernelGGL(rmsnorm_kernel<16>, g, b, 0, st, x, w, out, row_map, rows, d, eps, scale);
}
void launch_embed(hipStream_t st, const int* ids, const half_t* table, float* out, int rows, int d, int vocab, half_t* xraw, float* rowscale,
                  float xs, float eps) {
  hipLaunchKernelGGL(embed_gather_kernel, grid_waves(rows), dim3(256), 0, st, ids, table, out, rows, d, vocab, xraw, rowscale, xs, eps);
}
void launch_rowscale(hipStream_t st, const float* ssq, float* out, int rows, int nb, int d, float eps, float xs) {
  hipLaunchKernelGGL(rowscale_kernel, grid_rowscale(rows), dim3(256), 0, st, ssq, out, rows, nb, d, eps, xs);
}
void launch_head_rows(hipStream_t st, const half_t* x, const half_t* head, const int* out_ids, float* out, int n_seq, int n_out, int d) {
  hipLaunchKernelGGL(head_rows_kernel, grid_waves(n_seq * n_out), dim3(256), 0, st, x, head, out_ids, out, n_seq, n_out, d);
}
void launch_pair_verdict(hipStream_t st, const half_t* x, const half_t* head, int false_id, int true_id, float* out, int n_seq, int d) {
  hipLaunchKernelGGL(pair_verdict_kernel, grid_pairs(n_seq), dim3(256), 0, st, x, head, false_id, true_id, out, n_seq, d);
}
void launch_argmax_blocks(hipStream_t st, const float* bval, const int* bidx, int n_blocks, int* out, int rows) {
  hipLaunchKernelGGL(argmax_blocks_kernel, dim3(rows), dim3(256), 0, st, bval, bidx, n_blocks, out);
}
void launch_qlm_lse(hipStream_t st, const float2* stats, int nblk, const float* xlab, int n_pos, const int* row_off, const int* out_idx,
                    float* out, int n_seq) {
  hipLaunchKernelGGL(qlm_lse_kernel, dim3(n_seq), dim3(256), 0, st, stats, nblk, xlab, n_pos, row_off, out_idx, out);
}
// the prefill's rotation, in place on T rows of the fused QKV buffer: head width 64 or 128, with the Qwen2 bias (then the n_v
// value heads get theirs) or without (value heads untouched); qkn (Qwen3: the layer's q | k head-norm weights; width 128 and no
// bias, rk_engine_finalize sees to it): the entry with the norm, n_v = the kv head count there too
void launch_rope(hipStream_t st, int hd, half_t* qkv, const int* pos, const float* cos_t, const float* sin_t, int ld, int n_rot,
                 const float* bias, int n_v, int T, const float* qkn = nullptr, float qkn_eps = 0.f) {
  if (qkn) hipLaunchKernelGGL(rope128_qkn_kernel, dim3(T), dim3(256), 0, st, qkv, pos, cos_t, sin_t, ld, n_rot - n_v, n_v, qkn, qkn_eps);
  else if (hd == 64 && bias) hipLaunchKernelGGL(rope64_kernel<true>, dim3(T), dim3(256), 0, st, qkv, pos, cos_t, sin_t, ld, n_rot, bias, n_v);
  else if (hd == 64) hipLaunchKernelGGL(rope64_kernel<false>, dim3(T), dim3(256), 0, st, qkv, pos, cos_t, sin_t, ld, n_rot, (const float*)nullptr, 0);
  else if (bias) hipLaunchKernelGGL(rope128_kernel<true>, dim3(T), dim3(256), 0, st, qkv, pos, cos_t, sin_t, ld, n_rot, bias, n_v);
  else hipLaunchKernelGGL(rope128_kernel<false>, dim3(T), dim3(256), 0, st, qkv, pos, cos_t, sin_t, ld, n_rot, (const float*)nullptr, 0);
}
// layer `layer` of a K / V cache at `base`, n_layers layers of layout L back to back (kv_layout.h): the pointers the kernels take
Kv8Cache kv_cache_layer(const KvLayerLayout& L, void* base, int layer) {
  char* l0 = (char*)base + (size_t)layer * L.bytes;
  return Kv8Cache{(half_t*)(l0 + L.k), (half_t*)(l0 + L.v), L.pe ? (int8_t*)(l0 + L.ke) : nullptr, L.pe ? (int8_t*)(l0 + L.ve) : nullptr, L.pe};
}
// the prompt's rotated keys and its values into the cache: sequence b to cache row b, or to row slots[b] of n_slots
// cc: the layer's cache (kv_cache_layer).  kv8 (an FP8-cache engine): 1 = bytes and exponents into cc's four regions, 2 = the
// dequantised fp16 values into cc.kc / cc.vc; 0: the fp16 copy.  Which fills exist: both widths on an fp16 cache, 128 alone on an
// FP8 cache (dec_attn_exists' rule), each to rows or to slots.
void launch_kv_fill(hipStream_t st, int hd, const half_t* qkv, const int* seq_off, const int* slots, int n_slots, const Kv8Cache& cc,
                    int ld, int n_heads, int n_kv, int P, int maxL, int n_seq, int kv8 = 0) {
  const dim3 g = grid_kv_fill(maxL, n_seq), b(256);
  if (kv8 == 1 && (!cc.ke || !cc.ve || cc.pe < P)) abort();   // a byte fill without its exponent planes: a host bug
  with_width(hd, [&](auto W) {
    with_int<0, 1, 2>(kv8, [&](auto mode) {
      with_int<0, 1>(slots != nullptr, [&](auto to_slots) {
        constexpr int D = decltype(W)::value, KV8 = decltype(mode)::value;
        constexpr bool SLOTS = decltype(to_slots)::value != 0;
        const int ns = SLOTS ? n_slots : 0;
        if constexpr (KV8 != 0 && D != 128) abort();           // no such kernel
        else if constexpr (KV8 != 0) hipLaunchKernelGGL((kv8_cache_fill_kernel<SLOTS, KV8>), g, b, 0, st, qkv, seq_off, slots, ns, cc, ld, n_heads, n_kv, P);
        else hipLaunchKernelGGL((kv_cache_fill_kernel<D, SLOTS>), g, b, 0, st, qkv, seq_off, slots, ns, cc.kc, cc.vc, ld, n_heads, n_kv, P);
      });
    });
  });
}
// n vectors of 128 through the FP8 cache's quantiser (rk_debug_kv8_quant, rk_debug_kv8_step's cache conversion)
void launch_kv8_quant(hipStream_t st, const half_t* x, int n, uint8_t* q, int8_t* ex, half_t* deq) {
  hipLaunchKernelGGL(kv8_quant_rows_kernel, dim3((unsigned)(((size_t)n * 16 + 255) / 256)), dim3(256), 0, st, x, n, q, ex, deq);
}
void launch_greedy_advance(hipStream_t st, const int* argmax, int* state, const int* prefix, int* done, int* out, int* next_ids, int n_seq,
                           int dec_len, int max_new) {
  hipLaunchKernelGGL(greedy_advance_kernel, dim3(1), dim3(256), 0, st, argmax, state, prefix, done, out, next_ids, n_seq, dec_len, max_new);
}
// the decoders' state machines on their int blocks (decode_ints.h: one pointer struct per block).  SessionAdmit: the admit form of
// the session's two - row r of argmax is slot rec[r]'s (rec = slot[n] | len[n] | max_new[n]); the drafting form copies the prompts
// tokens[seq_off[r] ..] to the histories.  The default: a step.
struct SessionAdmit { const int* rec = nullptr; int n = 0; const int *tokens = nullptr, *seq_off = nullptr; };
void launch_llama_advance(hipStream_t st, const int* argmax, const GenInts& d, int n_seq) {
  hipLaunchKernelGGL(llama_advance_kernel, dim3(1), dim3(256), 0, st, argmax, d.st, d.len, d.done, d.pos, d.out, d.next, n_seq);
}
void launch_session_advance(hipStream_t st, const int* argmax, const SessionInts& d, int n_slots, const SessionAdmit& a = {}) {
  hipLaunchKernelGGL(llama_session_advance_kernel, dim3(1), dim3(256), 0, st, argmax, d.st, d.len, d.col, d.max_new, d.done, d.pos, d.out, d.next,
                     n_slots, a.rec, a.n);
}
void launch_session_advance_draft(hipStream_t st, const int* argmax, const SessionInts& d, int n_slots, int g1, const SessionAdmit& a = {}) {
  hipLaunchKernelGGL(llama_session_advance_draft_kernel, dim3(1), dim3(256), 0, st, argmax, d.st, d.len, d.col, d.max_new, d.done, d.out, n_slots,
                     a.rec, a.n, g1, d.rnext, d.dlen, d.hist, d.nstep, a.tokens, a.seq_off);
}
void launch_draft_lookup(hipStream_t st, const SessionInts& d, int n_slots, int g1) {
  hipLaunchKernelGGL(draft_lookup_kernel, dim3(n_slots), dim3(256), 0, st, d.st, d.len, d.col, d.max_new, d.done, g1, d.rnext, d.rpos, d.rlive,
                     d.dlen, d.hist, d.tab, d.tabn);
}

void rmsnorm(rk_engine* e, hipStream_t st, const float* x, const float* w, half_t* out, const int* row_map, int rows, float scale = 1.f) {
  if (rows <= 0) return;
  Bracket br(e, st, PC_NORM, 3.0 * rows * e->d.d_model, (double)rows * e->d.d_model * 6.0);
  launch_rmsnorm(st, x, w, out, row_map, rows, e->d.d_model, e->d.eps, scale);
}

void embed(rk_engine* e, hipStream_t st, const int* ids, float* out, int rows, half_t* xraw = nullptr, float* rowscale = nullptr) {
  if (rows <= 0) return;
  Bracket br(e, st, PC_EMBED, 0, (double)rows * e->d.d_model * 6.0);
  launch_embed(st, ids, e->emb, out, rows, e->d.d_model, e->d.vocab, xraw, rowscale, RK_XRAW_SCALE, e->d.eps);
}

// folded RMSNorm: block sums of squares (left by the residual GEMM epilogue) -> row factors
void rowscale(rk_engine* e, hipStream_t st, const float* ssq, float* out, int rows, int nb) {   // nb: block sums per row (the producer's plan)
  if (rows <= 0) return;
  Bracket br(e, st, PC_NORM, 0, (double)rows * (nb + 1) * 4.0);
  launch_rowscale(st, ssq, out, rows, nb, e->d.d_model, e->d.eps, RK_XRAW_SCALE);
}

void NormStream::begin(rk_engine* e, hipStream_t st, const int* ids, int rows_, bool fold_) {
  rows = rows_; fold = fold_; cur = 0; nb = 0;
  embed(e, st, ids, hidden, rows, fold ? xraw[0] : nullptr, fold ? factors : nullptr);
}

// The GEMM c behind the norm with weight ln (c reads x(); folded, its matrix carries ln).  Folded, it needs the row factors: the
// embedding wrote them (nb == 0), or they come from the last producer's block sums.  The persistent ping-pong GEMM takes them
// ready-made (loaded under its last MFMAs): rowscale_kernel runs in front of it.  Every other kernel can add the block sums itself
// in its epilogue (gemm_row_factors, same rk_row_factor -> same bits, one launch less where launches are what costs) and does
// where the chain allows it (own_factors - the whole of a site's policy); else rowscale_kernel again.
Gemm NormStream::consumer(rk_engine* e, hipStream_t st, const float* ln, Gemm c, bool own_factors) const {
  GemmFold f;
  if (!fold) rmsnorm(e, st, hidden, ln, xn, nullptr, rows);
  else if (nb && own_factors && !plan_gemm(e, c, st).pp2()) { f.ssq_in = ssq[cur]; f.nb_in = nb; }
  else { if (nb) rowscale(e, st, ssq[cur], factors, rows, nb); f.rowscale = factors; }
  return c.with(f);
}

// A residual GEMM (fp32 stream += c).  Folded and `stats` (all but the chain's last: the final norm reads the fp32 stream) it also
// leaves the next fp16 copy of the stream and its block sums: the GEMMs from here on read what this one writes.
int NormStream::producer(rk_engine* e, hipStream_t st, Gemm c, bool stats) {
  if (!(fold && stats)) return gemm(e, st, c);
  if (xraw[1]) cur ^= 1;
  c.fold.xraw = xraw[cur]; c.fold.ssq = ssq[cur];
  return gemm(e, st, c, &nb);
}

// ---- relative position bucket (hf: modeling_t5.py:216-262), float32 like torch ------------------------------
int rel_bucket(int rel, bool bidirectional, int num_buckets, int max_distance) {
  int ret = 0;
  if (bidirectional) {
    num_buckets /= 2;
    if (rel > 0) ret += num_buckets;
    rel = rel < 0 ? -rel : rel;
  } else {
    rel = rel < 0 ? -rel : 0;
  }
  const int max_exact = num_buckets / 2;
  if (rel < max_exact) return ret + rel;
  const float num = logf((float)rel / (float)max_exact);
  const float den = (float)std::log((double)max_distance / (double)max_exact);
  int large = max_exact + (int)(num / den * (float)(num_buckets - max_exact));
  if (large > num_buckets - 1) large = num_buckets - 1;
  return ret + large;
}

// ---- weight lookup -------------------------------------------------------------------------------------------
const HostTensor* need(rk_engine* e, const std::string& name, int64_t r, int64_t c, std::string* missing) {
  auto it = e->host.find(name);
  if (it == e->host.end()) { *missing += (missing->empty() ? "" : ", ") + name; return nullptr; }
  const HostTensor& t = it->second;
  const bool ok = (c < 0) ? (t.shape.size() == 1 && t.shape[0] == r) : (t.shape.size() == 2 && t.shape[0] == r && t.shape[1] == c);
  if (!ok) { *missing += (missing->empty() ? "" : ", ") + name + "(bad shape)"; return nullptr; }
  return &t;
}

int set_device(rk_engine* e) {
  HIPCHK(e, hipSetDevice(e->dev));
  return RK_OK;
}

int DecIndex::put(rk_engine* e, hipStream_t st, DecBuf b, const int* src, int n) {
  if (b >= IX_N_CACHED) return fail(e, RK_ERR_STATE, "index buffer %d has no pinned slot: write() it", (int)b);
  std::vector<int>& h = held[b];
  if ((int)h.size() == n && (n == 0 || memcmp(h.data(), src, n * sizeof(int)) == 0)) return RK_OK;
  HIPCHK(e, hipStreamSynchronize(st));   // the pinned slot may still be in flight
  ++epoch;
  h.clear();
  int* slot = pin + b * PIN_INTS;
  if (n > PIN_INTS) {                    // larger than a pinned slot: plain synchronous copy
    HIPCHK(e, hipMemcpy(d[b], src, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  } else {
    memcpy(slot, src, n * sizeof(int));
    HIPCHK(e, hipMemcpyAsync(d[b], slot, n * sizeof(int), hipMemcpyHostToDevice, st));
  }
  h.assign(src, src + n);
  return RK_OK;
}

int DecIndex::write(rk_engine* e, hipStream_t st, std::initializer_list<Src> srcs) {
  HIPCHK(e, hipStreamSynchronize(st));
  ++epoch;
  for (const Src& s : srcs) {
    if (s.b < IX_N_CACHED) held[s.b].clear();
    HIPCHK(e, hipMemcpy(d[s.b], s.v.data(), s.v.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  return RK_OK;
}

int DecIndex::tree(rk_engine* e, hipStream_t st, std::vector<int>& sig, std::initializer_list<Src> srcs) {
  if (tree_epoch == epoch && sig == tree_sig) return RK_OK;
  const int rc = write(e, st, srcs);
  if (rc) return rc;
  tree_sig.swap(sig);
  tree_epoch = epoch;
  return RK_OK;
}

// ---- forward passes -----------------------------------------------------------------------------------------
// Head width of the T5 kernels: 64, or 128 (t5-3b / t5-11b: monoT5-3B, duoT5-3B).  A 128-wide engine serves the ONE-POSITION calls
// only (rk_t5_score with dec_len 1, rk_t5_compare): the encoder through attn_enc128_kernel, the decoder through the W_o W_v product
// and the five-launch query-side cross-attention chain, whose per-head GEMMs carry the width.  Every other 64-wide kernel
// (decoder self-attention, the materialised K / V, the fused chain projections) is never launched there: refuse_wide.
// A Llama-family engine's is its head_dim (64 or 128: llama_kernels_hd64.h / llama_kernels.h serve every entry point at both); no T5
// path reads it there - every T5 entry point refuses a Llama engine first, and wide_heads, the T5 refusals' test, is T5 only.
inline int head_width(const rk_engine* e) { return e->family == 0 ? e->d.d_kv : e->ld.head_dim; }
inline bool wide_heads(const rk_engine* e) { return e->family == 0 && head_width(e) == 128; }
int refuse_wide(rk_engine* e, const char* entry, const char* what) {
  return fail(e, RK_ERR_STATE, "%s: d_kv=128 engines serve one decoder position only (rk_t5_score with dec_len 1, rk_t5_compare); %s", entry, what);
}
// a one-position call on a 128-wide engine: the options must select the paths that have a 128 form
int check_wide_one(rk_engine* e, const char* entry) {
  if (!wide_heads(e)) return RK_OK;
  if (!e->opt.xattn_direct) return refuse_wide(e, entry, "option xattn_direct = 0 selects the materialised K / V, which have no 128-wide kernel");
  if (e->opt.dec_fuse == 2) return refuse_wide(e, entry, "option dec_fuse = 2 forces the fused chain projections, which have no 128-wide kernel");
  return RK_OK;
}

#define XA_MAX_ROWS 512     // decoder rows (sequences x positions) per pass of the direct cross-attention path
#define XA_MAX_CHUNKS 4096  // rows x 64-key chunks of partial-sum workspace per pass
#define XA_MAX_LD 16        // decoder positions per sequence up to which the query-side form is used

// Everything a decoder pass decides from the POSITION COUNT of its sequences and that rounds differently on either side of
// the line: the ONE place these lines are drawn (run_decoder, use_xattn_direct and plan_dec_attn read them here).  Two
// position counts with the same key() take the same arithmetic row for row, so sequences of different label counts may share
// a ragged pass exactly when their keys agree (rk_t5_qlm_many); with the default options the classes are
// {1}, {2..4}, {5..16}, {17..64} and {65..max_dec_len}.
struct DecLenClass {
  bool one = false;          // a single position: the W_o W_v product form, fused cross-attention projections, tiled FFN-in
  bool stream = false;       // few positions: the weight-streaming GEMM family (and its folded norms), else the tiled one
  bool direct = false;       // query-side cross-attention, else the materialised K / V
  bool self_mfma = false, cross_mfma = false;   // attn_dec_cross_mfma_kernel for the self- / cross-attention, else the staged kernels
  int key() const { return (int)one | (int)stream << 1 | (int)direct << 2 | (int)self_mfma << 3 | (int)cross_mfma << 4; }
};
DecLenClass dec_len_class(const rk_engine* e, int Ld) {
  DecLenClass c;
  c.one = Ld == 1;
  c.stream = Ld <= 4;
  c.direct = e->opt.xattn_direct && Ld <= XA_MAX_LD;
  // the matrix-core kernel: cross-attention from two positions on; self-attention for long prefixes only (the materialised-K / V
  // regime, qlm: round 6); at most ATTX_MAXQ positions (two 32-query tiles)
  const bool mfma = e->opt.dec_cross_mfma && Ld <= ATTX_MAXQ;
  c.self_mfma = mfma && Ld > XA_MAX_LD;
  c.cross_mfma = mfma && Ld >= 2;
  return c;
}

// Query-side cross-attention (attention.h) or materialised K/V: the two round at different points, so the choice must
// not depend on what else shares the call (a row's logits have to be the same in any batch, on any rank): it is made
// from the decoder LENGTH of the call alone (the query-side form costs L_d x L x H x d flops per sequence against
// L x 2I x d for the projections: cheaper up to L_d ~ 64, and far fewer bytes below 16).  More rows than the workspace
// holds are taken in passes (run_decoder).
bool use_xattn_direct(const rk_engine* e, const Slot&, int max_ld) {
  return dec_len_class(e, max_ld).direct;
}

// ---- attention launch plans: like plan_gemm, each a function of the call shape, the options and the CU count (which kernels
// run, in order, their template parameter, grid, block, dynamic LDS, derived arguments); one launcher per plan runs it ----------
inline size_t attn_dec_lds(int keys) { return (64 + 256 + 8 + (size_t)keys) * sizeof(float); }   // attn_dec_kernel's dynamic LDS

// Encoder self-attention of one run_encoder call (hf: modeling_t5.py:144-173)
struct EncAttnPlan {
  enum Kind { DMA, LONG, TILED, D128 } kind = TILED;   // D128: attn_enc128_kernel (attention_d128.h), every call of a 128-wide engine
  int ng = 0, heads_per_wg = 0;       // DMA: attn_enc_dma_kernel<ng> (wave groups per workgroup), (sequence, head) items per group
  int nw = 0, nqb = 0, xcd_map = 0;   // LONG: attn_enc_long_kernel<nw> (waves per workgroup), query blocks of 32 nw, XCD grouping
  bool skip_long = false;             // LONG: attn_enc_kernel first, for the batch's sequences of at most ATT_ROW_MAXL keys
  dim3 grid, tiled_grid; int block = 0, lds = 0;   // DMA / long kernel; attn_enc_kernel's grid (256 threads, no dynamic LDS)
};
EncAttnPlan plan_enc_attn(const rk_engine* e, int n_seq, int maxL, int minL, int H) {
  const auto& o = e->opt;
  EncAttnPlan p;
  if (wide_heads(e)) {
    // 128-wide heads: ONE kernel for every length, whatever attn_short / attn_long say (they choose between 64-wide kernels).
    // One workgroup of four waves per 128 queries of a (sequence, head) pair: the pointwise batch (32 sequences x 184 tokens x 32
    // heads) is 2 048 workgroups, two resident per CU (LDS) - four rounds; a single duoT5 pair (2 x 512 tokens) 256: one per CU
    p.kind = EncAttnPlan::D128;
    p.nw = ATT128_NW;
    p.grid = dim3((maxL + 32 * p.nw - 1) / (32 * p.nw), H, n_seq); p.block = 64 * p.nw; p.lds = ATT128_LDS_BYTES;
    return p;
  }
  if (maxL <= ATT_ROW_MAXL && o.attn_short) {
    // Every sequence of the batch at most ATT_ROW_MAXL keys: the DMA kernel (attn_short = 5, the default: two six-wave groups
    // per 768-thread workgroup; 6: one group per workgroup).  The two compute a sequence bit-identically (attention.h: ATT_ROW_MAXL).
    // Persistent launch: at most one workgroup per CU, the (sequence, head) items dealt out evenly in contiguous runs per
    // wave group (320 sequences x 16 heads on 256 CUs x 2 groups: 10 items each)
    p.kind = EncAttnPlan::DMA; p.ng = o.attn_short == 6 ? 1 : 2;
    const long total = (long)n_seq * H, groups = (long)e->n_cu * p.ng;
    p.heads_per_wg = o.attn_heads_per_wg > 0 ? o.attn_heads_per_wg : (int)((total + groups - 1) / groups);
    p.grid = dim3((unsigned)((total + (long)p.ng * p.heads_per_wg - 1) / ((long)p.ng * p.heads_per_wg)));
    p.block = 384 * p.ng; p.lds = p.ng * ATTD_LDS_BYTES;
  } else if (o.attn_long) {
    // every sequence longer than ATT_ROW_MAXL keys: the chunked LDS-DMA kernel (round 5); the batch's short sequences (if any):
    // the tiled kernel, which reproduces the short kernel's bits - a sequence's result depends on ITS length only
    p.kind = EncAttnPlan::LONG; p.skip_long = minL <= ATT_ROW_MAXL; p.tiled_grid = dim3((ATT_ROW_MAXL + 127) / 128, H, n_seq);
    // waves per workgroup (same bits for every choice): option attn_long_nw, default 4
    // (measured, one to eight 1 560-token prompts: 4 waves = 128 queries per workgroup, two workgroups per CU, wins everywhere -
    // 36.9 / 49.1 / 157.5 us per layer at 1 / 2 / 8 prompts against 60 / 60 / 180 at twelve waves, 48 / 85 / 212 at six (384-thread
    // workgroups of this register size run one per CU) and 39.6 / 67.6 / 224.9 for the tiled kernel; profiles/r05_attn_long.jsonl)
    p.nw = (o.attn_long_nw == 12 || o.attn_long_nw == 6 || o.attn_long_nw == 3) ? o.attn_long_nw : 4;
    p.nqb = (maxL + 32 * p.nw - 1) / (32 * p.nw); p.grid = dim3(xcd_grid(n_seq * H, p.nqb)); p.block = 64 * p.nw; p.lds = ATTL_LDS_BYTES;
    p.xcd_map = o.attn_long_xcd;
  } else {   // option attn_long = 0: the tiled kernel for every length (the on-device cross-check of the two DMA kernels)
    p.tiled_grid = dim3((maxL + 127) / 128, H, n_seq);
  }
  return p;
}

// what the launcher reads of a call: run_encoder fills it from its slot and the model, rk_debug_attn from host operands
struct EncAttnCall { const half_t* qkv; half_t* ctx; const int* seq_off; const float* lut; int ld, ldctx, I, H, n_seq, maxL, T; };
void launch_enc_attn(rk_engine* e, hipStream_t st, const EncAttnCall& c, const EncAttnPlan& p) {
  const int I = c.I;
  if (p.kind == EncAttnPlan::D128) {
    const AttnEnc128Args a{c.qkv, c.ctx, c.seq_off, c.lut, c.ld, c.ldctx, I};
    Bracket br(e, st, PC_ENC_ATTN, 4.0 * (double)c.maxL * c.T * I, (double)c.T * 4 * I * 2.0);
    launch_lds<attn_enc128_kernel>(st, p.grid, p.block, p.lds, p.lds, a);
    return;
  }
  AttnEncArgs a{c.qkv, c.ctx, c.seq_off, c.lut, c.ld, c.ldctx, I, 1, e->opt.attn_ko};
#ifdef RK_MEASURE
  a.trace = e->attn_trace;
#endif
  Bracket br(e, st, PC_ENC_ATTN, 4.0 * (double)c.maxL * c.T * I, (double)c.T * 4 * I * 2.0);   // flops: exact for uniform lengths, upper bound if ragged
  if (p.kind == EncAttnPlan::TILED || p.skip_long) { a.skip_long = p.skip_long; hipLaunchKernelGGL(attn_enc_kernel, p.tiled_grid, dim3(256), 0, st, a); }
  if (p.kind == EncAttnPlan::DMA) {
    a.heads_per_wg = p.heads_per_wg; a.n_seq = c.n_seq;
    if (p.ng == 2) launch_lds<attn_enc_dma_kernel<2>>(st, p.grid, p.block, p.lds, p.lds, a);
    else launch_lds<attn_enc_dma_kernel<1>>(st, p.grid, p.block, p.lds, p.lds, a);
  } else if (p.kind == EncAttnPlan::LONG) {
    a.n_seq = c.n_seq; a.n_heads = c.H; a.nqb = p.nqb; a.xcd_map = p.xcd_map;
    if (p.nw == 12) launch_lds<attn_enc_long_kernel<12>>(st, p.grid, p.block, p.lds, p.lds, a);
    else if (p.nw == 6) launch_lds<attn_enc_long_kernel<6>>(st, p.grid, p.block, p.lds, p.lds, a);
    else if (p.nw == 4) launch_lds<attn_enc_long_kernel<4>>(st, p.grid, p.block, p.lds, p.lds, a);
    else launch_lds<attn_enc_long_kernel<3>>(st, p.grid, p.block, p.lds, p.lds, a);
  }
}

// Decoder attention of one run_decoder pass over decoder rows (self; tree: rk_t5_greedy2's shared prefixes) or over the
// materialised encoder K / V (cross): the matrix-core kernel, then a staged kernel for the sequences it leaves.  The call's
// position count decides whether the MFMA kernel runs at all, a sequence's own key count (<= ATTX_MAXK) whether it takes it.
struct DecAttnPlan {
  bool mfma = false;                            // attn_dec_cross_mfma_kernel, 128 threads, ATTX_LDS_BYTES
  enum Staged { NONE, SEQ, ROW } staged = ROW;  // then attn_dec_seq_kernel (one workgroup per (head, sequence): K / V staged
                                                // once) or attn_dec_kernel (same bits), 256 threads
  dim3 mfma_grid, grid; size_t lds = 0;         // grid and dynamic LDS of the staged kernel
};
// keys: per sequence, Ld (self) or the longest (cross); tree_rows > 0: the tree form.  Ragged rows (AttnDecArgs::row_off): Ld =
// the pass's longest sequence - grids and LDS are sized by it (work, not bits), the kernels take each sequence's own count
DecAttnPlan plan_dec_attn(const rk_engine* e, bool cross, int B, int Ld, int keys, int H, int tree_rows) {
  DecAttnPlan p;
  if (tree_rows) { p.grid = dim3(1, H, tree_rows); p.lds = attn_dec_lds(keys); return p; }
  const DecLenClass lc = dec_len_class(e, Ld);
  p.mfma = cross ? lc.cross_mfma : lc.self_mfma;
  p.mfma_grid = dim3(H, B);
  if (p.mfma && keys <= ATTX_MAXK) p.staged = DecAttnPlan::NONE;
  else if (e->opt.dec_attn_seq && Ld >= 2 && attn_dec_seq_lds(keys) <= 160 * 1024) { p.staged = DecAttnPlan::SEQ; p.grid = dim3(H, B); p.lds = attn_dec_seq_lds(keys); }
  else { p.grid = dim3(Ld, H, B); p.lds = attn_dec_lds(keys); }
  return p;
}

void launch_dec_attn(rk_engine* e, hipStream_t st, const DecAttnPlan& p, AttnDecArgs a, double flops, double bytes) {
  Bracket br(e, st, PC_DEC_ATTN, flops, bytes);
  if (p.mfma) { hipLaunchKernelGGL(attn_dec_cross_mfma_kernel, p.mfma_grid, dim3(128), ATTX_LDS_BYTES, st, a); a.skip_short = 1; }
  if (p.staged == DecAttnPlan::SEQ) hipLaunchKernelGGL(attn_dec_seq_kernel, p.grid, dim3(256), p.lds, st, a);
  else if (p.staged == DecAttnPlan::ROW) hipLaunchKernelGGL(attn_dec_kernel, p.grid, dim3(256), p.lds, st, a);
}

// Query-side cross-attention of one block of nr decoder rows (attention.h: XAttnArgs): qk = W_k^T q per head; scores, softmax and
// weighted sums over the raw encoder states in 64-key chunks; ctx = W_v (.) per head.  fuse (run_decoder): the projections around
// it fused per (head, row slab) - decoder_kernels.h: the q projection + W_k^T q in one launch, the chunk merge + W_v in another.
struct XAttnPlan {
  int nr = 0, nch = 0;                                      // rows, 64-key chunks of the longest sequence
  bool fuse_qk = false; int qk_R = 32, qk_CS = 1;           // dec_cross_qk_kernel (H, ceil(nr / R), CS); else the W_k^T GEMM per head
  enum Part { MFMA_FEW, MFMA, VALU16, VALU4 } part = MFMA;  // xattn_part_mfma_kernel<true / false>, xattn_part_kernel<16 / 4>
  dim3 part_grid;
  bool fuse_cv = false; int cv_R = 16;   // dec_cross_cv_kernel (H, ceil(nr / R)); else xattn_combine_kernel + the W_v GEMM per head
};
XAttnPlan plan_xattn(const rk_engine* e, bool fuse, int nr, int maxL, int H, int dm) {
  const auto& o = e->opt;
  XAttnPlan p;
  p.nr = nr; p.nch = (maxL + 63) / 64; p.fuse_qk = fuse;
  if (fuse) {
    if (o.dec_fuse_rows > 0) p.qk_R = std::min(32, o.dec_fuse_rows);
    else if (nr <= 16) p.qk_R = 16;   // (a setwise pass: 13 rows - half the MFMA columns, half the x rows; measured at 320 rows: 32 > 16 > 8)
    // few rows: several workgroups per (head, slab) share the output columns, each streaming 1 / CS of W_k^T (and all of W_q,h)
    while (p.qk_CS < 8 && (dm / 64) % (2 * p.qk_CS) == 0 && (long)((nr + p.qk_R - 1) / p.qk_R) * H * p.qk_CS < e->n_cu / 2) p.qk_CS *= 2;
  }
  // MFMA form (weighted sums on the matrix cores, the chunk's encoder rows staged in LDS by a loader wave) whenever the model
  // width allows its LDS image (every wave takes whole 64-column pieces of its quarter); the VALU form otherwise.  The choice
  // depends on the MODEL only, never on the batch (the two round differently).  Few workgroups (a setwise compare): the
  // latency-scheduled form, two pieces per wave (same bits; attention.h).
  const long wgs16 = (long)p.nch * nr * ((H + 15) / 16);
  if (o.xattn_mfma && dm % 256 == 0) p.part = wgs16 <= 2 * e->n_cu ? XAttnPlan::MFMA_FEW : XAttnPlan::MFMA;
  else p.part = wgs16 >= 2 * e->n_cu ? XAttnPlan::VALU16 : XAttnPlan::VALU4;
  p.part_grid = dim3(p.nch, nr, p.part == XAttnPlan::VALU4 ? (H + 3) / 4 : (H + 15) / 16);
  // fused merge: rows per workgroup: the largest slab that still gives about half the chip a workgroup (results do not depend on
  // it) (16 rows: 41 KiB of LDS at d = 1024, three workgroups per CU hide each other's load latency)
  p.fuse_cv = fuse && p.nch <= DECV_MAXCH;
  while (p.fuse_cv && p.cv_R > 2 && (long)((nr + p.cv_R - 1) / p.cv_R) * H < e->n_cu / 2) p.cv_R >>= 1;
  return p;
}

// The chunk kernel of the plan over xa's rows and, unless the merge is fused into the W_v product, xattn_combine_kernel (maxL, T:
// the longest sequence and the token count, for the profile only)
void launch_xattn_part(rk_engine* e, hipStream_t st, const XAttnPlan& p, const XAttnArgs& xa, int maxL, int T) {
  Bracket br(e, st, PC_DEC_ATTN, 4.0 * p.nr * (double)maxL * xa.H * xa.d, (double)T * xa.d * 2.0 * 2);
  if (p.part == XAttnPlan::MFMA_FEW) hipLaunchKernelGGL(xattn_part_mfma_kernel<true>, p.part_grid, dim3(256), 0, st, xa);
  else if (p.part == XAttnPlan::MFMA) hipLaunchKernelGGL(xattn_part_mfma_kernel<false>, p.part_grid, dim3(256), 0, st, xa);
  else if (p.part == XAttnPlan::VALU16) hipLaunchKernelGGL(xattn_part_kernel<16>, p.part_grid, dim3(256), 0, st, xa);
  else hipLaunchKernelGGL(xattn_part_kernel<4>, p.part_grid, dim3(256), 0, st, xa);
  if (!p.fuse_cv) hipLaunchKernelGGL(xattn_combine_kernel, dim3(xa.H, p.nr), dim3(256), 0, st, xa);
}

// W_k of one cross-attention layer ([H * hd, dm], HF layout; hd = the head width) regrouped per head and transposed, as
// dec_cross_qk_kernel (hd = 64 only) and the per-head W_k^T GEMM read it: ckT[h][c][j] = W_k[h * hd + j][c]
std::vector<half_t> regroup_ckT(const half_t* wk, int H, int dm, int hd) {
  std::vector<half_t> t((size_t)H * hd * dm);
  for (int h = 0; h < H; ++h)
    for (int c = 0; c < dm; ++c)
      for (int j = 0; j < hd; ++j) t[((size_t)h * dm + c) * hd + j] = wk[((size_t)h * hd + j) * dm + c];
  return t;
}

// The whole query-side cross-attention chain of one decoder layer over M rows: what run_xattn_chain reads of a call.  run_decoder
// fills it from its slot and layer, rk_debug_xattn_chain from host operands.
struct XAttnChain {
  const half_t* x; int ldx;                   // [M, ldx] input of the q projection (the norm folded: fold, or the normalised rows)
  const half_t *wq, *wkT, *wv;                // [H * hd, dm], [H][dm][hd] (regroup_ckT), [H * hd, dm]
  GemmFold fold;                              // the q projection's norm hooks: rowscale, or ssq_in / nb_in, or neither
  GemmFamily family;                          // kernel family of the q projection when it is a GEMM of its own
  const half_t* enc; const int* seq_off; const int* row_seq; int Ld, row0;   // encoder rows; decoder row row0 + m -> sequence (XAttnArgs)
  half_t* q;                                  // [M, H * hd] workspace: q of the unfused form
  half_t* qk; float* part; float* stat; half_t* xctx;   // workspaces of ONE block of rows (xattn_block_rows)
  half_t* ctx; int ldo;                       // [M, ldo] out: column h * hd + n
  int M, H, dm, maxL, T;                      // rows, heads, model width, the longest sequence, encoder tokens (profile only)
  bool fuse_asked;                            // the caller's regime asks for the fused projections (run_decoder)
  int hd = 64;                                // head width: 64, or 128 (only the three GEMMs of the unfused form see it)
};
// the fused form needs eight K ranges of whole k16 steps per workgroup, and its kernels are built for 64-wide heads; other model
// widths and 128-wide heads take the five-launch form
inline bool xattn_chain_fused(const XAttnChain& c) { return c.fuse_asked && c.dm % 128 == 0 && c.hd == 64; }
// rows per block: what the workspaces of one pass hold
inline int xattn_block_rows(int maxL) { return std::max(1, std::min(XA_MAX_ROWS, XA_MAX_CHUNKS / ((maxL + 63) / 64))); }
// the three GEMMs of the unfused form: q = W_q x over all rows, then per block qk_h = W_k,h^T q_h and ctx_h = W_v,h (.) per head
inline Gemm xattn_q_gemm(const XAttnChain& c) {
  return Gemm(PC_DEC_GEMM, EPI_STORE_F16, c.x, c.ldx, c.wq, c.dm, c.q, c.H * c.hd, c.M, c.H * c.hd, c.dm).on(c.family).with(c.fold);
}
inline Gemm xattn_qk_gemm(const XAttnChain& c, int r0, int nr, half_t* qk) {
  const int I = c.H * c.hd;
  return Gemm(PC_DEC_GEMM, EPI_STORE_F16, c.q + (size_t)r0 * I, I, c.wkT, c.hd, qk, c.H * c.dm, nr, c.dm, c.hd).heads(c.H, c.hd, (long)c.dm * c.hd, c.dm);
}
inline Gemm xattn_cv_gemm(const XAttnChain& c, int r0, int nr) {
  return Gemm(PC_DEC_GEMM, EPI_STORE_F16, c.xctx, c.H * c.dm, c.wv, c.dm, c.ctx + (size_t)r0 * c.ldo, c.ldo, nr, c.hd, c.dm).heads(c.H, c.dm, (long)c.hd * c.dm, c.hd);
}

// Rows [r0, r0 + p.nr) of the chain, their qk going to `qk` (the block's workspace).  Fused: c.x, c.wq and c.fold are the q projection's input, weight and norm; else c.q holds q.
int launch_xattn(rk_engine* e, hipStream_t st, const XAttnChain& c, const XAttnPlan& p, int r0, half_t* qk) {
  const int H = c.H, dm = c.dm, I = H * c.hd, nr = p.nr;
  int rc = RK_OK;
  if (p.fuse_qk) {
    DecQKArgs qa{c.x + (size_t)r0 * c.ldx, c.ldx, c.wq, c.wkT, qk, nr, dm, H, c.fold.rowscale ? c.fold.rowscale + r0 : nullptr,
                 c.fold.ssq_in ? c.fold.ssq_in + (size_t)r0 * c.fold.nb_in : nullptr, c.fold.nb_in, e->d.eps, RK_XRAW_SCALE, p.qk_R, p.qk_CS};
    Bracket br(e, st, PC_DEC_GEMM, 2.0 * nr * (double)dm * I * 2, 2.0 * ((double)I * dm * 2 + (double)nr * H * dm));
    hipLaunchKernelGGL(dec_cross_qk_kernel, dim3(H, (nr + p.qk_R - 1) / p.qk_R, p.qk_CS), dim3(64 * DEC_NW), 0, st, qa);
  } else {
    RC(gemm(e, st, xattn_qk_gemm(c, r0, nr, qk)));
  }
  launch_xattn_part(e, st, p, XAttnArgs{qk, c.enc, c.seq_off, c.part, c.stat, c.xctx, c.Ld, H, dm, p.nch, c.row0 + r0, c.row_seq}, c.maxL, c.T);
  if (!p.fuse_cv) return gemm(e, st, xattn_cv_gemm(c, r0, nr));
  DecCVArgs ca{c.part, c.stat, c.seq_off, c.row_seq, c.Ld, c.row0 + r0, c.wv, c.ctx + (size_t)r0 * c.ldo, nr, dm, H, p.nch, c.ldo, p.cv_R};
  Bracket br(e, st, PC_DEC_GEMM, 2.0 * nr * (double)dm * I, 2.0 * (double)I * dm + 4.0 * (double)nr * p.nch * H * dm);
  launch_lds<dec_cross_cv_kernel>(st, dim3(H, (nr + p.cv_R - 1) / p.cv_R), dim3(64 * DEC_NW), (int)dec_cv_lds_bytes(dm, p.cv_R), 160 * 1024, ca);
  return RK_OK;
}

// The chain over all M rows: the fuse decision, the q projection as a GEMM of its own when not fused, then blocks of rows that fit
// the workspaces, each planned by plan_xattn.  between (optional; the debug call): called in front of every block's launches and
// behind them with the block's first row and plan (front = true / false); in front it may give the block another qk workspace than
// c.qk through *qk (the debug call keeps every block's qk); the chain itself is never changed.  A non-zero return ends the chain
// with that status.
struct XAttnChainHook { int (*fn)(void* user, bool front, int r0, const XAttnPlan& p, half_t** qk); void* user; };
int run_xattn_chain(rk_engine* e, hipStream_t st, const XAttnChain& c, const XAttnChainHook* between = nullptr) {
  const bool fuse = xattn_chain_fused(c);
  int rc = RK_OK;
  if (!fuse) RC(gemm(e, st, xattn_q_gemm(c)));
  const int blk = xattn_block_rows(c.maxL);
  for (int r0 = 0; r0 < c.M; r0 += blk) {
    const XAttnPlan xp = plan_xattn(e, fuse, std::min(blk, c.M - r0), c.maxL, c.H, c.dm);
    half_t* qk = c.qk;
    if (between) RC(between->fn(between->user, true, r0, xp, &qk));
    RC(launch_xattn(e, st, c, xp, r0, qk));
    if (between) RC(between->fn(between->user, false, r0, xp, &qk));
  }
  return RK_OK;
}

// Causal attention of one llama_prefill call (hf: modeling_llama.py:130-214)
enum CausalAttnKind { CAUSAL_TILE, CAUSAL_DMA };
struct CausalAttnPlan {
  int kind = CAUSAL_TILE, hd = 128;        // attn_causal_tile_kernel<hd, .>, or attn_causal_dma_kernel<nw, .> (128 wide)
  int nw = 0, nqb = 0;                     // CAUSAL_DMA: waves per workgroup, query blocks of 32 nw
  int window = 0;                          // > 0: the kernel's windowed entry (WIN = 1)
  dim3 grid; int block = 256, lds = 0, lds_opt_in = 0;
};
// ---- which kernels the prefill attention has: THE one statement (the walk and the launch below follow it) ----
// the register-staged kernel at both widths, windowed at 64 only; the LDS-DMA kernel at 128, plain and windowed.  A caller whose
// plan is outside it (a window on a 128-wide engine with llama_attn_dma = 0) refuses the call: refuse_window.
constexpr bool causal_attn_exists(int kind, int D, bool win) {
  return kind == CAUSAL_TILE ? (D == 64 || (D == 128 && !win)) : (kind == CAUSAL_DMA && D == 128);
}
inline bool causal_attn_exists(const CausalAttnPlan& p) { return causal_attn_exists(p.kind, p.hd, p.window > 0); }
// The sliding window (rk_llama_set_sliding_window: W = e->window) enters here and nowhere else: the windowed entry is planned for a
// call whose LONGEST sequence exceeds W, the plain kernel otherwise.  That the choice may look at the call at all rests on the
// windowed kernels' contract (llama_kernels.h): they differ from the plain ones only in chunks they skip and keys they mask, so a
// sequence no longer than W gets the same bits from either - a row still depends on its own sequence alone.
CausalAttnPlan plan_llama_attn(const rk_engine* e, int n_seq, int maxL, int n_heads, int n_kv) {
  CausalAttnPlan p;
  if (e->window > 0 && maxL > e->window) p.window = e->window;
  if (head_width(e) == 64) {
    // 64-wide heads: ONE kernel for every length, whatever llama_attn_dma / llama_attn_nw say (they choose between 128-wide
    // kernels): plan_enc_attn's D128 precedent.  Static LDS (reported, not requested at launch).
    p.hd = 64; p.grid = dim3((maxL + 127) / 128, n_heads, n_seq); p.lds = ATC64_LDS_BYTES;
    return p;
  }
  // K / V chunks by LDS-DMA, V^T by transposing reads (round 5); chosen by the option alone: batch-independent
  if (!e->opt.llama_attn_dma) { p.grid = dim3((maxL + 127) / 128, n_heads, n_seq); return p; }   // (no windowed form: causal_attn_exists)
  p.kind = CAUSAL_DMA;
  p.nw = e->opt.llama_attn_nw == 8 ? 8 : 4;   // same bits either way
  p.nqb = (maxL + 32 * p.nw - 1) / (32 * p.nw); p.grid = dim3(xcd_grid(n_seq * n_kv, (n_heads / n_kv) * p.nqb));
  p.block = 64 * p.nw; p.lds = p.lds_opt_in = ATCD_LDS_BYTES;
#ifdef RK_MEASURE
  p.lds_opt_in += 49152;
  if (e->opt.attn_ko & 256) p.lds += 49152;   // residency probe: 112 KiB per workgroup = ONE per CU for certain
#endif
  return p;
}

// what the launcher reads of a call: llama_prefill fills it from its slot and the model, rk_debug_attn from host operands
struct CausalAttnCall { const half_t* qkv; half_t* ctx; const int* seq_off; int ld, ldctx, n_heads, n_kv, n_seq, maxL, T; };
// The one walk from a plan to the template arguments: f(kind, D, NW, WIN), each an integral_constant (NW = 0 for the tile kind).
// A plan outside causal_attn_exists is a host bug and aborts HERE (the callers refuse it first).
template <class Fn>
void with_causal_attn(const CausalAttnPlan& p, Fn&& f) {
  using std::integral_constant;
  with_int<CAUSAL_TILE, CAUSAL_DMA>(p.kind, [&](auto k) {
    with_width(p.hd, [&](auto d) {
      with_int<0, 1>(p.window > 0, [&](auto w) {
        auto go = [&](auto nw) {
          constexpr bool W = decltype(w)::value != 0;
          if constexpr (causal_attn_exists(decltype(k)::value, decltype(d)::value, W)) f(k, d, nw, std::bool_constant<W>());
          else abort();
        };
        if constexpr (decltype(k)::value == CAUSAL_TILE) go(integral_constant<int, 0>{});
        else switch (p.nw) {
          case 8: go(integral_constant<int, 8>{}); break;
          case 4: go(integral_constant<int, 4>{}); break;
          default: abort();
        }
      });
    });
  });
}
void launch_llama_attn(rk_engine* e, hipStream_t st, const CausalAttnCall& c, const CausalAttnPlan& p) {
  const int T = c.T, Q = c.n_heads * p.hd, KV = c.n_kv * p.hd;
  const float scale_log2e = (1.0f / std::sqrt((float)p.hd)) * 1.4426950408889634f;   // head_dim**-0.5 * log2(e)
  AttnCausalArgs a{c.qkv, c.ctx, c.seq_off, c.ld, c.ldctx, c.n_heads, c.n_kv, scale_log2e, 0, 0, e->opt.attn_ko};
  if (p.kind == CAUSAL_DMA) { a.n_seq = c.n_seq; a.nqb = p.nqb; }
  Bracket br(e, st, PC_ENC_ATTN, 2.0 * (double)c.maxL * T * Q, (double)T * (2 * Q + 2 * KV) * 2.0);   // causal: half of 4 L T Q
  with_causal_attn(p, [&](auto k, auto d, auto nw, auto w) {
    constexpr bool WIN = decltype(w)::value;
    const auto args = [&] { if constexpr (WIN) return AttnCausalWinArgs{a, p.window}; else return a; }();
    if constexpr (decltype(k)::value == CAUSAL_DMA) launch_lds<attn_causal_dma_kernel<decltype(nw)::value, WIN>>(st, p.grid, p.block, p.lds, p.lds_opt_in, args);
    else hipLaunchKernelGGL((attn_causal_tile_kernel<decltype(d)::value, WIN>), p.grid, dim3(p.block), 0, st, args);
  });
}
int refuse_window(rk_engine* e, const char* entry, int maxL) {
  return fail(e, RK_ERR_STATE, "%s: a sequence of %d tokens on an engine with sliding window %d needs a windowed attention kernel, and option llama_attn_dma = 0 selects attn_causal_tile_kernel<128>, which has none", entry, maxL, e->window);
}

// Single-token attention of one rk_llama_generate step over the K / V cache of P positions per sequence: the chunk kernel over
// (key chunks of P, groups of R query heads, rows), then the merge per (head, row).  R = the largest of 8 / 4 / 2 / 1 that divides
// the query heads per kv head G (Llama-3-8B: 4): a model constant, so a row's bits never depend on the call.  Nor do they depend
// on R: a head's arithmetic in attn_dec_cached_kernel indexes every per-head array by r alone and the merge is per head.
// R = G = 7 (Qwen2.5-7B: 28 heads on 4, R = 1 by the rule, every cached byte read 7 times) has an instantiation of its own behind
// option llama_dec_r = 2 (measurement and tests only; G = 6 / 5 / 3 were not measured and have none), but is NOT the rule: measured at Qwen2.5-7B widths it lost at one row (6.19 against 5.95 ms
// per token: 17 chunks x 4 kv heads = 68 workgroups on 256 CUs, where R = 1 has 476 and L2 serves the re-reads) and only tied
// at eight rows (7.60 / 7.65; profiles/rankr1_bench.txt).  llama_dec_r = 1 forces R = 1.  Same bits whichever (tests).
// A 64-wide engine runs the same kernels at D = 64 by the same rule with the same chunk length; it has no R = 7 instantiation, so
// llama_dec_r = 2 falls back to the rule there.
// On an engine with a sliding window every step runs the windowed entries (attn_dec_cached_win_kernel, attn_dec_combine_win_kernel):
// a model constant again.  A row at pos < W skips and masks nothing there and gets the plain kernels' bits.
// An FP8-cache engine (rk_llama_set_kv_fp8; 128 wide): kv8 = 1, the byte kernels (attn_dec_kv8_kernel<.., 1>, attn_dec_keys_kv8_kernel,
// kv8_cache_append_kernel) over the four regions of Kv8Cache, or kv8 = 2 (option llama_kv_fp8 = 0), the fp16 layout holding dequantised
// values: the fp16 reader with the rounded own key (attn_dec_kv8_kernel<.., 2>), the fp16 KEYS kernels behind the rounding append.  The
// same rule for R; it has no R = 7 instantiation, so llama_dec_r = 2 falls back to the rule, as at width 64.
struct LlamaDecAttnPlan { int R = 1, nch = 1, hd = 128, window = 0; dim3 grid, cgrid; int kv8 = 0; };
inline int kv8_mode(const rk_engine* e) { return e->kv_fp8 ? (e->opt.llama_kv_fp8 ? 1 : 2) : 0; }
LlamaDecAttnPlan plan_llama_dec_attn(const rk_engine* e, int rows, int P, int n_heads, int n_kv) {
  LlamaDecAttnPlan p;                                        // (no CU count enters: fixed chunk length, model-constant R)
  const int G = n_heads / n_kv;
  p.hd = head_width(e);
  p.kv8 = kv8_mode(e);
  p.R = G % 8 == 0 ? 8 : (G % 4 == 0 ? 4 : (G % 2 == 0 ? 2 : 1));
  if (e->opt.llama_dec_r == 1) p.R = 1;
  if (e->opt.llama_dec_r == 2 && G == 7 && p.hd == 128 && !p.kv8) p.R = 7;
  p.nch = (P + LDC_CHUNK - 1) / LDC_CHUNK;
  p.grid = dim3(p.nch, n_heads / p.R, rows);
  p.cgrid = dim3(n_heads, rows);
  p.window = e->window;
  return p;
}

// ---- which kernels the step's attention has: THE one statement (the walk, the entries and the launches below follow it) ----
// form: what the call carries, derived in launch_llama_dec_attn alone - Qwen3's head norm (never with bias or window: rk_engine_finalize),
// else the engine's window with or without the layer's Qwen2 bias, else the bias, else the Llama kernel as it was.
enum DecForm { DEC_PLAIN, DEC_BIAS, DEC_WIN, DEC_WIN_BIAS, DEC_QKN };
constexpr bool dec_form_bias(int f) { return f == DEC_BIAS || f == DEC_WIN_BIAS; }
constexpr bool dec_form_win(int f) { return f == DEC_WIN || f == DEC_WIN_BIAS; }
// * R = 8 / 4 / 2 / 1 everywhere; R = 7 at width 128 on an fp16 cache alone (plan_llama_dec_attn gives it nowhere else);
// * the head norm at width 128 only; an FP8 cache (kv8 = 1 bytes, 2 dequantised fp16) at width 128 only;
// * each of these as the plain step and as the KEYS step (a drafting session's, behind the append): KEYS constrains nothing.
constexpr bool dec_attn_exists(int D, int R, int form, int kv8) {
  return (D == 128 || D == 64) && (R == 8 || R == 4 || R == 2 || R == 1 || (R == 7 && D == 128 && kv8 == 0)) &&
         form >= DEC_PLAIN && form <= DEC_QKN && (form != DEC_QKN || D == 128) && (kv8 == 0 || ((kv8 == 1 || kv8 == 2) && D == 128));
}
// The chunk kernel of a combination that exists.  kv8 = 2 with KEYS is the fp16 KEYS kernel: it forms no key, and the rounding
// append in front of it has left dequantised values in the fp16 layout.
template <int D, int R, int F, bool KEYS, int KV8>
constexpr auto dec_attn_entry() {
  static_assert(dec_attn_exists(D, R, F, KV8), "no such kernel");
  constexpr bool B = dec_form_bias(F), W = dec_form_win(F), Q = F == DEC_QKN;
  if constexpr (KV8 == 1 && KEYS) return &attn_dec_keys_kv8_kernel<R, B, W, Q>;
  else if constexpr (KV8 != 0 && !KEYS) return &attn_dec_kv8_kernel<R, B, W, Q, KV8>;
  else if constexpr (Q && KEYS) return &attn_dec_keys_qkn_kernel<D, R>;
  else if constexpr (Q) return &attn_dec_cached_qkn_kernel<D, R>;
  else if constexpr (W && KEYS) return &attn_dec_keys_win_kernel<D, R, B>;
  else if constexpr (W) return &attn_dec_cached_win_kernel<D, R, B>;
  else if constexpr (KEYS) return &attn_dec_keys_kernel<D, R, B>;
  else return &attn_dec_cached_kernel<D, R, B>;
}
// ... and the append in front of a KEYS step, which knows no R and no window: the fp16 kernel, or the rounding one in the cache's mode
template <int D, int F, int KV8>
constexpr auto kv_append_entry() {
  constexpr bool B = dec_form_bias(F), Q = F == DEC_QKN;
  if constexpr (KV8 != 0) return &kv8_cache_append_kernel<B, Q, KV8>;
  else return &kv_cache_append_kernel<D, B, Q>;
}
// The one walk from a plan and a call's form to the template arguments: f(D, R, form, KEYS, kv8), each an integral_constant.  A
// combination outside dec_attn_exists is a host bug and aborts HERE.
template <class Fn>
void with_dec_attn(const LlamaDecAttnPlan& p, int form, bool keys, Fn&& f) {
  with_width(p.hd, [&](auto d) {
    auto go = [&](auto r) {
      with_int<DEC_PLAIN, DEC_BIAS, DEC_WIN, DEC_WIN_BIAS, DEC_QKN>(form, [&](auto fm) {
        with_int<0, 1>(keys, [&](auto k) {
          with_int<0, 1, 2>(p.kv8, [&](auto m) {
            constexpr bool K = decltype(k)::value != 0;
            if constexpr (dec_attn_exists(decltype(d)::value, decltype(r)::value, decltype(fm)::value, decltype(m)::value))
              f(d, r, fm, std::bool_constant<K>(), m);
            else abort();
          });
        });
      });
    };
    using std::integral_constant;
    switch (p.R) {
      case 8: go(integral_constant<int, 8>{}); break;
      case 7: go(integral_constant<int, 7>{}); break;
      case 4: go(integral_constant<int, 4>{}); break;
      case 2: go(integral_constant<int, 2>{}); break;
      case 1: go(integral_constant<int, 1>{}); break;
      default: abort();
    }
  });
}

// The step's attention, the one entry of its callers (llama_step_rows, rk_debug_attn kind 5, rk_debug_kv8_step): `rows` step rows
// over the layer's cache cc (llama_kv_layer; a.kc / a.vc come from it).  g1 == 1 (and no `live`): the plain step - the chunk kernel
// forms, uses and writes each row's key - then the merge.  Else a drafting session's step (rk_llama_session_open_draft): rows =
// cache rows * g1; the append puts every live row's key and value where a plain step would have written them, then the KEYS
// entries (the plain body without the new-key select and the cache write) run by the SAME plan over `rows`, and the plain merge:
// one more small launch per layer than the plain step.
void launch_llama_dec_attn(rk_engine* e, hipStream_t st, const LlamaDecAttnPlan& p, LlamaDecAttnArgs a, int rows, int g1, const int* live,
                           const Kv8Cache& cc) {
  const bool keys = g1 != 1;
  a.kc = cc.kc; a.vc = cc.vc; a.nch = p.nch; a.window = p.window;
  const LlamaDecAttnKv8Args a8{{a, g1, live}, cc.ke, cc.ve, cc.pe};   // every entry takes it, or the base of it that is its own struct
  const int form = a.qkn ? DEC_QKN : (p.window > 0 ? (a.bias ? DEC_WIN_BIAS : DEC_WIN) : (a.bias ? DEC_BIAS : DEC_PLAIN));
  // a byte plan without its exponent planes, a KEYS step without its live flags, a head norm beside a bias or a window: host bugs
  if ((p.kv8 == 1 && (!cc.ke || !cc.ve || cc.pe < a.P)) || (keys && (g1 < 1 || !live)) || (a.qkn && (a.bias || p.window > 0))) abort();
  Bracket br(e, st, PC_DEC_ATTN, 4.0 * rows * (double)a.P * a.n_heads * p.hd, 2.0 * rows * (double)a.P * a.n_kv * p.hd * (p.kv8 == 1 ? 1.0 : 2.0));
  with_dec_attn(p, form, keys, [&](auto d, auto r, auto f, auto k, auto m) {
    constexpr int D = decltype(d)::value, R = decltype(r)::value, F = decltype(f)::value, KV8 = decltype(m)::value;
    constexpr bool KEYS = decltype(k)::value;
    if constexpr (KEYS) hipLaunchKernelGGL((kv_append_entry<D, F, KV8>()), dim3(rows), dim3(256), 0, st, a8);
    hipLaunchKernelGGL((dec_attn_entry<D, R, F, KEYS, KV8>()), p.grid, dim3(256), 0, st, a8);
    // the merge is per (head, row): the plain kernels for every form, mode and step
    hipLaunchKernelGGL((dec_form_win(F) ? attn_dec_combine_win_kernel<D> : attn_dec_combine_kernel<D>), p.cgrid, dim3(D), 0, st, a8);
  });
}

// The slot's previous launch may still be in its decoder: the encoder chain stops here until that one is done.  (Read back
// already, or everything on one stream: nothing to wait for.)
int wait_prev_decoder(rk_engine* e, Slot& sl) {
  hipStream_t se = enc_stream(e, sl);
  if (sl.dec_pending && dec_stream(e, sl) != se) HIPCHK(e, hipStreamWaitEvent(se, sl.ev_dec, 0));
  return RK_OK;
}

// hf: modeling_t5.py:663-750 (T5Stack.forward, encoder) over the slot's staged ragged batch, then the stacked
// cross-attention K/V projections of all decoder layers (:325-326 with key_value_states = encoder output).
int run_encoder(rk_engine* e, Slot& sl, bool need_cross_kv) {
  const rk_model_desc& d = e->d;
  hipStream_t st = enc_stream(e, sl);
  const int T = sl.T, I = e->inner, dm = d.d_model, F = d.d_ff;
  // The fill-in tile variants of small launches (one setwise prompt) may form their row factors themselves (option consumer_stats):
  // two 5-us launches per layer less where launches are what costs.
  const bool own = e->opt.consumer_stats != 0;
  int rc = RK_OK;
  NormStream ns = sl.enc;
  const EncAttnPlan ap = plan_enc_attn(e, sl.n_seq, sl.maxL, sl.minL, d.n_heads);
  const int* seq_off = sl.stg_seq_off[sl.gen];
  ns.begin(e, st, sl.stg_tokens[sl.gen], T, e->opt.fold_norm != 0);
  for (int l = 0; l < d.n_enc_layers; ++l) {
    const EncLayerW& w = e->enc[l];
    const bool last = l + 1 == d.n_enc_layers;
    RC(gemm(e, st, ns.consumer(e, st, w.ln0, Gemm(PC_ENC_GEMM_QKV, EPI_STORE_F16, ns.x(), dm, ns.fold ? w.qkv_f : w.qkv, dm, sl.qkv, 3 * I, T, 3 * I, dm), own)));
    launch_enc_attn(e, st, EncAttnCall{sl.qkv, sl.ctx, seq_off, e->lut_enc, 3 * I, I, I, d.n_heads, sl.n_seq, sl.maxL, sl.T}, ap);
    RC(ns.producer(e, st, Gemm(PC_ENC_GEMM_O, EPI_RESID_F32, sl.ctx, I, w.o, I, ns.hidden, dm, T, dm, I)));
    RC(gemm(e, st, ns.consumer(e, st, w.ln1, Gemm(PC_ENC_GEMM_FFN_IN, d.gated_gelu ? EPI_GEGLU_F16 : EPI_RELU_F16, ns.x(), dm, ns.fold ? w.ffn_in_f : w.ffn_in, dm,
                                                 sl.ffh, F, T, d.gated_gelu ? 2 * F : F, dm), own)));
    RC(ns.producer(e, st, Gemm(PC_ENC_GEMM_FFN_OUT, EPI_RESID_F32, sl.ffh, F, w.ffn_out, F, ns.hidden, dm, T, dm, F), !last));
  }
  // From here on the chain writes what the decoder of the slot's previous launch reads (the table at Slot): dec_seq_off, enc_out, cross_kv
  RC(wait_prev_decoder(e, sl));
  if (sl.off_of != sl.stage_no) {   // the decoder's own copy of the offsets: it outlives the generation the host stages next
    HIPCHK(e, hipMemcpyAsync(sl.dec_seq_off, seq_off, (size_t)(sl.n_seq + 1) * sizeof(int), hipMemcpyDeviceToDevice, st));
    sl.off_of = sl.stage_no;
  }
  rmsnorm(e, st, ns.hidden, e->enc_final_ln, sl.enc_out, nullptr, T);
  // the stacked K/V projections are only materialised when the decoder has too many rows for the query-side form
  if (need_cross_kv)
    RC(gemm(e, st, Gemm(PC_GEMM_CROSS_KV, EPI_STORE_F16, sl.enc_out, dm, e->cross_kv_w, dm, sl.cross_kv, 2 * I, T, d.n_dec_layers * 2 * I, dm)
                       .split(2 * I, (long)d.max_tokens * 2 * I)));
  sl.have_cross_kv = need_cross_kv;
  HIPCHK(e, hipGetLastError());
  return RK_OK;
}

// hf: modeling_t5.py:663-750 (decoder stack) for Ld teacher-forced positions per sequence (ids already on the
// device in sl.idx.d[IX_DEC_IDS], row = b*Ld + t).  Leaves the residual stream in sl.dec.hidden.
// tree (rk_t5_greedy2): the decoder rows are not Ld per sequence - several continuations of a prompt share the rows of their
// common prefix.  rows = row count, Ld = longest position count; device arrays: keys[r * Ld + j] = row at position j of
// row r's sequence, pos[r] = position of row r, seq[r] = its encoder sequence.  Query-side cross-attention only.
// ragged (rk_t5_qlm_many): the pass covers the sequences seq0 .. seq0 + n_seq - 1 of the slot's batch, each with its OWN position
// count (all of one DecLenClass; Ld = the longest): sequence seq0 + b owns the rows row_off[b] .. row_off[b + 1] - 1 at positions
// 0, 1, ..; seq[r] = encoder sequence of row r (index into the slot's batch), ids = the pass's decoder ids; cross_kv: the pass
// reads the materialised K / V (the encoder made them) - otherwise the query-side form, whatever the encoder left.
struct DecRows {
  int rows; const int* keys; const int* pos; const int* seq;
  const int* row_off; int seq0, n_seq; bool cross_kv; const int* ids;
  bool tree() const { return keys != nullptr; }
};
// cache (rk_t5_generate): the incremental pass - ONE new row per sequence (Ld = 1) at the position *pos on the device, layer l's
// self-attention K / V cache at kv + l * B * P * 2I.  The layer is the one-position chain's (fused query-side cross-attention,
// folded norms, tiled FFN-in: every family from the call shape, never from B) but for self-attention: the QKV projection of the
// new row, then attn_dec_cached_kernel over the cache.  tree_keys / tree_pos: option dec_cached_attn = 0 (attn_dec_kernel's
// tree form over the cache rows b * P + j).
struct DecCache { half_t* kv; int P; const int* pos; const int* tree_keys; int* tree_pos; };
// The T5 cached step's self-attention, one new row per sequence: attn_dec_cached_kernel, or (option dec_cached_attn = 0) the cache
// append and attn_dec_kernel's tree form over the cache rows tree_keys [B][P] names (row b P + j), at the position kv_append_kernel
// publishes in tree_pos.  run_decoder's cached branch and rk_debug_attn kind 6 both launch through here.
void launch_dec_cached_step(const rk_engine* e, hipStream_t st, const AttnCachedArgs& ca, int B, int H, const int* tree_keys, int* tree_pos) {
  if (e->opt.dec_cached_attn) {
    hipLaunchKernelGGL(attn_dec_cached_kernel, dim3(H, B), dim3(256), attn_dec_lds(ca.P), st, ca);
  } else {
    hipLaunchKernelGGL(kv_append_kernel, dim3(B), dim3(256), 0, st, ca, tree_pos);
    hipLaunchKernelGGL(attn_dec_kernel, dim3(1, H, B), dim3(256), attn_dec_lds(ca.P), st,
                       AttnDecArgs{ca.qkv, ca.ldqkv, ca.cache, ca.cache + ca.inner, 2 * ca.inner, nullptr, ca.ctx, ca.ldctx, ca.bias_lut, ca.P, 1, ca.P,
                                   tree_keys, tree_pos});
  }
}
// (Tried and dropped, round 3: the single-position pass of 320 rows as TWO or THREE chains of 32-row-aligned row ranges on
// helper streams, fork / join by events (parallel branches of the decoder graph) - bit-identical, but 6.4-6.6k passages/s
// against 7.3k: what the decoder costs the encoder running beside it is every one of its kernels delaying the persistent
// GEMM it meets, so more, smaller decoder kernels cost more, not less.  The lever is fewer and shorter decoder kernels.)
int run_decoder(rk_engine* e, Slot& sl, int Ld, const DecRows* rows = nullptr, const DecCache* cache = nullptr) {
  const rk_model_desc& d = e->d;
  hipStream_t st = dec_stream(e, sl);
  const bool tree = rows && rows->tree(), ragged = rows && !rows->tree();
  const int B = ragged ? rows->n_seq : sl.n_seq, M = rows ? rows->rows : B * Ld, I = e->inner, dm = d.d_model, F = d.d_ff;
  const bool have_kv = ragged ? rows->cross_kv : sl.have_cross_kv;
  const int* seq_off = sl.dec_seq_off + (ragged ? rows->seq0 : 0);
  const DecLenClass lc = dec_len_class(e, Ld);
  if (tree && (have_kv || lc.one)) return fail(e, RK_ERR_STATE, "the tree form needs the query-side cross-attention and L_d >= 2");
  if (ragged && have_kv && !sl.have_cross_kv) return fail(e, RK_ERR_STATE, "the ragged pass needs the K / V the encoder did not materialise");
  if (cache && (rows || have_kv || Ld != 1)) return fail(e, RK_ERR_STATE, "the incremental pass needs the query-side cross-attention and one row per sequence");
  // 128-wide heads: the plain one-position pass only (the entry points refuse everything else before they stage or launch)
  if (wide_heads(e) && (!lc.one || rows || cache || have_kv || e->opt.dec_fuse == 2))
    return refuse_wide(e, "run_decoder", "this pass would launch a 64-wide kernel");
  const bool ws = lc.stream;   // few decoder positions: weight-streaming GEMMs (any number of sequences); else tiled
  // Folded RMSNorm on the weight-streaming path (as in the encoder, minus the statistics kernel): the residual GEMMs leave
  // the new rows as fp16 with their sums of squares per 32-column block, the GEMM behind the norm reads those with the norm
  // weight folded into its matrix and forms the row factor itself (gemm.h: GemmArgs::ssq_in) - three launches per layer less.
  const bool dfold = ws && e->opt.dec_fold_norm && (e->opt.skinny & 0x3F) == 0x3F;
  // Few-row GEMV family (round 6, gemv_rows.h): the pass of ONE setwise / pairwise prompt - a handful of rows at two or more
  // positions ("<pad> Passage": 2 rows; the second greedy step: 3) - runs its plain projections one wave per output column over all
  // CUs.  Decided from the PASS (rows, positions), so every row of a pass takes one family; a row scored alone and the same row in
  // a lockstep call of more than eight prompts differ in the last bits.  The one-position pointwise decoder
  // (any row count) never takes it: its batch independence stays bit-exact.
  // Row limit (option dec_gemv_rows, default 4): measured cross-over at flan-t5-large dims and 1 450-token prompts, whole calls,
  // GEMV against weight-streaming MFMA family: 2 rows 4.87 / 5.20 ms, 4 rows 6.38 / 6.67, 6 rows 8.30 / 8.25, 8 rows 9.41 / 9.39,
  // 12 rows 12.86 / 12.36, 16 rows 15.18 / 14.58 (profiles/r06_few_rows_ab.txt) - every workgroup stages ALL rows in LDS and the
  // per-column VALU work grows with the rows; rk_t5_greedy2's 13-row tree pass stays on the matrix cores.  A pass that asked for
  // the fused cross-attention projections (below) never takes it, whether or not they can run.
  // Query-side cross-attention with the projections around it fused per (head, row slab) (dec_fuse = 1, the default): 3 launches
  // instead of 5.  Measured (r04): at 100-320 rows (pointwise, one decoder position) the fused pair is 9 us per layer faster and the
  // grouped pipeline gains 1.2 %; at the 13 rows x 23 chunks of a setwise compare it is 4 us per layer SLOWER (the separate GEMMs
  // spread the cold weights of a layer over 512 + 5120 workgroups).  The family follows from the CALL SHAPE, never from the batch
  // (the two round differently): fused for one decoder position, separate beyond (dec_fuse = 2 forces the fused form: tests)
  const bool fuse_asked = e->opt.dec_fuse == 2 || (e->opt.dec_fuse == 1 && lc.one);
  const bool few = dfold && e->opt.dec_gemv && !lc.one && M <= e->opt.dec_gemv_rows && !fuse_asked &&
                   gemv_fits(M, dm) && gemv_fits(M, I) && gemv_fits(M, F);   // every K of the pass's projections
  const GemmFamily fam = few ? GEMM_GEMV : (ws ? GEMM_STREAM : GEMM_TILED);
  int rc = RK_OK;
  NormStream ns = sl.dec;
  if (few) { ns.ssq[0] = sl.dssq_few[0]; ns.ssq[1] = sl.dssq_few[1]; }
  // the GEMM c of this pass's family behind the norm ln: every consumer here may form its row factors itself
  auto normed = [&](const float* ln, Gemm c) { return ns.consumer(e, st, ln, c.on(fam), true); };
  auto resid = [&](Gemm c, bool stats = true) { return ns.producer(e, st, c.on(fam), stats); };
  ns.begin(e, st, ragged && rows->ids ? rows->ids : sl.idx.d[IX_DEC_IDS], M, dfold);
  const DecAttnPlan self_plan = plan_dec_attn(e, false, B, Ld, Ld, d.n_heads, tree ? rows->rows : 0);
  const DecAttnPlan cross_plan = plan_dec_attn(e, true, B, Ld, sl.maxL, d.n_heads, 0);
  for (int l = 0; l < d.n_dec_layers; ++l) {
    const DecLayerW& w = e->dec[l];
    if (!cache && lc.one) {
      // one decoder position: softmax over a single key is 1, so self-attention is exactly o(v(x)) — the q/k
      // projections, scores and bias are dead (hf: modeling_t5.py:448-509 at L_d = 1)
      // ... and o(v(x)) = (W_o W_v) x: one GEMM with the product matrix formed once at finalize
      RC(resid(normed(w.ln0, Gemm(PC_DEC_GEMM, EPI_RESID_F32, ns.x(), dm, dfold ? w.ov_f : w.ov, dm, ns.hidden, dm, M, dm, dm))));
    } else {
      RC(gemm(e, st, normed(w.ln0, Gemm(PC_DEC_GEMM, EPI_STORE_F16, ns.x(), dm, dfold ? w.qkv_f : w.qkv, dm, sl.dqkv, 3 * I, M, 3 * I, dm))));
      if (cache) {
        const AttnCachedArgs ca{sl.dqkv, 3 * I, cache->kv + (size_t)l * B * cache->P * 2 * I, cache->P, I, cache->pos, sl.dctx, I, e->lut_dec};
        Bracket br(e, st, PC_DEC_ATTN, 4.0 * B * (double)cache->P * I, (double)B * cache->P * 2 * I * 2.0);
        launch_dec_cached_step(e, st, ca, B, d.n_heads, cache->tree_keys, cache->tree_pos);
      } else {
        launch_dec_attn(e, st, self_plan, AttnDecArgs{sl.dqkv, 3 * I, sl.dqkv + I, sl.dqkv + 2 * I, 3 * I, nullptr, sl.dctx, I, e->lut_dec, Ld, 1, Ld,
                                                      tree ? rows->keys : nullptr, tree ? rows->pos : nullptr, 0, ragged ? rows->row_off : nullptr},
                        4.0 * M * Ld * I, 0);
      }
      RC(resid(Gemm(PC_DEC_GEMM, EPI_RESID_F32, sl.dctx, I, w.o, I, ns.hidden, dm, M, dm, I)));
    }
    // the cross-attention q projection: a GEMM of its own, or fused into the chain's first kernel, which takes the same norm hooks
    const Gemm cq = normed(w.ln1, Gemm(PC_DEC_GEMM, EPI_STORE_F16, ns.x(), dm, dfold ? w.cq_f : w.cq, dm, sl.dq, I, M, I, dm));
    if (!have_kv) {
      RC(run_xattn_chain(e, st, XAttnChain{cq.A, cq.lda, cq.W, w.ckT, e->cross_kv_w + ((size_t)l * 2 * I + I) * dm, cq.fold, cq.family,
                                           sl.enc_out, sl.dec_seq_off, rows ? rows->seq : nullptr, Ld, 0, sl.dq, sl.xqk, sl.xpart, sl.xstat, sl.xctx,
                                           sl.dctx, I, M, d.n_heads, dm, sl.maxL, sl.T, fuse_asked, head_width(e)}));
    } else {
      RC(gemm(e, st, cq));
      const half_t* kv = sl.cross_kv + (size_t)l * d.max_tokens * 2 * I;
      launch_dec_attn(e, st, cross_plan, AttnDecArgs{sl.dq, I, kv, kv + I, 2 * I, seq_off, sl.dctx, I, nullptr, Ld, 0, sl.maxL, nullptr, nullptr, 0,
                                                       ragged ? rows->row_off : nullptr},
                      4.0 * Ld * (double)sl.T * I, (double)sl.T * 2 * I * 2.0);
    }
    RC(resid(Gemm(PC_DEC_GEMM, EPI_RESID_F32, sl.dctx, I, w.co, I, ns.hidden, dm, M, dm, I)));
    {
      // ONE decoder position (pointwise yes_no, MonoT5), folded: FFN-in runs on the TILED kernels whatever the number of rows.  Its
      // 5632 output columns are 176 column blocks x (rows / 32) workgroups for the weight-streaming kernel - 1760 at the
      // bench's 320 rows, 29.9 us per layer - against 440 tiles of 64x64 on the matrix cores, 14.5 us (dec_gemm 0.32 ->
      // 0.28 ms per step, +0.9 % passages/s).  The family follows from the call shape (L_d == 1), never from the batch, so a
      // row's bits still do not depend on what shares its launch; the other projections of the layer (1024 columns: 80 tiles)
      // measured the same on either family and stay where they were.
      // (Many rows, or a forced tile shape: the persistent ping-pong kernel takes its row factors ready-made - same block sums,
      // same rk_row_factor, same bits as the fill-in kernels form in their epilogue.)
      const bool tiled_in = dfold && e->opt.dec_ffn_tiled && lc.one;
      RC(gemm(e, st, ns.consumer(e, st, w.ln2, Gemm(PC_DEC_GEMM, d.gated_gelu ? EPI_GEGLU_F16 : EPI_RELU_F16, ns.x(), dm, dfold ? w.ffn_in_f : w.ffn_in, dm,
                                                   sl.dffh, F, M, d.gated_gelu ? 2 * F : F, dm).on(tiled_in ? GEMM_TILED : fam), true)));
    }
    // (the tiled form for FFN-out - 80 tiles of 64x64 with 44 K steps each - took 9 us per layer off the serial profile and
    // nothing measurable off the pipeline: left on the weight-streaming kernel)
    RC(resid(Gemm(PC_DEC_GEMM, EPI_RESID_F32, sl.dffh, F, w.ffn_out, F, ns.hidden, dm, M, dm, F), l + 1 < d.n_dec_layers));
  }
  HIPCHK(e, hipGetLastError());
  return RK_OK;
}

// Encoder on s_enc, decoder on s_dec, ordered by events.  The decoder of this slot's PREVIOUS launch must be done before the
// encoder overwrites what it reads - the chain's last kernels only (run_encoder: wait_prev_decoder), so the layers before them run
// beside that decoder.  Option enc_serial: the chain also starts behind the OTHER slot's last encoder chain - one encoder at a
// time with the decoder before it alongside, instead of two encoder chains sharing the chip kernel by kernel; same bits.
// query_side: the caller's decoder takes the query-side cross-attention whatever its length (rk_t5_generate: one row per step).
// need_cross_kv: some decoder pass of the call reads the materialised K / V.
int encoder_then_handoff_kv(rk_engine* e, Slot& sl, bool need_cross_kv) {
  hipStream_t se = enc_stream(e, sl), sd = dec_stream(e, sl);
  if (need_cross_kv && !sl.cross_kv) return refuse_wide(e, "encoder", "the materialised cross-attention K / V are not allocated");
  static_assert(RK_SLOTS == 2, "the other slot");
  const Slot& other = e->slots[(&sl - e->slots) ^ 1];
  if (e->opt.enc_serial && sd != se && other.enc_gen >= 0) HIPCHK(e, hipStreamWaitEvent(se, other.ev_enc[other.enc_gen], 0));
  sl.gen_launched = true;
  const int rc = run_encoder(e, sl, need_cross_kv);
  HIPCHK(e, hipEventRecord(sl.ev_enc[sl.gen], se));   // (also behind a chain that stopped half-way: what it enqueued reads the generation)
  sl.enc_gen = sl.gen;
  if (rc) return rc;
  if (sd != se) HIPCHK(e, hipStreamWaitEvent(sd, sl.ev_enc[sl.gen], 0));
  return RK_OK;
}

int encoder_then_handoff(rk_engine* e, Slot& sl, int max_ld, bool query_side = false) {
  return encoder_then_handoff_kv(e, sl, !query_side && !use_xattn_direct(e, sl, max_ld));
}

int mark_decoder_done(rk_engine* e, Slot& sl) {
  HIPCHK(e, hipEventRecord(sl.ev_dec, dec_stream(e, sl)));
  sl.dec_pending = true;
  return RK_OK;
}

int sync_all(rk_engine* e) {
  for (Slot& sl : e->slots) {
    HIPCHK(e, hipStreamSynchronize(sl.se));
    HIPCHK(e, hipStreamSynchronize(sl.sd));
  }
  return RK_OK;
}

// The blocking T5 entry points end here: the slot's decoder event, every stream drained.
int finish_blocking(rk_engine* e, Slot& sl) {
  int rc = mark_decoder_done(e, sl);
  if (rc || (rc = sync_all(e))) return rc;
  sl.dec_pending = false;
  return RK_OK;
}

template <class T>
int Grown<T>::reserve(rk_engine* e, size_t n, int* gen) {
  if (n <= cap) return RK_OK;
  int rc = sync_all(e);
  if (rc) return rc;
  if (p) HIPCHK(e, hipFree(p));
  p = nullptr; cap = 0;
  HIPCHK(e, hipMalloc((void**)&p, n * sizeof(T)));
  cap = n;
  if (gen) ++*gen;
  return RK_OK;
}

int ensure_logits(rk_engine* e, size_t rows) {
  // fused qlm head: rows x ceil(vocab / 32) float2 block statistics, then rows floats of label logits (the [rows, vocab]
  // fp32 logits this buffer used to hold are never materialised)
  return e->logits.reserve(e, rows * (2 * ((size_t)(e->d.vocab + 31) / 32) + 1), &e->logits_gen);
}

float head_scale(const rk_engine* e) {   // hf: modeling_t5.py:1044-1045 (scale_decoder_outputs)
  return e->d.tied_head ? 1.0f / std::sqrt((float)e->d.d_model) : 1.0f;
}

// The checks of a ragged batch; with a slot, its shape is recorded there (without: the caller stages another order of it).
int check_batch(rk_engine* e, Slot* sl, const int32_t* tokens, const int32_t* off, int n_seq) {
  if (!e->finalized) return fail(e, RK_ERR_STATE, "engine not finalized");
  if (!tokens || !off || n_seq <= 0) return fail(e, RK_ERR_INVALID, "empty batch (n_seq=%d)", n_seq);
  if (n_seq > e->d.max_seqs) return fail(e, RK_ERR_CAPACITY, "n_seq %d > max_seqs %d", n_seq, e->d.max_seqs);
  if (off[0] != 0) return fail(e, RK_ERR_INVALID, "seq_offsets[0] must be 0");
  int maxL = 0, minL = 1 << 30;
  for (int b = 0; b < n_seq; ++b) {
    const int L = off[b + 1] - off[b];
    if (L <= 0) return fail(e, RK_ERR_INVALID, "sequence %d is empty", b);
    maxL = std::max(maxL, L);
    minL = std::min(minL, L);
  }
  const int T = off[n_seq];
  if (T > e->d.max_tokens) return fail(e, RK_ERR_CAPACITY, "%d tokens > max_tokens %d", T, e->d.max_tokens);
  for (int t = 0; t < T; ++t)
    if (tokens[t] < 0 || tokens[t] >= e->d.vocab) return fail(e, RK_ERR_INVALID, "token id %d out of range at %d", tokens[t], t);
  if (attn_dec_lds(maxL) > 160 * 1024 || maxL > 65536)
    return fail(e, RK_ERR_CAPACITY, "sequence of %d tokens exceeds the cross-attention LDS budget", maxL);
  if (sl) { sl->maxL = maxL; sl->minL = minL; sl->T = T; sl->n_seq = n_seq; }
  return RK_OK;
}

int check_ids(rk_engine* e, const int32_t* ids, int n, const char* what) {
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= e->d.vocab) return fail(e, RK_ERR_INVALID, "%s id %d out of range", what, ids[i]);
  return RK_OK;
}

// the same Ld decoder ids for every sequence of the slot's batch
int put_dec_ids_shared(rk_engine* e, Slot& sl, const int32_t* prefix, int Ld) {
  std::vector<int> ids((size_t)sl.n_seq * Ld);
  for (int b = 0; b < sl.n_seq; ++b) memcpy(&ids[(size_t)b * Ld], prefix, Ld * sizeof(int));
  return sl.idx.put(e, dec_stream(e, sl), IX_DEC_IDS, ids.data(), (int)ids.size());
}

// decoder input of teacher-forced labels = shift_right(labels): [decoder_start(0), labels[:-1]]  (hf: modeling_t5.py:618-637)
void shift_right(const int32_t* labels, int n, std::vector<int>* out) {
  for (int t = 0; t < n; ++t) out->push_back(t ? labels[t - 1] : 0);
}

// dec_prefix / dec_len / max_new of the greedy entry points
int check_greedy_args(rk_engine* e, const int32_t* dec_prefix, int dec_len, int max_new) {
  if (!dec_prefix || dec_len <= 0 || max_new <= 0 || dec_len + max_new - 1 > e->d.max_dec_len)
    return fail(e, RK_ERR_CAPACITY, "dec_len %d + max_new %d exceeds max_dec_len %d", dec_len, max_new, e->d.max_dec_len);
  return RK_OK;
}

// The end of a blocking call that returns floats: the slot's first n scores through its pinned buffer, the call's stream st
// finished (T5, with its two streams per slot: finish_blocking).
int read_scores_blocking(rk_engine* e, Slot& sl, hipStream_t st, size_t n, float* out) {
  HIPCHK(e, hipMemcpyAsync(sl.h_scores, sl.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, st));
  if (e->family == 0) { const int rc = finish_blocking(e, sl); if (rc) return rc; }
  else HIPCHK(e, hipStreamSynchronize(st));
  HIPCHK(e, hipGetLastError());
  memcpy(out, sl.h_scores, n * sizeof(float));
  return RK_OK;
}

int stage_slot(rk_engine* e, int slot, const int32_t* tokens, const int32_t* seq_offsets, int n_seq) {
  if (slot < 0 || slot >= RK_SLOTS) return fail(e, RK_ERR_INVALID, "slot %d out of range", slot);
  if (e->family != 0) return fail(e, RK_ERR_STATE, "T5 entry point called on a Llama engine (use rk_llama_*)");
  int rc = set_device(e);
  if (rc) return rc;
  Slot& sl = e->slots[slot];
  sl.staged = false;
  if ((rc = check_batch(e, &sl, tokens, seq_offsets, n_seq))) return rc;
  // The generation no enqueued launch reads (the table at Slot): the other one if a launch took the current, else the current
  // again.  Its last reader was an encoder chain, the slot's last but one at the latest: this waits for no decoder and not for
  // the slot's newest launch.
  const int g = sl.gen_launched ? sl.gen ^ 1 : sl.gen;
  HIPCHK(e, hipEventSynchronize(sl.ev_enc[g]));   // (never recorded: returns at once)
  HIPCHK(e, hipMemcpy(sl.stg_tokens[g], tokens, (size_t)sl.T * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.stg_seq_off[g], seq_offsets, (size_t)(n_seq + 1) * sizeof(int), hipMemcpyHostToDevice));
  sl.gen = g; sl.gen_launched = false; ++sl.stage_no;
  sl.staged = true;
  return RK_OK;
}

// The decoder chain of a call is ~300 dependent launches of kernels that run for a few microseconds each: issued eagerly
// it is bound by the host's launch rate (about 10 us per launch end to end), replayed as ONE HIP graph by the GPU's own
// dependent-kernel boundary (1-2 us).  `body` enqueues the chain on `st`; the second time a key is seen the chain is
// captured, instantiated and cached, from then on it is replayed.  A replay carries the launch arguments of the call it was
// captured from, so the key holds every value those depend on (shapes, the chunk count or the longest sequence, buffer
// generations, the options epoch); everything else a chain reads (lengths, ids, positions) lives in device memory that is
// per-slot and never moves (tests/test_gpu_graph_replay.py replays every kind on batches that share a key and differ in the rest).
// The buffers that DO move (Grown) stand in the key with their move counters: tests/test_gpu_graph_moves.py moves each behind a capture.
// Profiling runs and dec_graph = 0 stay eager (per-kernel events) and leave the table alone.
// The table holds at most RK_GRAPH_CACHE_KEYS keys: the key that would pass the bound ERASES every other entry (evict_graphs) -
// their graphs, their sightings, and the entries of epochs that no call can reach any more - and the keys still in use come back
// on their next two sightings.  One eviction per RK_GRAPH_CACHE_KEYS new keys; every outcome is counted (rk_debug_graph_stats).
enum GraphKind { GK_T5_SCORE, GK_T5_GREEDY_STEP, GK_T5_GREEDY2, GK_T5_GENERATE_STEP, GK_LLAMA_STEP, GK_T5_COMPARE, GK_LLAMA_SESSION_STEP, GK_LLAMA_STEP_SAMPLED, GK_LLAMA_SESSION_STEP_SAMPLED, GK_LLAMA_SESSION_STEP_DRAFT };   // which chain: the key's first int
// Every entry but `keep` goes.  A graph of the other slot, or of this stream's previous call, may still be replaying: both slots'
// decoder streams and slot 0's encoder stream (the Llama family's, and every decoder's with overlap = 0) are drained first, so
// no graph is destroyed under a launch.  (Erasing the other elements of a std::map leaves the reference to `keep` valid.)
int evict_graphs(rk_engine* e, const rk_engine::GraphEntry* keep) {
  for (Slot& sl : e->slots) HIPCHK(e, hipStreamSynchronize(sl.sd));
  HIPCHK(e, hipStreamSynchronize(e->slots[0].se));
  for (auto it = e->graphs.begin(); it != e->graphs.end();) {
    if (&it->second == keep) { ++it; continue; }
    if (it->second.exec) { hipGraphExecDestroy(it->second.exec); ++e->graph_count.evictions; }
    it = e->graphs.erase(it);
  }
  return RK_OK;
}
template <class F>
int run_graphed(rk_engine* e, hipStream_t st, std::vector<int> key, F&& body) {
  auto& n = e->graph_count;
  auto eager = [&]() -> int { ++n.eager; return body(); };
  key.push_back(e->opt_epoch);
  if (!e->opt.dec_graph || e->prof_on) return eager();
  auto& g = e->graphs[key];
  if (g.exec) { HIPCHK(e, hipGraphLaunch(g.exec, st)); ++n.replays; return RK_OK; }
  if ((int)e->graphs.size() > RK_GRAPH_CACHE_KEYS) {      // bounded cache: this key passed the bound, everything else goes
    const int rc = evict_graphs(e, &g);
    if (rc) return rc;
  }
  if (g.failed || g.seen++ == 0) return eager();          // first sighting: eager (also does the one-off kernel attribute calls)
  auto failed = [&]() -> int { g.failed = true; ++n.failed; return eager(); };   // nothing was executed during a capture: run it now
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return failed(); }
  const int rc = body();
  const hipError_t ec = hipStreamEndCapture(st, &graph);
  if (rc != RK_OK || ec != hipSuccess || !graph) {
    (void)hipGetLastError();
    if (graph) hipGraphDestroy(graph);
    if (rc != RK_OK) { g.failed = true; ++n.failed; return rc; }
    return failed();
  }
  const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (ei != hipSuccess || !g.exec) { (void)hipGetLastError(); g.exec = nullptr; return failed(); }
  HIPCHK(e, hipGraphLaunch(g.exec, st));
  ++n.captures;
  return RK_OK;
}

// The cached decoding loop of rk_t5_generate, rk_llama_generate and rk_llama_session_run.  `step` (one graph under `key`) decodes
// one position of every sequence on st and leaves the decoder's word in *d_word: the step at which the last sequence finished (0:
// none yet), or a session's running number of finishes.  `forced` steps (a prefix) run before the first step that yields an output
// column; columns below `first_col` were produced, and *d_word set, before the call (the Llama prefill's).  The host reads back one
// word per column into a two-entry pinned ring and waits for the PREVIOUS column's while the next step is queued: one step stays
// ahead, and a step after the last changes nothing (the advance kernels).  It stops behind the word that differs from `baseline`,
// or at column `limit`; *issued (null: not wanted) = the steps it enqueued.  Nothing is allocated here: the ring is the caller's
// to ensure (ensure_decode_ring, with its other memory, before the chain starts).
int ensure_decode_ring(rk_engine* e) {
  if (e->gen_pin) return RK_OK;
  HIPCHK(e, hipHostMalloc((void**)&e->gen_pin, 16 * sizeof(int), hipHostMallocDefault));
  for (hipEvent_t& ev : e->ev_gen) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  return RK_OK;
}
template <class F>
int decode_loop(rk_engine* e, hipStream_t st, const std::vector<int>& key, F&& step, int forced, int first_col, int limit, const int* d_word,
                int baseline, int* issued = nullptr) {
  int* pin = e->gen_pin;
  auto request = [&](int c) -> int {                                       // column c's word, read back
    HIPCHK(e, hipMemcpyAsync(pin + (c & 1), d_word, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipEventRecord(e->ev_gen[c & 1], st));
    return RK_OK;
  };
  int rc = RK_OK, steps = 0;
  if (first_col > 0) RC(request(first_col - 1));
  bool stop = false;
  for (int c = first_col - forced; c < limit && !stop; ++c, ++steps) {     // this step's column (< 0: a forced step)
    RC(run_graphed(e, st, key, step));
    if (c >= 0) RC(request(c));
    if (c >= 1) {                                                          // the previous column's word, while this step runs
      HIPCHK(e, hipEventSynchronize(e->ev_gen[(c - 1) & 1]));
      stop = pin[(c - 1) & 1] != baseline;
    }
  }
  if (issued) *issued = steps;
  return RK_OK;
}
// behind decode_loop: d_out's [n_seq][max_new] tokens and the final word; the stream is idle afterwards
int decode_result(rk_engine* e, hipStream_t st, int n_seq, int max_new, const int* d_word, const int* d_out, int32_t* out_tokens, int32_t* out_steps) {
  std::vector<int> res((size_t)n_seq * max_new + 1);
  HIPCHK(e, hipMemcpyAsync(res.data(), d_out, (size_t)n_seq * max_new * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(e, hipMemcpyAsync(res.data() + (size_t)n_seq * max_new, d_word, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(e, hipStreamSynchronize(st));
  HIPCHK(e, hipGetLastError());
  memcpy(out_tokens, res.data(), (size_t)n_seq * max_new * sizeof(int));
  if (out_steps) *out_steps = res[(size_t)n_seq * max_new];
  return RK_OK;
}

int score_slot(rk_engine* e, int slot, const int32_t* dec_prefix, int dec_len, const int32_t* out_token_ids, int n_out) {
  if (slot < 0 || slot >= RK_SLOTS) return fail(e, RK_ERR_INVALID, "slot %d out of range", slot);
  int rc = set_device(e);
  if (rc) return rc;
  Slot& sl = e->slots[slot];
  if (!sl.staged) return fail(e, RK_ERR_STATE, "no staged batch in slot %d", slot);
  if (!dec_prefix || dec_len <= 0 || dec_len > e->d.max_dec_len) return fail(e, RK_ERR_CAPACITY, "dec_len %d out of range (max %d)", dec_len, e->d.max_dec_len);
  if (!out_token_ids || n_out <= 0 || n_out > 64) return fail(e, RK_ERR_INVALID, "n_out must be in 1..64 (got %d)", n_out);
  if ((rc = check_ids(e, dec_prefix, dec_len, "decoder")) || (rc = check_ids(e, out_token_ids, n_out, "output"))) return rc;
  if (wide_heads(e) && dec_len > 1) return refuse_wide(e, "rk_t5_score", "dec_len > 1 has no 128-wide decoder self-attention");
  if ((rc = check_wide_one(e, "rk_t5_score"))) return rc;
  hipStream_t sd = dec_stream(e, sl);
  if ((rc = put_dec_ids_shared(e, sl, dec_prefix, dec_len))) return rc;
  if ((rc = sl.idx.put(e, sd, IX_OUT_IDS, out_token_ids, n_out))) return rc;
  std::vector<int> rows(sl.n_seq);
  for (int b = 0; b < sl.n_seq; ++b) rows[b] = b * dec_len + dec_len - 1;
  if ((rc = sl.idx.put(e, sd, IX_LAST_ROWS, rows.data(), sl.n_seq))) return rc;
  if ((rc = encoder_then_handoff(e, sl, dec_len))) return rc;
#ifdef RK_MEASURE   // measurement builds only (never what build() ships): encoder-chain floor, scores are garbage
  static const bool skip_dec = getenv("RK_DEBUG_SKIP_DECODER") != nullptr;
#else
  constexpr bool skip_dec = false;
#endif
  rc = run_graphed(e, sd, {GK_T5_SCORE, slot, sl.n_seq, dec_len, sl.have_cross_kv ? sl.maxL : (sl.maxL + 63) / 64, (int)sl.have_cross_kv, n_out, (int)skip_dec}, [&]() -> int {
    int r = RK_OK;
    if (!skip_dec && (r = run_decoder(e, sl, dec_len))) return r;
    rmsnorm(e, sd, sl.dec.hidden, e->dec_final_ln, sl.dlast, sl.idx.d[IX_LAST_ROWS], sl.n_seq, head_scale(e));
    Bracket br(e, sd, PC_HEAD, 2.0 * sl.n_seq * n_out * e->d.d_model, 0);
    launch_head_rows(sd, sl.dlast, e->lm_head, sl.idx.d[IX_OUT_IDS], sl.d_scores, sl.n_seq, n_out, e->d.d_model);
    return RK_OK;
  });
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(sl.h_scores, sl.d_scores, (size_t)sl.n_seq * n_out * sizeof(float), hipMemcpyDeviceToHost, sd));
  HIPCHK(e, hipGetLastError());
  sl.last_floats = sl.n_seq * n_out;
  return mark_decoder_done(e, sl);
}

// score_slot's twin for the duoT5 compare: the staged batch is pairs of sequences (2p, 2p + 1), the decoder has one position,
// and pair_verdict_kernel takes the place of head_rows_kernel: logits, P(true) and verdicts in the slot's score buffer.
int compare_slot(rk_engine* e, int slot, int dec_start_id, int false_id, int true_id) {
  if (slot < 0 || slot >= RK_SLOTS) return fail(e, RK_ERR_INVALID, "slot %d out of range", slot);
  if (e->family != 0) return fail(e, RK_ERR_STATE, "T5 entry point called on a Llama engine (use rk_llama_*)");
  int rc = set_device(e);
  if (rc) return rc;
  Slot& sl = e->slots[slot];
  if (!sl.staged) return fail(e, RK_ERR_STATE, "no staged batch in slot %d", slot);
  if (sl.n_seq % 2) return fail(e, RK_ERR_INVALID, "a compare needs pairs of sequences (staged n_seq = %d)", sl.n_seq);
  const int32_t out_ids[2] = {false_id, true_id};
  if ((rc = check_ids(e, &dec_start_id, 1, "decoder")) || (rc = check_ids(e, out_ids, 2, "output"))) return rc;
  if (false_id == true_id) return fail(e, RK_ERR_INVALID, "false_id and true_id are the same id %d", false_id);
  if ((rc = check_wide_one(e, "rk_t5_compare"))) return rc;
  hipStream_t sd = dec_stream(e, sl);
  if ((rc = put_dec_ids_shared(e, sl, &dec_start_id, 1))) return rc;
  std::vector<int> rows(sl.n_seq);
  for (int b = 0; b < sl.n_seq; ++b) rows[b] = b;
  if ((rc = sl.idx.put(e, sd, IX_LAST_ROWS, rows.data(), sl.n_seq))) return rc;
  if ((rc = encoder_then_handoff(e, sl, 1))) return rc;
  rc = run_graphed(e, sd, {GK_T5_COMPARE, slot, sl.n_seq, sl.have_cross_kv ? sl.maxL : (sl.maxL + 63) / 64, (int)sl.have_cross_kv, false_id, true_id}, [&]() -> int {
    int r = RK_OK;
    if ((r = run_decoder(e, sl, 1))) return r;
    rmsnorm(e, sd, sl.dec.hidden, e->dec_final_ln, sl.dlast, sl.idx.d[IX_LAST_ROWS], sl.n_seq, head_scale(e));
    Bracket br(e, sd, PC_HEAD, 2.0 * sl.n_seq * 2 * e->d.d_model, 0);
    launch_pair_verdict(sd, sl.dlast, e->lm_head, false_id, true_id, sl.d_scores, sl.n_seq, e->d.d_model);
    return RK_OK;
  });
  if (rc) return rc;
  const int n_floats = 3 * sl.n_seq + sl.n_seq / 2;
  HIPCHK(e, hipMemcpyAsync(sl.h_scores, sl.d_scores, (size_t)n_floats * sizeof(float), hipMemcpyDeviceToHost, sd));
  HIPCHK(e, hipGetLastError());
  sl.last_floats = n_floats;
  return mark_decoder_done(e, sl);
}


// ---- RCCL, loaded on first use: a 1-GPU process never needs it, and when PyTorch is in the process the SONAME
// librccl.so.1 resolves to the copy torch already mapped (one RCCL per process, like the HIP runtime) ----------------
struct RcclApi {
  void* h = nullptr; bool tried = false; std::string err;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;   // optional
};
RcclApi g_rccl;

// Which librccl: ONE per process.  When PyTorch is in the process its wheel's own copy (torch/lib/librccl.so, 2.26.6 in this
// image against 2.27.7 under /opt/rocm) is usually mapped already - a second, different RCCL beside it would bring its own
// HSA / IPC state.  So: (1) the copy already mapped into this process (first "librccl" entry of /proc/self/maps), by its
// exact path; (2) the SONAME through the loader's search path; (3) the ROCm install.  rk_comm_library_info reports the
// path and version actually bound, and bench.py / run.py log it.
std::string mapped_rccl_path() {
  FILE* f = fopen("/proc/self/maps", "r");
  if (!f) return "";
  char line[4096];
  std::string found;
  while (fgets(line, sizeof line, f)) {
    const char* p = strstr(line, "librccl");
    if (!p) continue;
    const char* path = strchr(line, '/');
    if (!path) continue;
    found.assign(path);
    while (!found.empty() && (found.back() == '\n' || found.back() == ' ')) found.pop_back();
    break;
  }
  fclose(f);
  return found;
}

const RcclApi* rccl_api() {
  if (g_rccl.tried) return g_rccl.h ? &g_rccl : nullptr;
  g_rccl.tried = true;
  const std::string mapped = mapped_rccl_path();
  if (!mapped.empty()) g_rccl.h = dlopen(mapped.c_str(), RTLD_NOW | RTLD_GLOBAL);
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    if (g_rccl.h) break;
    g_rccl.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
  }
  if (!g_rccl.h) { g_rccl.err = std::string("dlopen(librccl.so.1) failed: ") + (dlerror() ? dlerror() : "?"); return nullptr; }
#define RK_SYM(field, sym)                                                              \
  g_rccl.field = (decltype(g_rccl.field))dlsym(g_rccl.h, sym);                        \
  if (!g_rccl.field) { g_rccl.err = std::string("librccl lacks ") + sym; dlclose(g_rccl.h); g_rccl.h = nullptr; return nullptr; }
  RK_SYM(GetUniqueId, "ncclGetUniqueId") RK_SYM(CommInitRank, "ncclCommInitRank") RK_SYM(CommDestroy, "ncclCommDestroy")
  RK_SYM(AllGather, "ncclAllGather") RK_SYM(GetErrorString, "ncclGetErrorString")
#undef RK_SYM
  g_rccl.GetVersion = (decltype(g_rccl.GetVersion))dlsym(g_rccl.h, "ncclGetVersion");
  return &g_rccl;
}

void comm_release(rk_engine* e) {
  if (e->comm) { if (const RcclApi* r = rccl_api()) r->CommDestroy(e->comm); e->comm = nullptr; }
  for (int i = 0; i < RK_SLOTS; ++i) {
    if (e->d_gather[i]) { hipFree(e->d_gather[i]); e->d_gather[i] = nullptr; }
    if (e->h_gather[i]) { hipHostFree(e->h_gather[i]); e->h_gather[i] = nullptr; }
    if (e->ev_gather[i]) { hipEventDestroy(e->ev_gather[i]); e->ev_gather[i] = nullptr; }
    e->gather_pending[i] = false;
  }
  if (e->d_gsend) { hipFree(e->d_gsend); e->d_gsend = nullptr; }
  if (e->d_gall) { hipFree(e->d_gall); e->d_gall = nullptr; }
  if (e->h_gall) { hipHostFree(e->h_gall); e->h_gall = nullptr; }
  if (e->h_gstage) { hipHostFree(e->h_gstage); e->h_gstage = nullptr; }
  if (e->ev_gall) { hipEventDestroy(e->ev_gall); e->ev_gall = nullptr; }
  if (e->ev_append) { hipEventDestroy(e->ev_append); e->ev_append = nullptr; }
  e->gall_pending = false; e->append_foreign = false; e->gall_n = 0;
  e->gather_cap = 0; e->comm_world = 1; e->comm_rank = 0;
}

// the gather / send / staging buffers of a communicator just created (rk_comm_init); on an error the caller releases everything
int comm_alloc_buffers(rk_engine* e) {
  const int world = e->comm_world;
  for (int i = 0; i < RK_SLOTS; ++i) {
    HIPCHK(e, hipMalloc((void**)&e->d_gather[i], e->gather_cap * world * sizeof(float)));
    HIPCHK(e, hipHostMalloc((void**)&e->h_gather[i], e->gather_cap * world * sizeof(float), hipHostMallocDefault));
    HIPCHK(e, hipEventCreateWithFlags(&e->ev_gather[i], hipEventDisableTiming));
  }
  HIPCHK(e, hipMalloc((void**)&e->d_gsend, e->gather_cap * sizeof(float)));
  HIPCHK(e, hipMemset(e->d_gsend, 0, e->gather_cap * sizeof(float)));
  HIPCHK(e, hipMalloc((void**)&e->d_gall, e->gather_cap * world * sizeof(float)));
  HIPCHK(e, hipHostMalloc((void**)&e->h_gall, e->gather_cap * world * sizeof(float), hipHostMallocDefault));
  HIPCHK(e, hipHostMalloc((void**)&e->h_gstage, e->gather_cap * sizeof(float), hipHostMallocDefault));
  HIPCHK(e, hipEventCreateWithFlags(&e->ev_gall, hipEventDisableTiming));
  HIPCHK(e, hipEventCreateWithFlags(&e->ev_append, hipEventDisableTiming));
  return RK_OK;
}

}  // namespace

// =============================================== C ABI =======================================================
extern "C" {

int rk_abi_version(void) { return 1; }

int rk_rel_bucket(int relative_position, int bidirectional, int num_buckets, int max_distance) {
  return rel_bucket(relative_position, bidirectional != 0, num_buckets, max_distance);
}

const char* rk_last_error(const rk_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int rk_profile_num_classes(void) { return PC_COUNT; }
const char* rk_profile_class_name(int cls) { return (cls >= 0 && cls < PC_COUNT) ? kProfNames[cls] : ""; }

int rk_engine_create(const rk_model_desc* desc, int device_ordinal, rk_engine** out) {
  if (!desc || !out) return fail(nullptr, RK_ERR_INVALID, "null argument");
  *out = nullptr;
  const rk_model_desc& d = *desc;
  if (d.d_kv != 64 && d.d_kv != 128)
    return fail(nullptr, RK_ERR_INVALID, "d_kv=%d unsupported: the gfx950 attention kernels are built for d_kv=64 and, for one decoder position, d_kv=128", d.d_kv);
  if (d.d_model % 64 || (d.n_heads * d.d_kv) % 64 || d.d_ff % 64 || d.vocab % 4)
    return fail(nullptr, RK_ERR_INVALID, "d_model, n_heads*d_kv, d_ff must be multiples of 64 and vocab of 4");
  if (d.d_model > 4096)
    return fail(nullptr, RK_ERR_INVALID, "d_model=%d unsupported: rmsnorm_kernel holds a row of at most 4096 columns in registers (d_model <= 4096)", d.d_model);
  if (d.max_distance > RK_LUT_R || d.n_buckets < 4 || d.n_buckets > 256)
    return fail(nullptr, RK_ERR_INVALID, "relative attention config unsupported (max_distance<=%d)", RK_LUT_R);
  if (d.max_tokens <= 0 || d.max_seqs <= 0 || d.max_dec_len <= 0 || d.n_enc_layers <= 0 || d.n_dec_layers <= 0)
    return fail(nullptr, RK_ERR_INVALID, "capacities and layer counts must be positive");
  if ((long)d.max_seqs * d.max_dec_len > 8192 * 8) return fail(nullptr, RK_ERR_INVALID, "max_seqs*max_dec_len too large");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
    return fail(nullptr, RK_ERR_NO_DEVICE, "no HIP device visible: this engine has no CPU path");
  if (device_ordinal < 0 || device_ordinal >= n_dev)
    return fail(nullptr, RK_ERR_NO_DEVICE, "device ordinal %d out of range (%d devices)", device_ordinal, n_dev);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess)
    return fail(nullptr, RK_ERR_HIP, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, RK_ERR_NO_DEVICE, "device %d is %s; kernels are built for gfx950 (MI355X) only", device_ordinal, prop.gcnArchName);
  rk_engine* e = new rk_engine();
  e->d = d; e->dev = device_ordinal; e->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256; e->inner = d.n_heads * d.d_kv;
  int prio_lo = 0, prio_hi = 0;
  bool ok = hipSetDevice(device_ordinal) == hipSuccess;
  ok = ok && hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess;
  // the decoder chain is a long sequence of tiny dependent kernels: give it dispatch priority over the encoder's
  // chip-filling GEMM grids so it progresses while they run
  for (int i = 0; ok && i < RK_SLOTS; ++i)
    ok = hipStreamCreateWithPriority(&e->slots[i].se, hipStreamNonBlocking, prio_lo) == hipSuccess &&
         hipStreamCreateWithPriority(&e->slots[i].sd, hipStreamNonBlocking, prio_hi) == hipSuccess;
  ok = ok && hipEventCreate(&e->t0) == hipSuccess && hipEventCreate(&e->t1) == hipSuccess &&
       hipEventCreateWithFlags(&e->t_tmp, hipEventDisableTiming) == hipSuccess;
  for (int i = 0; ok && i < RK_SLOTS; ++i)
    ok = hipEventCreateWithFlags(&e->slots[i].ev_enc[0], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&e->slots[i].ev_enc[1], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&e->slots[i].ev_dec, hipEventDisableTiming) == hipSuccess;
  for (int i = 0; ok && i < 2 * RK_SLOTS; ++i) {
    rk_engine::SkWs& w = e->sk_ws[i];
    w.st = (i & 1) ? e->slots[i >> 1].sd : e->slots[i >> 1].se;
    ok = hipMalloc((void**)&w.slabs, (size_t)KSPLIT_MAX_SLABS * 65536 * sizeof(float)) == hipSuccess &&
         hipMalloc((void**)&w.cnt, KSPLIT_MAX_SLABS * sizeof(int)) == hipSuccess &&
         hipMemset(w.cnt, 0, KSPLIT_MAX_SLABS * sizeof(int)) == hipSuccess;
  }
  if (!ok) {
    for (auto& w : e->sk_ws) { if (w.slabs) hipFree(w.slabs); if (w.cnt) hipFree(w.cnt); }
    delete e;
    return fail(nullptr, RK_ERR_HIP, "stream/event/workspace creation failed");
  }
  *out = e;
  return RK_OK;
}

void rk_engine_destroy(rk_engine* e) {
  if (!e) return;
  hipSetDevice(e->dev);
  for (auto& sl : e->slots) {
    if (sl.se) hipStreamSynchronize(sl.se);
    if (sl.sd) hipStreamSynchronize(sl.sd);
  }
  comm_release(e);
  for (auto& kv : e->graphs) if (kv.second.exec) hipGraphExecDestroy(kv.second.exec);
  e->graphs.clear();
  for (void* p : e->allocs) hipFree(p);
  if (e->gen_pin) hipHostFree(e->gen_pin);
  for (hipEvent_t ev : e->ev_gen) if (ev) hipEventDestroy(ev);
  for (auto& w : e->sk_ws) { if (w.slabs) hipFree(w.slabs); if (w.cnt) hipFree(w.cnt); }
  for (auto& sl : e->slots) {
    if (sl.h_scores) hipHostFree(sl.h_scores);
    if (sl.idx.pin) hipHostFree(sl.idx.pin);
    for (hipEvent_t ev : sl.ev_enc) if (ev) hipEventDestroy(ev);
    if (sl.ev_dec) hipEventDestroy(sl.ev_dec);
  }
  for (auto& r : e->prof_recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  if (e->t0) hipEventDestroy(e->t0);
  if (e->t1) hipEventDestroy(e->t1);
  if (e->t_tmp) hipEventDestroy(e->t_tmp);
  for (auto& sl : e->slots) {
    if (sl.se) hipStreamDestroy(sl.se);
    if (sl.sd) hipStreamDestroy(sl.sd);
  }
  delete e;   // (frees the Grown buffers)
}

int rk_engine_load_tensor(rk_engine* e, const char* hf_name, const void* data, int dtype, const int64_t* shape, int ndim) {
  if (!e || !hf_name || !data || !shape) return fail(e, RK_ERR_INVALID, "null argument");
  if (e->finalized) return fail(e, RK_ERR_STATE, "engine already finalized");
  if (ndim < 1 || ndim > 2) return RK_OK;   // nothing on the path has another rank
  std::string name(hf_name);
  // duplicates of shared.weight in HF checkpoints
  if (name == "encoder.embed_tokens.weight" || name == "decoder.embed_tokens.weight") return RK_OK;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  const bool keep_f32 = ndim == 1 || name.find("relative_attention_bias") != std::string::npos;
  auto get = [&](size_t i) -> float {
    switch (dtype) {
      case RK_F32: return ((const float*)data)[i];
      case RK_F16: return (float)((const half_t*)data)[i];
      case RK_BF16: { uint32_t u = (uint32_t)((const uint16_t*)data)[i] << 16; float f; memcpy(&f, &u, 4); return f; }
      default: return 0.f;
    }
  };
  if (dtype < RK_F32 || dtype > RK_BF16) return fail(e, RK_ERR_INVALID, "unknown dtype %d", dtype);
  if (keep_f32) { t.f.resize(n); for (size_t i = 0; i < n; ++i) t.f[i] = get(i); }
  else if (dtype == RK_F16) { t.h.assign((const half_t*)data, (const half_t*)data + n); }
  else { t.h.resize(n); for (size_t i = 0; i < n; ++i) t.h[i] = (half_t)get(i); }
  e->host[name] = std::move(t);
  return RK_OK;
}

static int llama_finalize(rk_engine* e);

int rk_engine_finalize(rk_engine* e) {
  if (!e) return RK_ERR_INVALID;
  if (e->finalized) return fail(e, RK_ERR_STATE, "already finalized");
  int rc = set_device(e);
  if (rc) return rc;
  if (e->family == 1) return llama_finalize(e);
  const rk_model_desc& d = e->d;
  const int I = e->inner, dm = d.d_model, F = d.d_ff, V = d.vocab;
  std::string missing;
  auto N2 = [&](const std::string& n, int64_t r, int64_t c) { return need(e, n, r, c, &missing); };
  auto N1 = [&](const std::string& n, int64_t r) { return need(e, n, r, -1, &missing); };

  // pass 1: presence / shape check of everything so the error lists all problems at once
  N2("shared.weight", V, dm);
  if (!d.tied_head) N2("lm_head.weight", V, dm);
  N1("encoder.final_layer_norm.weight", dm); N1("decoder.final_layer_norm.weight", dm);
  N2("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", d.n_buckets, d.n_heads);
  N2("decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", d.n_buckets, d.n_heads);
  auto ffn_names = [&](const std::string& p, std::vector<std::string>* v) {
    if (d.gated_gelu) { v->push_back(p + ".wi_0.weight"); v->push_back(p + ".wi_1.weight"); } else v->push_back(p + ".wi.weight");
  };
  for (int l = 0; l < d.n_enc_layers; ++l) {
    const std::string p = "encoder.block." + std::to_string(l) + ".layer";
    for (const char* m : {"q", "k", "v"}) N2(p + ".0.SelfAttention." + m + ".weight", I, dm);
    N2(p + ".0.SelfAttention.o.weight", dm, I);
    N1(p + ".0.layer_norm.weight", dm); N1(p + ".1.layer_norm.weight", dm);
    std::vector<std::string> fn; ffn_names(p + ".1.DenseReluDense", &fn);
    for (auto& s : fn) N2(s, F, dm);
    N2(p + ".1.DenseReluDense.wo.weight", dm, F);
  }
  for (int l = 0; l < d.n_dec_layers; ++l) {
    const std::string p = "decoder.block." + std::to_string(l) + ".layer";
    for (const char* a : {".0.SelfAttention.", ".1.EncDecAttention."}) {
      for (const char* m : {"q", "k", "v"}) N2(p + a + m + ".weight", I, dm);
      N2(p + a + "o.weight", dm, I);
    }
    N1(p + ".0.layer_norm.weight", dm); N1(p + ".1.layer_norm.weight", dm); N1(p + ".2.layer_norm.weight", dm);
    std::vector<std::string> fn; ffn_names(p + ".2.DenseReluDense", &fn);
    for (auto& s : fn) N2(s, F, dm);
    N2(p + ".2.DenseReluDense.wo.weight", dm, F);
  }
  if (!missing.empty()) return fail(e, RK_ERR_MISSING, "missing or mis-shaped tensors: %s", missing.c_str());

  auto H = [&](const std::string& n) -> const std::vector<half_t>& { return e->host[n].h; };
  auto Fv = [&](const std::string& n) -> const std::vector<float>& { return e->host[n].f; };
  auto up_h = [&](half_t** dst, const std::vector<half_t>& v) { return upload(e, dst, v.data(), v.size()); };
  auto up_f = [&](float** dst, const std::vector<float>& v) { return upload(e, dst, v.data(), v.size()); };
  auto cat3 = [&](const std::string& p) {
    std::vector<half_t> v;
    v.reserve((size_t)3 * I * dm);
    for (const char* m : {"q", "k", "v"}) { const auto& s = H(p + m + ".weight"); v.insert(v.end(), s.begin(), s.end()); }
    return v;
  };
  // wi_0 | wi_1 interleaved in groups of 32 output rows: the GEGLU epilogue finds gate and up of one output
  // column in the same lane / same accumulator index of two adjacent 32x32 MFMA fragments.
  auto ffn_in = [&](const std::string& p) {
    if (!d.gated_gelu) return H(p + ".wi.weight");
    const auto& g = H(p + ".wi_0.weight"); const auto& u = H(p + ".wi_1.weight");
    std::vector<half_t> v((size_t)2 * F * dm);
    for (int blk = 0; blk < F / 32; ++blk) {
      memcpy(&v[((size_t)blk * 64) * dm], &g[((size_t)blk * 32) * dm], (size_t)32 * dm * sizeof(half_t));
      memcpy(&v[((size_t)blk * 64 + 32) * dm], &u[((size_t)blk * 32) * dm], (size_t)32 * dm * sizeof(half_t));
    }
    return v;
  };
  // folded RMSNorm: W'[n][k] = fp16(W[n][k] * ln[k])  (the norm weight multiplies the GEMM's input channels)
  auto folded = [&](const std::vector<half_t>& wm, const std::vector<float>& ln) {
    std::vector<half_t> v(wm.size());
    const size_t rows = wm.size() / dm;
    for (size_t r = 0; r < rows; ++r)
      for (int k = 0; k < dm; ++k) v[r * dm + k] = (half_t)((float)wm[r * dm + k] * ln[k]);
    return v;
  };
  RC(up_h(&e->emb, H("shared.weight")));
  if (d.tied_head) e->lm_head = e->emb; else RC(up_h(&e->lm_head, H("lm_head.weight")));
  RC(up_f(&e->enc_final_ln, Fv("encoder.final_layer_norm.weight")));
  RC(up_f(&e->dec_final_ln, Fv("decoder.final_layer_norm.weight")));
  for (int stack = 0; stack < 2; ++stack) {
    const auto& tab = Fv(std::string(stack ? "decoder" : "encoder") + ".block.0.layer.0.SelfAttention.relative_attention_bias.weight");
    std::vector<float> lut((size_t)d.n_heads * RK_LUT_N);
    for (int rel = -RK_LUT_R; rel <= RK_LUT_R; ++rel) {
      const int bkt = rel_bucket(rel, stack == 0, d.n_buckets, d.max_distance);
      for (int h = 0; h < d.n_heads; ++h) lut[(size_t)h * RK_LUT_N + rel + RK_LUT_R] = tab[(size_t)bkt * d.n_heads + h];
    }
    RC(up_f(stack ? &e->lut_dec : &e->lut_enc, lut));
  }
  e->enc.resize(d.n_enc_layers);
  for (int l = 0; l < d.n_enc_layers; ++l) {
    const std::string p = "encoder.block." + std::to_string(l) + ".layer";
    EncLayerW& w = e->enc[l];
    RC(up_h(&w.qkv, cat3(p + ".0.SelfAttention.")));
    RC(up_h(&w.o, H(p + ".0.SelfAttention.o.weight")));
    RC(up_h(&w.ffn_in, ffn_in(p + ".1.DenseReluDense")));
    RC(up_h(&w.ffn_out, H(p + ".1.DenseReluDense.wo.weight")));
    RC(up_f(&w.ln0, Fv(p + ".0.layer_norm.weight")));
    RC(up_f(&w.ln1, Fv(p + ".1.layer_norm.weight")));
    RC(up_h(&w.qkv_f, folded(cat3(p + ".0.SelfAttention."), Fv(p + ".0.layer_norm.weight"))));
    RC(up_h(&w.ffn_in_f, folded(ffn_in(p + ".1.DenseReluDense"), Fv(p + ".1.layer_norm.weight"))));
  }
  e->dec.resize(d.n_dec_layers);
  std::vector<half_t> ckv;
  ckv.reserve((size_t)d.n_dec_layers * 2 * I * dm);
  for (int l = 0; l < d.n_dec_layers; ++l) {
    const std::string p = "decoder.block." + std::to_string(l) + ".layer";
    DecLayerW& w = e->dec[l];
    RC(up_h(&w.qkv, cat3(p + ".0.SelfAttention.")));
    RC(up_h(&w.o, H(p + ".0.SelfAttention.o.weight")));
    RC(up_h(&w.cq, H(p + ".1.EncDecAttention.q.weight")));
    RC(up_h(&w.co, H(p + ".1.EncDecAttention.o.weight")));
    RC(up_h(&w.ckT, regroup_ckT(H(p + ".1.EncDecAttention.k.weight").data(), d.n_heads, dm, d.d_kv)));
    RC(up_h(&w.ffn_in, ffn_in(p + ".2.DenseReluDense")));
    RC(up_h(&w.ffn_out, H(p + ".2.DenseReluDense.wo.weight")));
    RC(up_f(&w.ln0, Fv(p + ".0.layer_norm.weight")));
    RC(up_f(&w.ln1, Fv(p + ".1.layer_norm.weight")));
    RC(up_f(&w.ln2, Fv(p + ".2.layer_norm.weight")));
    RC(up_h(&w.qkv_f, folded(cat3(p + ".0.SelfAttention."), Fv(p + ".0.layer_norm.weight"))));
    RC(up_h(&w.cq_f, folded(H(p + ".1.EncDecAttention.q.weight"), Fv(p + ".1.layer_norm.weight"))));
    RC(up_h(&w.ffn_in_f, folded(ffn_in(p + ".2.DenseReluDense"), Fv(p + ".2.layer_norm.weight"))));
    for (const char* m : {"k", "v"}) { const auto& s = H(p + ".1.EncDecAttention." + m + ".weight"); ckv.insert(ckv.end(), s.begin(), s.end()); }
  }
  RC(up_h(&e->cross_kv_w, ckv));
  {
    // W_ov[n][k] = sum_j W_o[n][j] W_v[j][k]  via the engine GEMM: A = W_o [d, I], W = W_v^T [d, I]  (fp32 out)
    half_t* d_vT = nullptr; float* d_ov32 = nullptr;
    RC(dalloc(e, &d_vT, (size_t)dm * I)); RC(dalloc(e, &d_ov32, (size_t)dm * dm));
    std::vector<half_t> vT((size_t)dm * I), ov16((size_t)dm * dm);
    std::vector<float> ov32((size_t)dm * dm);
    for (int l = 0; l < d.n_dec_layers; ++l) {
      const std::string p = "decoder.block." + std::to_string(l) + ".layer.0.SelfAttention.";
      const auto& wv = H(p + "v.weight");
      for (int j = 0; j < I; ++j)
        for (int k = 0; k < dm; ++k) vT[(size_t)k * I + j] = wv[(size_t)j * dm + k];
      HIPCHK(e, hipMemcpy(d_vT, vT.data(), vT.size() * 2, hipMemcpyHostToDevice));
      RC(gemm(e, e->slots[0].se, Gemm(PC_OTHER, EPI_STORE_F32, e->dec[l].o, I, d_vT, I, d_ov32, dm, dm, dm, I)));
      HIPCHK(e, hipStreamSynchronize(e->slots[0].se));
      HIPCHK(e, hipMemcpy(ov32.data(), d_ov32, ov32.size() * 4, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < ov32.size(); ++i) ov16[i] = (half_t)ov32[i];
      RC(up_h(&e->dec[l].ov, ov16));
      const auto& ln0 = Fv("decoder.block." + std::to_string(l) + ".layer.0.layer_norm.weight");
      for (size_t i = 0; i < ov32.size(); ++i) ov16[i] = (half_t)(ov32[i] * ln0[i % dm]);
      RC(up_h(&e->dec[l].ov_f, ov16));
    }
    HIPCHK(e, hipGetLastError());
  }
  e->host.clear();

  // workspaces, sized once for the 288 GB part: nothing is allocated on the hot path afterwards
  const size_t Tc = d.max_tokens, Bc = d.max_seqs, Mc = (size_t)d.max_seqs * d.max_dec_len;
  e->scores_cap = Bc * 64;                                  // rk_t5_score: n_out <= 64 floats per sequence; rk_t5_compare: 3.5
  if (2 * e->scores_cap < 7 * Bc) return fail(e, RK_ERR_CAPACITY, "score buffer of %zu floats cannot hold a compare of %zu sequences", e->scores_cap, Bc);
  for (Slot& sl : e->slots) {
    RC(dalloc(e, &sl.enc.hidden, Tc * dm)); RC(dalloc(e, &sl.enc.xn, Tc * dm)); RC(dalloc(e, &sl.qkv, Tc * 3 * I));
    RC(dalloc(e, &sl.ctx, Tc * I)); RC(dalloc(e, &sl.ffh, Tc * F)); RC(dalloc(e, &sl.enc_out, Tc * dm));
    RC(dalloc(e, &sl.enc.xraw[0], Tc * dm)); RC(dalloc(e, &sl.enc.ssq[0], Tc * ((dm + 63) / 64))); RC(dalloc(e, &sl.enc.factors, Tc + 512));   // padded: the ping-pong GEMM reads the row factors of a whole 256-row tile
    HIPCHK(e, hipMemset(sl.enc.factors, 0, (Tc + 512) * sizeof(float)));
    for (int g = 0; g < 2; ++g) { RC(dalloc(e, &sl.stg_tokens[g], Tc)); RC(dalloc(e, &sl.stg_seq_off[g], Bc + 1)); }
    RC(dalloc(e, &sl.dec_seq_off, Bc + 1));
    // (128-wide heads: one decoder position only, which never reads the materialised K / V - 393 KB per token at t5-3b)
    if (!wide_heads(e)) RC(dalloc(e, &sl.cross_kv, (size_t)d.n_dec_layers * Tc * 2 * I));
    RC(dalloc(e, &sl.idx.d[IX_DEC_IDS], Mc)); RC(dalloc(e, &sl.idx.d[IX_LAST_ROWS], Bc)); RC(dalloc(e, &sl.idx.d[IX_OUT_IDS], 8192));
    RC(dalloc(e, &sl.idx.d[IX_ROW_LABEL], Mc)); RC(dalloc(e, &sl.idx.d[IX_ROW_OFF], 2 * Bc + 1)); RC(dalloc(e, &sl.idx.d[IX_OUT_IDX], Bc)); RC(dalloc(e, &sl.d_argmax, Bc));
    RC(dalloc(e, &sl.idx.d[IX_ROW_SEQ], Mc)); RC(dalloc(e, &sl.idx.d[IX_TREE_KEYS], Mc * (size_t)d.max_dec_len)); RC(dalloc(e, &sl.idx.d[IX_TREE_POS], Mc));
    RC(dalloc(e, &sl.dec.hidden, Mc * dm)); RC(dalloc(e, &sl.dec.xn, Mc * dm)); RC(dalloc(e, &sl.dqkv, Mc * 3 * I));
    RC(dalloc(e, &sl.dctx, Mc * I)); RC(dalloc(e, &sl.dq, Mc * I)); RC(dalloc(e, &sl.dffh, Mc * F));
    RC(dalloc(e, &sl.dlast, Bc * dm));
    for (int i = 0; i < 2; ++i) { RC(dalloc(e, &sl.dec.xraw[i], Mc * dm)); RC(dalloc(e, &sl.dec.ssq[i], Mc * ((dm + 31) / 32))); RC(dalloc(e, &sl.dssq_few[i], (size_t)GEMV_MAX_ROWS * e->n_cu)); }
    RC(dalloc(e, &sl.dec.factors, Mc));
    RC(dalloc(e, &sl.xqk, (size_t)XA_MAX_ROWS * d.n_heads * dm)); RC(dalloc(e, &sl.xctx, (size_t)XA_MAX_ROWS * d.n_heads * dm));
    RC(dalloc(e, &sl.xpart, (size_t)XA_MAX_CHUNKS * d.n_heads * dm)); RC(dalloc(e, &sl.xstat, (size_t)XA_MAX_CHUNKS * d.n_heads * 2));
    RC(dalloc(e, &sl.d_scores, e->scores_cap));
    HIPCHK(e, hipHostMalloc((void**)&sl.h_scores, e->scores_cap * sizeof(float), hipHostMallocDefault));
    HIPCHK(e, hipHostMalloc((void**)&sl.idx.pin, IX_N_CACHED * DecIndex::PIN_INTS * sizeof(int), hipHostMallocDefault));
  }
  // dynamic-LDS opt-in (best effort) for the kernels that may exceed the 64 KiB default (check_batch refuses longer calls)
  const int dec_smem_max = (int)attn_dec_lds(std::max(d.max_tokens, d.max_dec_len));
  (void)hipFuncSetAttribute((const void*)attn_dec_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, std::min(dec_smem_max, 160 * 1024));
  (void)hipFuncSetAttribute((const void*)attn_dec_seq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
#define GEMM_ATTR(EPI)                                                                                              \
  (void)hipFuncSetAttribute((const void*)gemm_f16_kernel<EPI, true>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES); \
  (void)hipFuncSetAttribute((const void*)gemm_f16_kernel<EPI, false>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES);
  GEMM_ATTR(EPI_STORE_F16) GEMM_ATTR(EPI_RESID_F32) GEMM_ATTR(EPI_GEGLU_F16) GEMM_ATTR(EPI_RELU_F16) GEMM_ATTR(EPI_STORE_F32) GEMM_ATTR(EPI_SWIGLU_F16)
#undef GEMM_ATTR
  (void)hipGetLastError();
  HIPCHK(e, hipDeviceSynchronize());
  e->finalized = true;
  return RK_OK;
}

int rk_t5_stage_slot(rk_engine* e, int slot, const int32_t* tokens, const int32_t* seq_offsets, int n_seq) {
  if (!e) return RK_ERR_INVALID;
  return stage_slot(e, slot, tokens, seq_offsets, n_seq);
}
int rk_t5_stage(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq) {
  return rk_t5_stage_slot(e, 0, tokens, seq_offsets, n_seq);
}

int rk_t5_score_slot(rk_engine* e, int slot, const int32_t* dec_prefix, int dec_len, const int32_t* out_token_ids, int n_out) {
  if (!e) return RK_ERR_INVALID;
  return score_slot(e, slot, dec_prefix, dec_len, out_token_ids, n_out);
}
int rk_t5_score_staged(rk_engine* e, const int32_t* dec_prefix, int dec_len, const int32_t* out_token_ids, int n_out) {
  return rk_t5_score_slot(e, 0, dec_prefix, dec_len, out_token_ids, n_out);
}

int rk_engine_sync(rk_engine* e) {
  if (!e) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  return sync_all(e);
}

int rk_t5_read_scores_slot(rk_engine* e, int slot, float* out_logits, int n_floats) {
  if (!e || !out_logits || slot < 0 || slot >= RK_SLOTS) return RK_ERR_INVALID;
  Slot& sl = e->slots[slot];
  if (n_floats > sl.last_floats) return fail(e, RK_ERR_INVALID, "asked for %d floats, have %d", n_floats, sl.last_floats);
  if (sl.dec_pending) { HIPCHK(e, hipEventSynchronize(sl.ev_dec)); sl.dec_pending = false; }
  memcpy(out_logits, sl.h_scores, (size_t)n_floats * sizeof(float));
  return RK_OK;
}
int rk_t5_read_scores(rk_engine* e, float* out_logits, int n_floats) { return rk_t5_read_scores_slot(e, 0, out_logits, n_floats); }

int rk_t5_scores_device_ptr(rk_engine* e, void** out_ptr) {
  if (!e || !out_ptr) return RK_ERR_INVALID;
  *out_ptr = e->slots[0].d_scores;
  return RK_OK;
}

int rk_engine_num_slots(void) { return RK_SLOTS; }

int rk_t5_score(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, const int32_t* dec_prefix,
                int dec_len, const int32_t* out_token_ids, int n_out, float* out_logits) {
  int rc;
  if ((rc = rk_t5_stage(e, tokens, seq_offsets, n_seq))) return rc;
  if ((rc = rk_t5_score_staged(e, dec_prefix, dec_len, out_token_ids, n_out))) return rc;
  return rk_t5_read_scores(e, out_logits, n_seq * n_out);
}

int rk_t5_compare_slot(rk_engine* e, int slot, int dec_start_id, int false_id, int true_id) {
  if (!e) return RK_ERR_INVALID;
  return compare_slot(e, slot, dec_start_id, false_id, true_id);
}

int rk_t5_compare(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_pairs, int dec_start_id, int false_id,
                  int true_id, float* out_logits, float* out_p_true, int32_t* out_first_wins) {
  if (!e) return RK_ERR_INVALID;
  if (n_pairs <= 0 || n_pairs > (1 << 28) || !out_logits || !out_p_true || !out_first_wins) return fail(e, RK_ERR_INVALID, "empty compare (n_pairs=%d)", n_pairs);
  const int n_seq = 2 * n_pairs;
  int rc;
  if ((rc = rk_t5_stage(e, tokens, seq_offsets, n_seq))) return rc;
  if ((rc = rk_t5_compare_slot(e, 0, dec_start_id, false_id, true_id))) return rc;
  std::vector<float> res((size_t)7 * n_pairs);
  if ((rc = rk_t5_read_scores(e, res.data(), 7 * n_pairs))) return rc;
  memcpy(out_logits, res.data(), (size_t)2 * n_seq * sizeof(float));
  memcpy(out_p_true, res.data() + (size_t)2 * n_seq, (size_t)n_seq * sizeof(float));
  for (int p = 0; p < n_pairs; ++p) out_first_wins[p] = res[(size_t)3 * n_seq + p] != 0.f;
  return RK_OK;
}

// One decoder pass of a qlm call over the sequences s0 .. s0 + n_seq - 1 of the staged batch: `rows` rows from row r0 of
// IX_DEC_IDS / IX_ROW_LABEL (/ IX_ROW_SEQ), ld positions at most.  Uniform (off0 < 0; the whole batch, ld rows per sequence, scores
// in batch order) or ragged (run_decoder: DecRows; the sequences' row offsets from IX_ROW_OFF + off0, their scores to the
// places IX_OUT_IDX + s0 names).  cross_kv: the pass reads the materialised K / V.
struct QlmPass { int s0, n_seq, r0, rows, ld, off0; bool cross_kv; };

// The qlm computation of both entry points over the staged batch, its index buffers written: the encoder once, then per pass the
// decoder, the final norm, the head GEMM with the log-sum-exp fused into its epilogue (per row and 32-column block (max, sum exp)
// + the label's logit) and the merge into one score per sequence; the scores read back once.
static int run_qlm(rk_engine* e, Slot& sl, const std::vector<QlmPass>& passes, float* out_scores) {
  hipStream_t sd = dec_stream(e, sl);
  int* const* ix = sl.idx.d;
  int rc = RK_OK, max_rows = 0;
  bool need_kv = false;
  for (const QlmPass& p : passes) { max_rows = std::max(max_rows, p.rows); need_kv = need_kv || p.cross_kv; }
  RC(ensure_logits(e, (size_t)max_rows));
  RC(encoder_then_handoff_kv(e, sl, need_kv));
  const int nblk = (e->d.vocab + 31) / 32, dm = e->d.d_model;
  for (const QlmPass& p : passes) {
    const bool ragged = p.off0 >= 0;
    const int* off = ragged ? ix[IX_ROW_OFF] + p.off0 : nullptr;
    const DecRows rows{p.rows, nullptr, nullptr, ix[IX_ROW_SEQ] + p.r0, off, p.s0, p.n_seq, p.cross_kv, ix[IX_DEC_IDS] + p.r0};
    RC(run_decoder(e, sl, p.ld, ragged ? &rows : nullptr));
    rmsnorm(e, sd, sl.dec.hidden, e->dec_final_ln, sl.dec.xn, nullptr, p.rows, head_scale(e));
    float* xlab = e->logits.p + (size_t)p.rows * nblk * 2;
    RC(gemm(e, sd, Gemm(PC_HEAD, EPI_LSE_F32, sl.dec.xn, dm, e->lm_head, dm, e->logits.p, nblk, p.rows, e->d.vocab, dm).lse(ix[IX_ROW_LABEL] + p.r0, xlab)));
    launch_qlm_lse(sd, (const float2*)e->logits.p, nblk, xlab, ragged ? 0 : p.ld, off, ragged ? ix[IX_OUT_IDX] + p.s0 : nullptr, sl.d_scores, p.n_seq);
  }
  return read_scores_blocking(e, sl, sd, (size_t)sl.n_seq, out_scores);
}

int rk_t5_qlm(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, const int32_t* labels,
              int n_labels, float* out_scores) {
  int rc;
  if (e && wide_heads(e)) return refuse_wide(e, "rk_t5_qlm", "qlm scores several decoder positions");
  if ((rc = rk_t5_stage(e, tokens, seq_offsets, n_seq))) return rc;
  Slot& sl = e->slots[0];
  if (!labels || n_labels <= 0 || n_labels > e->d.max_dec_len) return fail(e, RK_ERR_CAPACITY, "n_labels %d out of range (max %d)", n_labels, e->d.max_dec_len);
  if ((rc = check_ids(e, labels, n_labels, "label"))) return rc;
  std::vector<int> dec_in, row_label;   // the head's label per ROW (the array rk_t5_qlm_many fills per sequence)
  shift_right(labels, n_labels, &dec_in);
  for (int b = 0; b < n_seq; ++b) row_label.insert(row_label.end(), labels, labels + n_labels);
  if ((rc = put_dec_ids_shared(e, sl, dec_in.data(), n_labels))) return rc;
  if ((rc = sl.idx.write(e, dec_stream(e, sl), {{IX_ROW_LABEL, row_label}}))) return rc;
  // ONE uniform pass: run_decoder's plain form, as rk_t5_score_slot runs it
  return run_qlm(e, sl, {{0, n_seq, 0, n_seq * n_labels, n_labels, -1, !use_xattn_direct(e, sl, n_labels)}}, out_scores);
}

// rk_t5_qlm for sequences that each score their OWN label sequence.  A sequence's score is bit for bit what rk_t5_qlm gives it
// with those labels, whatever shares the call: the sequences are ordered by the class of their label count (dec_len_class - the
// encoder does not care about order), the encoder runs ONCE over all of them (cross K / V materialised iff some class reads
// them), then every non-empty class is one ragged pass of run_qlm over its contiguous sequence range, and qlm_lse_kernel writes
// each score at the sequence's place in the caller's order.  (A pass of at most dec_gemv_rows rows at two or more positions
// takes the few-row GEMV family, as in rk_t5_qlm: DESIGN.md section 4.)
int rk_t5_qlm_many(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, const int32_t* labels,
                   const int32_t* label_offsets, float* out_scores) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 0) return fail(e, RK_ERR_STATE, "T5 entry point called on a Llama engine (use rk_llama_*)");
  if (wide_heads(e)) return refuse_wide(e, "rk_t5_qlm_many", "qlm scores several decoder positions");
  int rc;
  if ((rc = check_batch(e, nullptr, tokens, seq_offsets, n_seq))) return rc;   // before the reorder reads the batch
  if (!out_scores || !labels || !label_offsets || label_offsets[0] != 0) return fail(e, RK_ERR_INVALID, "labels, label_offsets (from 0) or output missing");
  const int max_ld = e->d.max_dec_len;
  auto n_of = [&](int b) { return label_offsets[b + 1] - label_offsets[b]; };
  for (int b = 0; b < n_seq; ++b)
    if (n_of(b) <= 0 || n_of(b) > max_ld) return fail(e, RK_ERR_CAPACITY, "sequence %d: n_labels %d out of range (max %d)", b, n_of(b), max_ld);
  if ((rc = check_ids(e, labels, label_offsets[n_seq], "label"))) return rc;
  // class index of every label count, in order of first appearance as the count grows; the sequences in class order (stable)
  std::vector<int> cls_of((size_t)max_ld + 1, 0), keys;
  std::vector<DecLenClass> classes;
  for (int n = 1; n <= max_ld; ++n) {
    const DecLenClass c = dec_len_class(e, n);
    size_t i = 0;
    while (i < keys.size() && keys[i] != c.key()) ++i;
    if (i == keys.size()) { keys.push_back(c.key()); classes.push_back(c); }
    cls_of[n] = (int)i;
  }
  std::vector<int> order((size_t)n_seq);
  for (int b = 0; b < n_seq; ++b) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cls_of[n_of(x)] < cls_of[n_of(y)]; });
  std::vector<int> ptok((size_t)seq_offsets[n_seq]), poff((size_t)n_seq + 1, 0);
  for (int s = 0; s < n_seq; ++s) {
    const int b = order[s], L = seq_offsets[b + 1] - seq_offsets[b];
    memcpy(&ptok[poff[s]], tokens + seq_offsets[b], (size_t)L * sizeof(int));
    poff[s + 1] = poff[s] + L;
  }
  if ((rc = rk_t5_stage(e, ptok.data(), poff.data(), n_seq))) return rc;
  Slot& sl = e->slots[0];
  // per row, pass after pass: decoder id, label, sequence; per pass: its sequences' row offsets (relative to the pass)
  std::vector<QlmPass> passes;
  std::vector<int> ids, rlab, rseq, roff;
  for (int s = 0; s < n_seq;) {
    const int cls = cls_of[n_of(order[s])];
    QlmPass p{s, 0, (int)ids.size(), 0, 0, (int)roff.size(), !classes[cls].direct};
    for (; s < n_seq && cls_of[n_of(order[s])] == cls; ++s, ++p.n_seq) {
      const int b = order[s], nb = n_of(b);
      const int32_t* lab = labels + label_offsets[b];
      roff.push_back(p.rows);
      shift_right(lab, nb, &ids);
      rlab.insert(rlab.end(), lab, lab + nb);
      rseq.insert(rseq.end(), nb, s);
      p.rows += nb; p.ld = std::max(p.ld, nb);
    }
    roff.push_back(p.rows);
    passes.push_back(p);
  }
  if ((rc = sl.idx.write(e, dec_stream(e, sl), {{IX_DEC_IDS, ids}, {IX_ROW_LABEL, rlab}, {IX_ROW_SEQ, rseq}, {IX_ROW_OFF, roff}, {IX_OUT_IDX, order}}))) return rc;
  return run_qlm(e, sl, passes, out_scores);
}

// Greedy head: full-vocabulary logits of `rows` final-normed rows (x: [rows, d_model] fp16) reduced to their first arg-max
// WITHOUT writing the logits: the weight-streaming GEMM keeps per 32-column block the maximum and its first column
// (gemm.h: EPI_ARGMAX_F32), argmax_blocks_kernel picks per row.  hf: modeling_t5.py:1044-1047 + torch.argmax.
// (amax_gen counts the moves of the two buffers: part of the key of every graph that holds a head)
static int ensure_amax(rk_engine* e, size_t rows) {
  const size_t n = rows * ((size_t)(e->d.vocab + 31) / 32);
  const int rc = e->amax_val.reserve(e, n, &e->amax_gen);
  return rc ? rc : e->amax_idx.reserve(e, n, &e->amax_gen);
}
static int head_argmax(rk_engine* e, hipStream_t st, const half_t* x, int rows, int d_model, int vocab, int* d_out) {
  const int nblk = (vocab + 31) / 32;
  const int rc = gemm(e, st, Gemm(PC_HEAD, EPI_ARGMAX_F32, x, d_model, e->lm_head, d_model, e->amax_val.p, nblk, rows, vocab, d_model).on(GEMM_STREAM).argmax(e->amax_idx.p));
  if (rc == RK_OK) launch_argmax_blocks(st, e->amax_val.p, e->amax_idx.p, nblk, d_out, rows);
  return rc;
}
// Sampling head (Llama family, rk_llama_set_sampling): the full-vocabulary fp32 logits of `rows` final-normed rows into e->logits
// - the weight-streaming family again, a row's logits are its own dot products whatever shares the launch - and one draw per row by
// sample_rows_kernel (sampling_kernels.h) into d_out, where the advance kernels expect the arg-max.  The token index of row r is
// pos[pos_map ? pos_map[r] : r] + 1 (the decoders' device positions: the row's last token), its seed e->d_seeds[seed_map ?
// seed_map[r] : r].  ensure_sample_head before the chain starts, never inside a capture: logits_gen stands in the graph keys.
static int ensure_sample_head(rk_engine* e, size_t rows) {
  if (e->d.vocab > sampling::MAX_VOCAB) return fail(e, RK_ERR_STATE, "sampling head: vocabulary %d beyond %d (the fixed-point sums' headroom)", e->d.vocab, sampling::MAX_VOCAB);
  int rc = e->logits.reserve(e, rows * (size_t)e->d.vocab, &e->logits_gen);
  if (rc == RK_OK && !e->d_seeds) rc = dalloc(e, &e->d_seeds, (size_t)e->d.max_seqs);
  return rc;
}
static void launch_sample_rows(hipStream_t st, const float* logits, int n_logit_rows, int vocab, const rk_engine::Sampling& sp,
                               const unsigned long long* seeds, const int* seed_map, const int* pos, const int* pos_map, int pos_add,
                               int* d_out, int* kept, int rows) {
  hipLaunchKernelGGL(sample_rows_kernel, dim3(rows), dim3(sampling::THREADS), 0, st, logits, n_logit_rows, (long)vocab, vocab, sp.T, sp.k, sp.p,
                     seeds, seed_map, pos, pos_map, pos_add, d_out, kept);
}
static int head_sample(rk_engine* e, hipStream_t st, const half_t* x, int rows, int d_model, int vocab, const rk_engine::Sampling& sp,
                       const int* seed_map, const int* pos, const int* pos_map, int* d_out) {
  const int rc = gemm(e, st, Gemm(PC_HEAD, EPI_STORE_F32, x, d_model, e->lm_head, d_model, e->logits.p, vocab, rows, vocab, d_model).on(GEMM_STREAM));
  if (rc) return rc;
  Bracket br(e, st, PC_HEAD, 0, 10.0 * rows * vocab * 4.0);
  launch_sample_rows(st, e->logits.p, rows, vocab, sp, e->d_seeds, seed_map, pos, pos_map, 1, d_out, nullptr, rows);
  return RK_OK;
}
// T5: final norm of `rows` decoder rows (row_map, or the first rows) -> arg-max head -> sl.d_argmax
static int final_argmax(rk_engine* e, hipStream_t st, Slot& sl, const int* row_map, int rows) {
  rmsnorm(e, st, sl.dec.hidden, e->dec_final_ln, sl.dlast, row_map, rows, head_scale(e));
  return head_argmax(e, st, sl.dlast, rows, e->d.d_model, e->d.vocab, sl.d_argmax);
}
// the first n arg-max ints of sl.d_argmax, read back on st (blocking)
static int read_argmax(rk_engine* e, hipStream_t st, const Slot& sl, int* out, int n) {
  HIPCHK(e, hipMemcpyAsync(out, sl.d_argmax, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(e, hipStreamSynchronize(st));
  HIPCHK(e, hipGetLastError());
  return RK_OK;
}

// One greedy step over the staged batch (encoder done): decoder over rows[b] (Ld ids per sequence), final norm of the last
// position, full-vocabulary head, arg-max -> amax[b].  Synchronous (the caller decides the next ids on the host).
static int greedy_step(rk_engine* e, Slot& sl, const std::vector<std::vector<int>>& rows, int Ld, std::vector<int>& amax) {
  const int n_seq = (int)rows.size();
  hipStream_t sd = dec_stream(e, sl);
  std::vector<int> flat((size_t)n_seq * Ld), rowmap(n_seq);
  for (int b = 0; b < n_seq; ++b) { memcpy(&flat[(size_t)b * Ld], rows[b].data(), Ld * sizeof(int)); rowmap[b] = b * Ld + Ld - 1; }
  int rc = sl.idx.write(e, sd, {{IX_DEC_IDS, flat}, {IX_LAST_ROWS, rowmap}});
  if (rc) return rc;
  rc = run_graphed(e, sd, {GK_T5_GREEDY_STEP, 0, n_seq, Ld, sl.have_cross_kv ? sl.maxL : (sl.maxL + 63) / 64, (int)sl.have_cross_kv, e->amax_gen}, [&]() -> int {
    const int r = run_decoder(e, sl, Ld);
    return r ? r : final_argmax(e, sd, sl, sl.idx.d[IX_LAST_ROWS], n_seq);
  });
  if (rc) return rc;
  amax.resize(n_seq);
  return read_argmax(e, sd, sl, amax.data(), n_seq);
}

int rk_t5_greedy(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, const int32_t* dec_prefix,
                 int dec_len, int max_new, int eos_id, int pad_id, int32_t* out_tokens, int32_t* out_steps) {
  int rc;
  if (e && wide_heads(e)) return refuse_wide(e, "rk_t5_greedy", "greedy decoding runs the decoder self-attention");
  if ((rc = rk_t5_stage(e, tokens, seq_offsets, n_seq))) return rc;
  Slot& sl = e->slots[0];
  if ((rc = check_greedy_args(e, dec_prefix, dec_len, max_new))) return rc;
  if ((rc = check_ids(e, dec_prefix, dec_len, "decoder"))) return rc;
  if ((rc = ensure_amax(e, (size_t)n_seq))) return rc;
  if ((rc = encoder_then_handoff(e, sl, dec_len + max_new - 1))) return rc;
  // Per-row decoder ids grow by one token per step; the tiny decoder is recomputed over the whole prefix each
  // step (cross K/V are reused), which equals HF's KV-cached greedy loop (hf: generation/utils.py:2868-2935).
  std::vector<std::vector<int>> rows(n_seq, std::vector<int>(dec_prefix, dec_prefix + dec_len));
  std::vector<char> done(n_seq, 0);
  std::vector<int> amax(n_seq);
  for (int b = 0; b < n_seq; ++b)
    for (int t = 0; t < max_new; ++t) out_tokens[b * max_new + t] = pad_id;
  int steps = 0;
  for (int t = 0; t < max_new; ++t) {
    if ((rc = greedy_step(e, sl, rows, dec_len + t, amax))) return rc;
    ++steps;
    bool all_done = true;
    for (int b = 0; b < n_seq; ++b) {
      const int tok = done[b] ? pad_id : amax[b];      // finished rows emit pad (hf: generation/utils.py:2927-2929)
      out_tokens[b * max_new + t] = tok;
      rows[b].push_back(tok);
      if (tok == eos_id) done[b] = 1;
      all_done = all_done && done[b];
    }
    if (all_done) break;
  }
  if ((rc = finish_blocking(e, sl))) return rc;
  if (out_steps) *out_steps = steps;
  return RK_OK;
}

// rk_t5_generate's device memory, grown between calls only: the K / V cache for n_seq sequences of P positions (a move changes
// kv_gen, which is part of the step graph's key) and the per-call int block.
static int ensure_gen(rk_engine* e, int n_seq, int P) {
  // state, prefix, finished rows, tree positions, output [n_seq][max_new], tree keys [n_seq][P]: at most this many ints
  const size_t L = (size_t)e->d.max_dec_len, S = (size_t)e->d.max_seqs;
  int rc = RK_OK;
  RC(e->kv_cache.reserve(e, (size_t)e->d.n_dec_layers * n_seq * P * 2 * e->inner, &e->kv_gen));
  RC(e->gen_buf.reserve(e, 8 + L + 2 * S + S * L + S * (L + 1)));
  return ensure_decode_ring(e);
}

// Greedy decoding with a self-attention K / V cache: one decoder row per sequence and step (run_decoder's incremental pass), the
// arg-max fed back on the device (greedy_advance_kernel), the step replayed as ONE graph whose launch arguments never change within
// the call - position, finished rows and next ids live in device memory.  Prefix positions run as forced steps through the same
// graph.  The host reads back one word per step (the finished step) and keeps one step queued ahead of the one it waits for; a
// step after the last changes nothing (greedy_advance_kernel).  Same contract as rk_t5_greedy, which recomputes the whole prefix
// every step (hf: generation/utils.py:2868-2935 is this cached loop).
int rk_t5_generate(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, const int32_t* dec_prefix,
                   int dec_len, int max_new, int eos_id, int pad_id, int32_t* out_tokens, int32_t* out_steps) {
  int rc;
  if (e && wide_heads(e)) return refuse_wide(e, "rk_t5_generate", "cached decoding runs the decoder self-attention");
  if ((rc = rk_t5_stage(e, tokens, seq_offsets, n_seq))) return rc;
  Slot& sl = e->slots[0];
  if ((rc = check_greedy_args(e, dec_prefix, dec_len, max_new))) return rc;
  if (!out_tokens) return fail(e, RK_ERR_INVALID, "null output");
  if ((rc = check_ids(e, dec_prefix, dec_len, "decoder"))) return rc;
  const int P = dec_len + max_new;                                       // cache positions per sequence (the last: a step past the end)
  if ((rc = ensure_amax(e, (size_t)n_seq))) return rc;
  if ((rc = ensure_gen(e, n_seq, P))) return rc;
  if ((rc = encoder_then_handoff(e, sl, 1, true))) return rc;
  hipStream_t sd = dec_stream(e, sl);
  // the call's int block: {t, finished step, eos, pad} | prefix | done[n] | tree_pos[n] | out[n][max_new] | tree_keys[n][P]
  const size_t o_pre = 8, o_done = o_pre + dec_len, o_tpos = o_done + n_seq, o_out = o_tpos + n_seq, o_keys = o_out + (size_t)n_seq * max_new;
  const size_t n_ints = o_keys + (size_t)n_seq * P;
  std::vector<int> init(n_ints, 0);
  init[2] = eos_id; init[3] = pad_id;
  memcpy(&init[o_pre], dec_prefix, dec_len * sizeof(int));
  for (size_t k = 0; k < (size_t)n_seq * max_new; ++k) init[o_out + k] = pad_id;
  for (int b = 0; b < n_seq; ++b)
    for (int j = 0; j < P; ++j) init[o_keys + (size_t)b * P + j] = b * P + j;
  std::vector<int> ids0(n_seq, dec_prefix[0]);
  int* g = e->gen_buf.p;
  if ((rc = sl.idx.write(e, sd, {{IX_DEC_IDS, ids0}}))) return rc;   // (leaves sd idle)
  HIPCHK(e, hipMemcpy(g, init.data(), n_ints * sizeof(int), hipMemcpyHostToDevice));
  const DecCache kc{e->kv_cache.p, P, g, g + o_keys, g + o_tpos};
  auto step = [&]() -> int {
    int r = run_decoder(e, sl, 1, nullptr, &kc);
    if (r || (r = final_argmax(e, sd, sl, nullptr, n_seq))) return r;
    Bracket br(e, sd, PC_OTHER, 0, 0);
    launch_greedy_advance(sd, sl.d_argmax, g, g + o_pre, g + o_done, g + o_out, sl.idx.d[IX_DEC_IDS], n_seq, dec_len, max_new);
    return RK_OK;
  };
  const std::vector<int> key{GK_T5_GENERATE_STEP, 0, n_seq, (sl.maxL + 63) / 64, dec_len, max_new, e->amax_gen, e->kv_gen};
  // dec_len - 1 forced prefix steps, then one step per new column
  if ((rc = decode_loop(e, sd, key, step, dec_len - 1, 0, max_new, g + 1, 0))) return rc;
  if ((rc = decode_result(e, sd, n_seq, max_new, g + 1, g + o_out, out_tokens, out_steps))) return rc;
  return finish_blocking(e, sl);
}

// Two greedy tokens in ONE decoder pass (the setwise `generation` compare: ref llmrankers/setwise.py:113-121 runs
// generate(max_new_tokens=2) after "<pad> Passage").  The first new token is almost always one of a few label tokens, and a
// decoder pass over a handful of rows costs what its ~270 launches cost, so the second step is computed for EVERY candidate
// at once: the prefix rows of a prompt once, plus one row per candidate at position dec_len that attends to the prefix rows
// and itself (attn_dec_kernel's tree form) and to the prompt (XAttnArgs::row_seq).  The last prefix row gives token 1 over
// the full vocabulary; the row of the candidate that IS token 1 gives token 2.  Rows are independent of the batch they run in (tests), so both tokens are bit-identical to
// rk_t5_greedy(max_new = 2); a first token outside the candidates, or a batch too large for the workspace, takes that path.
int rk_t5_greedy2(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, const int32_t* dec_prefix,
                  int dec_len, const int32_t* cand_ids, int n_cand, int eos_id, int pad_id, int32_t* out_tokens, int32_t* out_steps) {
  if (!e) return RK_ERR_INVALID;
  if (wide_heads(e)) return refuse_wide(e, "rk_t5_greedy2", "greedy decoding runs the decoder self-attention");
  const int Ld = dec_len + 1;
  const long per_seq = (long)dec_len + n_cand;                         // rows of one prompt: the prefix once, one row per candidate
  const long M = (long)n_seq * per_seq, R = (long)n_seq * (1 + n_cand);
  const bool fits = cand_ids && n_cand > 0 && dec_prefix && dec_len > 0 && Ld <= e->d.max_dec_len && R <= e->d.max_seqs &&
                    M <= (long)e->d.max_seqs * e->d.max_dec_len && M <= XA_MAX_ROWS && M <= e->opt.greedy_spec &&
                    use_xattn_direct(e, e->slots[0], Ld);
  if (!fits) return rk_t5_greedy(e, tokens, seq_offsets, n_seq, dec_prefix, dec_len, 2, eos_id, pad_id, out_tokens, out_steps);
  int rc;
  if ((rc = check_ids(e, cand_ids, n_cand, "candidate"))) return rc;
  if ((rc = rk_t5_stage(e, tokens, seq_offsets, n_seq))) return rc;
  Slot& sl = e->slots[0];
  if ((rc = check_ids(e, dec_prefix, dec_len, "decoder"))) return rc;
  if ((rc = ensure_amax(e, (size_t)R))) return rc;
  if ((rc = encoder_then_handoff(e, sl, Ld))) return rc;
  hipStream_t sd = dec_stream(e, sl);
  // row layout of prompt b: [prefix position 0 .. dec_len-1][candidate 0 .. n_cand-1 at position dec_len]
  std::vector<int> ids((size_t)M), rows((size_t)R), rseq((size_t)M), rpos((size_t)M), keys((size_t)M * Ld, 0), amax((size_t)R);
  for (int b = 0; b < n_seq; ++b) {
    const int r0 = (int)(b * per_seq);
    for (int i = 0; i < dec_len; ++i) {
      const int r = r0 + i;
      ids[r] = dec_prefix[i]; rseq[r] = b; rpos[r] = i;
      for (int j = 0; j <= i; ++j) keys[(size_t)r * Ld + j] = r0 + j;
    }
    rows[b] = r0 + dec_len - 1;                                       // token 1: the last prefix row
    for (int c = 0; c < n_cand; ++c) {
      const int r = r0 + dec_len + c;
      ids[r] = cand_ids[c]; rseq[r] = b; rpos[r] = dec_len;
      for (int j = 0; j < dec_len; ++j) keys[(size_t)r * Ld + j] = r0 + j;
      keys[(size_t)r * Ld + dec_len] = r;
      rows[n_seq + b * n_cand + c] = r;                                // token 2 if token 1 was candidate c
    }
  }
  // the five index arrays are the same for every compare of a query (same prefix, candidates and prompt count): uploaded
  // only when they differ from what this path left on the device or something else was written since (DecIndex::tree)
  std::vector<int> sig;
  sig.reserve(ids.size() + rows.size() + rseq.size() + rpos.size() + keys.size() + 2);
  sig.push_back(n_seq); sig.push_back(Ld);
  for (const std::vector<int>* v : {&ids, &rows, &rseq, &rpos, &keys}) sig.insert(sig.end(), v->begin(), v->end());
  if ((rc = sl.idx.tree(e, sd, sig, {{IX_DEC_IDS, ids}, {IX_LAST_ROWS, rows}, {IX_ROW_SEQ, rseq}, {IX_TREE_POS, rpos}, {IX_TREE_KEYS, keys}}))) return rc;
  const DecRows tree{(int)M, sl.idx.d[IX_TREE_KEYS], sl.idx.d[IX_TREE_POS], sl.idx.d[IX_ROW_SEQ]};
  rc = run_graphed(e, sd, {GK_T5_GREEDY2, 0, n_seq, Ld, (sl.maxL + 63) / 64, n_cand, e->amax_gen}, [&]() -> int {
    const int r = run_decoder(e, sl, Ld, &tree);
    return r ? r : final_argmax(e, sd, sl, sl.idx.d[IX_LAST_ROWS], (int)R);
  });
  if (rc || (rc = read_argmax(e, sd, sl, amax.data(), (int)R))) return rc;
  bool all_done = true, miss = false;
  for (int b = 0; b < n_seq; ++b) {
    const int t1 = amax[b];
    out_tokens[b * 2] = t1;
    out_tokens[b * 2 + 1] = pad_id;                                    // finished rows emit pad (hf: generation/utils.py:2927-2929)
    if (t1 == eos_id) continue;
    all_done = false;
    int c = 0;
    while (c < n_cand && cand_ids[c] != t1) ++c;
    if (c == n_cand) miss = true;
    else out_tokens[b * 2 + 1] = amax[n_seq + b * n_cand + c];
  }
  if (miss) {
    // a first token outside the candidates: the ordinary second step (same encoder output, one more decoder pass)
    std::vector<std::vector<int>> seq_rows(n_seq, std::vector<int>(dec_prefix, dec_prefix + dec_len));
    for (int b = 0; b < n_seq; ++b) seq_rows[b].push_back(out_tokens[b * 2]);
    std::vector<int> a2;
    if ((rc = greedy_step(e, sl, seq_rows, Ld, a2))) return rc;
    for (int b = 0; b < n_seq; ++b)
      if (out_tokens[b * 2] != eos_id) out_tokens[b * 2 + 1] = a2[b];
  }
  if ((rc = finish_blocking(e, sl))) return rc;
  if (out_steps) *out_steps = all_done ? 1 : 2;
  return RK_OK;
}

// =============================================== Llama family ================================================
// Decoder-only setwise scoring (ref: llmrankers/setwise.py:60-69, 159-177): prefill of the whole prompt, then the
// arg-max of the last position's logits (generate(max_new_tokens=1, do_sample=False)).  hf: models/llama/modeling_llama.py.
int rk_llama_create(const rk_llama_desc* desc, int device_ordinal, rk_engine** out) {
  if (!desc || !out) return fail(nullptr, RK_ERR_INVALID, "null argument");
  *out = nullptr;
  const rk_llama_desc& l = *desc;
  if (l.head_dim != 64 && l.head_dim != 128)
    return fail(nullptr, RK_ERR_INVALID, "head_dim=%d unsupported: the gfx950 causal attention kernels are built for head_dim=64 and head_dim=128", l.head_dim);
  if (l.n_kv_heads <= 0 || l.n_heads % l.n_kv_heads) return fail(nullptr, RK_ERR_INVALID, "n_heads must be a multiple of n_kv_heads");
  if (l.hidden % 64 || l.intermediate % 64 || l.vocab % 4 || l.hidden > 4096) return fail(nullptr, RK_ERR_INVALID, "hidden / intermediate must be multiples of 64 (hidden <= 4096), vocab of 4");
  if (l.max_tokens <= 0 || l.max_seqs <= 0 || l.n_layers <= 0) return fail(nullptr, RK_ERR_INVALID, "capacities and layer count must be positive");
  rk_model_desc d{};
  d.vocab = l.vocab; d.d_model = l.hidden; d.n_heads = l.n_heads; d.d_kv = 64; d.d_ff = l.intermediate;   // d_kv only passes the T5 checks
  d.n_enc_layers = l.n_layers; d.n_dec_layers = 1; d.n_buckets = 32; d.max_distance = 128; d.gated_gelu = 1; d.tied_head = l.tied_head;
  d.eps = l.eps; d.max_tokens = l.max_tokens; d.max_seqs = l.max_seqs; d.max_dec_len = 1;
  if ((long)d.n_heads * 64 % 64) return fail(nullptr, RK_ERR_INVALID, "bad head count");
  int rc = rk_engine_create(&d, device_ordinal, out);
  if (rc) return rc;
  (*out)->family = 1; (*out)->ld = l; (*out)->inner = l.n_heads * l.head_dim;
  return RK_OK;
}

// The engine's FP8 quantiser (gemm_fp8.h) on a device matrix W [N][K] (row stride ldw): allocates the bytes in device order and the
// exponents (engine-owned) and describes them in *out; q_rm (optional): the bytes row-major [N][K]; deq (optional, may be W): the
// dequantised fp16 matrix, row stride ldw.
static int quant_fp8(rk_engine* e, hipStream_t st, const half_t* W, int N, int K, int ldw, GemmW8* out, uint8_t* q_rm, half_t* deq) {
  if (N <= 0 || K <= 0 || K % 16 || ldw < K || ldw % 8 || (double)N * fp8_ldq(K) >= 4294967296.0)
    return fail(e, RK_ERR_INVALID, "FP8 quantiser: K %% 16, ldw >= K, ldw %% 8, N * K below 4 Gi (got N=%d K=%d ldw=%d)", N, K, ldw);
  uint8_t* q = nullptr; int8_t* ex = nullptr;
  const int ldq = fp8_ldq(K), lde = fp8_lde(K);
  int rc = RK_OK;
  RC(dalloc(e, &q, (size_t)N * ldq)); RC(dalloc(e, &ex, (size_t)N * lde));
  HIPCHK(e, hipMemsetAsync(q, 0, (size_t)N * ldq, st)); HIPCHK(e, hipMemsetAsync(ex, 0, (size_t)N * lde, st));
  hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3((unsigned)((fp8_groups(K) + 3) / 4) * (unsigned)N), dim3(256), 0, st, QuantFp8Args{W, ldw, N, K, q, ldq, ex, lde, q_rm, deq, ldw});
  HIPCHK(e, hipGetLastError());
  *out = GemmW8{q, ex, ldq, lde};
  return RK_OK;
}

static int llama_finalize(rk_engine* e) {
  const rk_llama_desc& l = e->ld;
  const int hd = l.head_dim, dm = l.hidden, Q = l.n_heads * hd, KV = l.n_kv_heads * hd, F = l.intermediate, V = l.vocab;
  // Qwen3's q / k head norm has kernels at width 128 without a bias and without a window: what every Qwen3 checkpoint is
  if (e->qk_norm && (hd != 128 || e->window > 0 || e->qkv_bias))
    return fail(e, RK_ERR_STATE, "the q / k head norm (rk_llama_set_qk_norm) is built for head_dim 128 without a sliding window and without q / k / v biases (got head_dim %d, window %d, biases %d): no Qwen3 checkpoint has another shape", hd, e->window, (int)e->qkv_bias);
  if (e->qk_norm && !(l.eps > 0.f)) return fail(e, RK_ERR_INVALID, "the q / k head norm needs rms_norm_eps > 0 (got %g)", (double)l.eps);
  if (e->kv_fp8 && hd != 128)
    return fail(e, RK_ERR_STATE, "the FP8 K / V cache (rk_llama_set_kv_fp8) is built for head_dim 128 (got %d): the 64-wide models' caches are small, and no 64-wide FP8 kernels are built", hd);
  std::string missing;
  auto N2 = [&](const std::string& n, int64_t r, int64_t c) { return need(e, n, r, c, &missing); };
  auto N1 = [&](const std::string& n, int64_t r) { return need(e, n, r, -1, &missing); };
  N2("model.embed_tokens.weight", V, dm);
  if (!l.tied_head) N2("lm_head.weight", V, dm);
  N1("model.norm.weight", dm);
  for (int i = 0; i < l.n_layers; ++i) {
    const std::string p = "model.layers." + std::to_string(i);
    N2(p + ".self_attn.q_proj.weight", Q, dm); N2(p + ".self_attn.k_proj.weight", KV, dm); N2(p + ".self_attn.v_proj.weight", KV, dm);
    N2(p + ".self_attn.o_proj.weight", dm, Q);
    N2(p + ".mlp.gate_proj.weight", F, dm); N2(p + ".mlp.up_proj.weight", F, dm); N2(p + ".mlp.down_proj.weight", dm, F);
    N1(p + ".input_layernorm.weight", dm); N1(p + ".post_attention_layernorm.weight", dm);
    if (e->qkv_bias) { N1(p + ".self_attn.q_proj.bias", Q); N1(p + ".self_attn.k_proj.bias", KV); N1(p + ".self_attn.v_proj.bias", KV); }
    if (e->qk_norm) { N1(p + ".self_attn.q_norm.weight", hd); N1(p + ".self_attn.k_norm.weight", hd); }
  }
  if (!missing.empty()) return fail(e, RK_ERR_MISSING, "missing or mis-shaped tensors: %s", missing.c_str());
  auto H = [&](const std::string& n) -> const std::vector<half_t>& { return e->host[n].h; };
  auto Fv = [&](const std::string& n) -> const std::vector<float>& { return e->host[n].f; };
  int rc = RK_OK;
  RC(upload(e, &e->emb, H("model.embed_tokens.weight").data(), H("model.embed_tokens.weight").size()));
  if (l.tied_head) e->lm_head = e->emb; else RC(upload(e, &e->lm_head, H("lm_head.weight").data(), H("lm_head.weight").size()));
  RC(upload(e, &e->l_final_ln, Fv("model.norm.weight").data(), (size_t)dm));
  e->ll.resize(l.n_layers);
  std::vector<half_t> buf;
  for (int i = 0; i < l.n_layers; ++i) {
    const std::string p = "model.layers." + std::to_string(i);
    LlamaLayerW& w = e->ll[i];
    {   // q | k | v rows with the input RMSNorm weight folded into the columns
      const auto& ln = Fv(p + ".input_layernorm.weight");
      buf.resize((size_t)(Q + 2 * KV) * dm);
      size_t r0 = 0;
      for (const char* m : {"q_proj", "k_proj", "v_proj"}) {
        const auto& src = H(p + ".self_attn." + m + ".weight");
        const size_t rows = src.size() / dm;
        for (size_t r = 0; r < rows; ++r)
          for (int k = 0; k < dm; ++k) buf[(r0 + r) * dm + k] = (half_t)((float)src[r * dm + k] * ln[k]);
        r0 += rows;
      }
      RC(upload(e, &w.qkv_f, buf.data(), buf.size()));
    }
    if (e->qkv_bias) {   // q | k | v bias, fp32, as it is: it is added AFTER the folded norm's row factor, so no norm weight enters
      std::vector<float> bias;
      for (const char* m : {"q_proj", "k_proj", "v_proj"}) {
        const auto& src = Fv(p + ".self_attn." + m + ".bias");
        bias.insert(bias.end(), src.begin(), src.end());
      }
      RC(upload(e, &w.qkv_bias, bias.data(), bias.size()));
    }
    if (e->qk_norm) {    // q | k head-norm weights, fp32 as they are (the kernels multiply in fp32, one fp16 rounding behind the rotation)
      std::vector<float> nw(Fv(p + ".self_attn.q_norm.weight"));
      const auto& kn = Fv(p + ".self_attn.k_norm.weight");
      nw.insert(nw.end(), kn.begin(), kn.end());
      RC(upload(e, &w.qk_norm, nw.data(), nw.size()));
    }
    RC(upload(e, &w.o, H(p + ".self_attn.o_proj.weight").data(), (size_t)dm * Q));
    {   // gate | up interleaved in groups of 32 rows (the SwiGLU epilogue pairs them in one lane), post-attention norm folded
      const auto& ln = Fv(p + ".post_attention_layernorm.weight");
      const auto& g = H(p + ".mlp.gate_proj.weight"); const auto& u = H(p + ".mlp.up_proj.weight");
      buf.resize((size_t)2 * F * dm);
      for (int blk = 0; blk < F / 32; ++blk)
        for (int r = 0; r < 32; ++r)
          for (int k = 0; k < dm; ++k) {
            buf[((size_t)blk * 64 + r) * dm + k] = (half_t)((float)g[((size_t)blk * 32 + r) * dm + k] * ln[k]);
            buf[((size_t)blk * 64 + 32 + r) * dm + k] = (half_t)((float)u[((size_t)blk * 32 + r) * dm + k] * ln[k]);
          }
      RC(upload(e, &w.gu_f, buf.data(), buf.size()));
    }
    RC(upload(e, &w.down, H(p + ".mlp.down_proj.weight").data(), (size_t)dm * F));
    if (e->weight_fp8) {
      // FP8 step weights: bytes and exponents kept, the fp16 matrix overwritten with the dequantised values - prefill, the heads,
      // the session admit and the step (either kernel) then run ONE model
      hipStream_t st = e->slots[0].se;
      RC(quant_fp8(e, st, w.qkv_f, Q + 2 * KV, dm, dm, &w.qkv8, nullptr, w.qkv_f)); RC(quant_fp8(e, st, w.o, dm, Q, Q, &w.o8, nullptr, w.o));
      RC(quant_fp8(e, st, w.gu_f, 2 * F, dm, dm, &w.gu8, nullptr, w.gu_f)); RC(quant_fp8(e, st, w.down, dm, F, F, &w.down8, nullptr, w.down));
    }
  }
  e->host.clear();
  {   // rotary tables [max_tokens][hd / 2], float32 like hf: modeling_llama.py:94-127: freq_i = theta^(-2i/hd), then the llama3 rope type's
      // wavelength-dependent scaling (hf: modeling_rope_utils.py _compute_llama3_parameters) when it was asked for
    const size_t Tc = l.max_tokens;
    const size_t hh = (size_t)hd / 2;
    std::vector<float> c(Tc * hh), sn(Tc * hh);
    for (int i = 0; i < (int)hh; ++i) {
      float inv = 1.0f / powf(l.rope_theta, (float)(2 * i) / (float)hd);
      if (e->rope_factor > 0.f) {
        const float orig = (float)e->rope_orig, wavelen = 6.283185307179586f / inv;
        const float scaled = wavelen > orig / e->rope_low ? inv / e->rope_factor : inv;
        const float smooth = (orig / wavelen - e->rope_low) / (e->rope_high - e->rope_low);
        const bool medium = !(wavelen < orig / e->rope_high) && !(wavelen > orig / e->rope_low);
        inv = medium ? (1.0f - smooth) * scaled / e->rope_factor + smooth * scaled : scaled;
      }
      for (size_t t = 0; t < Tc; ++t) { const float a = (float)t * inv; c[t * hh + i] = cosf(a); sn[t * hh + i] = sinf(a); }
    }
    RC(upload(e, &e->rope_cos, c.data(), c.size())); RC(upload(e, &e->rope_sin, sn.data(), sn.size()));
  }
  const size_t Tc = l.max_tokens, Bc = l.max_seqs;
  Slot& sl = e->slots[0];
  RC(dalloc(e, &sl.enc.hidden, Tc * dm)); RC(dalloc(e, &sl.enc.xraw[0], Tc * dm)); RC(dalloc(e, &sl.enc.ssq[0], Tc * ((dm + 63) / 64)));
  RC(dalloc(e, &sl.enc.factors, Tc + 512)); HIPCHK(e, hipMemset(sl.enc.factors, 0, (Tc + 512) * sizeof(float)));
  RC(dalloc(e, &sl.qkv, Tc * (Q + 2 * KV))); RC(dalloc(e, &sl.ctx, Tc * Q)); RC(dalloc(e, &sl.ffh, Tc * F));
  RC(dalloc(e, &sl.d_tokens, Tc)); RC(dalloc(e, &e->d_pos, Tc)); RC(dalloc(e, &sl.d_seq_off, Bc + 1));
  RC(dalloc(e, &sl.idx.d[IX_LAST_ROWS], Bc)); RC(dalloc(e, &sl.idx.d[IX_OUT_IDS], 8192)); RC(dalloc(e, &sl.d_argmax, Bc)); RC(dalloc(e, &sl.dlast, Bc * dm));
  e->scores_cap = Bc * 64;
  RC(dalloc(e, &sl.d_scores, e->scores_cap));
  HIPCHK(e, hipHostMalloc((void**)&sl.h_scores, e->scores_cap * sizeof(float), hipHostMallocDefault));
  HIPCHK(e, hipHostMalloc((void**)&sl.idx.pin, IX_N_CACHED * DecIndex::PIN_INTS * sizeof(int), hipHostMallocDefault));
  HIPCHK(e, hipDeviceSynchronize());
  e->finalized = true;
  return RK_OK;
}

// prefill of the ragged batch; leaves the final-normed LAST hidden state of every sequence in sl.dlast [n_seq, hidden]
// keep (rk_llama_generate only): every layer's rotated K and its V are also copied to the cache, P positions per sequence
// slots (rk_llama_session_admit): sequence b goes to cache row slots[b] (device ints) of a cache of `rows` rows
struct LlamaKeep { half_t* kv; int P; const int* slots = nullptr; int rows = 0; };
// One layer's K / V cache inside lkv, for `rows` cache rows of P positions, in the engine's shape: kv_layout.h's layout.
static KvLayerLayout llama_kv_layout(const rk_engine* e, int kv8, int rows, int P) {
  return kv_layer_layout(kv8, rows, e->ld.n_kv_heads, e->ld.head_dim, P);
}
static size_t llama_kv_layer_halfs(const rk_engine* e, int kv8, int rows, int P) { return llama_kv_layout(e, kv8, rows, P).bytes / 2; }
static Kv8Cache llama_kv_layer(const rk_engine* e, half_t* base, int kv8, int layer, int rows, int P) {
  return kv_cache_layer(llama_kv_layout(e, kv8, rows, P), base, layer);
}
static int llama_prefill(rk_engine* e, const int32_t* tokens, const int32_t* off, int n_seq, const LlamaKeep* keep = nullptr) {
  if (!e || e->family != 1) return fail(e, RK_ERR_STATE, "not a Llama engine");
  int rc = set_device(e);
  if (rc) return rc;
  Slot& sl = e->slots[0];
  if ((rc = check_batch(e, &sl, tokens, off, n_seq))) return rc;
  const rk_llama_desc& l = e->ld;
  const int hd = l.head_dim, T = sl.T, dm = l.hidden, Q = l.n_heads * hd, KV = l.n_kv_heads * hd, F = l.intermediate, ldq = Q + 2 * KV;
  const CausalAttnPlan ap = plan_llama_attn(e, n_seq, sl.maxL, l.n_heads, l.n_kv_heads);
  if (!causal_attn_exists(ap)) return refuse_window(e, "llama prefill", sl.maxL);
  hipStream_t st = sl.se;
  HIPCHK(e, hipStreamSynchronize(st));
  std::vector<int> pos(T), last(n_seq);
  for (int b = 0; b < n_seq; ++b) {
    for (int t = off[b]; t < off[b + 1]; ++t) pos[t] = t - off[b];
    last[b] = off[b + 1] - 1;
  }
  HIPCHK(e, hipMemcpy(sl.d_tokens, tokens, (size_t)T * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(e->d_pos, pos.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.d_seq_off, off, (size_t)(n_seq + 1) * sizeof(int), hipMemcpyHostToDevice));
  RC(sl.idx.write(e, st, {{IX_LAST_ROWS, last}}));
  // every consumer takes its row factors from rowscale_kernel (own_factors = false), also where a fill-in tile variant could
  // form them itself
  NormStream ns = sl.enc;
  ns.begin(e, st, sl.d_tokens, T, true);
  for (int i = 0; i < l.n_layers; ++i) {
    const LlamaLayerW& w = e->ll[i];
    RC(gemm(e, st, ns.consumer(e, st, nullptr, Gemm(PC_ENC_GEMM_QKV, EPI_STORE_F16, ns.x(), dm, w.qkv_f, dm, sl.qkv, ldq, T, ldq, dm), false)));
    {
      Bracket br(e, st, PC_OTHER, 0, (double)T * (Q + KV) * 4.0);
      launch_rope(st, hd, sl.qkv, e->d_pos, e->rope_cos, e->rope_sin, ldq, l.n_heads + l.n_kv_heads, w.qkv_bias, l.n_kv_heads, T, w.qk_norm, l.eps);
    }
    if (keep) {
      const int kv8 = kv8_mode(e);
      const Kv8Cache cc = llama_kv_layer(e, keep->kv, kv8, i, keep->slots ? keep->rows : n_seq, keep->P);
      Bracket br(e, st, PC_OTHER, 0, (double)T * KV * 8.0);
      launch_kv_fill(st, hd, sl.qkv, sl.d_seq_off, keep->slots, keep->rows, cc, ldq, l.n_heads, l.n_kv_heads, keep->P, sl.maxL, n_seq, kv8);
    }
    launch_llama_attn(e, st, CausalAttnCall{sl.qkv, sl.ctx, sl.d_seq_off, ldq, Q, l.n_heads, l.n_kv_heads, sl.n_seq, sl.maxL, T}, ap);
    RC(ns.producer(e, st, Gemm(PC_ENC_GEMM_O, EPI_RESID_F32, sl.ctx, Q, w.o, Q, ns.hidden, dm, T, dm, Q)));
    RC(gemm(e, st, ns.consumer(e, st, nullptr, Gemm(PC_ENC_GEMM_FFN_IN, EPI_SWIGLU_F16, ns.x(), dm, w.gu_f, dm, sl.ffh, F, T, 2 * F, dm), false)));
    RC(ns.producer(e, st, Gemm(PC_ENC_GEMM_FFN_OUT, EPI_RESID_F32, sl.ffh, F, w.down, F, ns.hidden, dm, T, dm, F), i + 1 < l.n_layers));
  }
  rmsnorm(e, st, ns.hidden, e->l_final_ln, sl.dlast, sl.idx.d[IX_LAST_ROWS], n_seq);
  HIPCHK(e, hipGetLastError());
  return RK_OK;
}

int rk_llama_last_logits(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                         const int32_t* out_token_ids, int n_out, float* out_logits) {
  if (!e || !out_logits) return RK_ERR_INVALID;
  if (e->ls.open) return fail(e, RK_ERR_STATE, "rk_llama_last_logits while a decoding session is open (it shares the prefill's buffers): rk_llama_session_close first");
  if (!out_token_ids || n_out <= 0 || n_out > 64) return fail(e, RK_ERR_INVALID, "n_out must be in 1..64 (got %d)", n_out);
  int rc = check_ids(e, out_token_ids, n_out, "output");
  if (rc) return rc;
  if ((rc = llama_prefill(e, tokens, seq_offsets, n_seq))) return rc;
  Slot& sl = e->slots[0];
  hipStream_t st = sl.se;
  HIPCHK(e, hipMemcpyAsync(sl.idx.d[IX_OUT_IDS], out_token_ids, n_out * sizeof(int), hipMemcpyHostToDevice, st));
  launch_head_rows(st, sl.dlast, e->lm_head, sl.idx.d[IX_OUT_IDS], sl.d_scores, n_seq, n_out, e->ld.hidden);
  return read_scores_blocking(e, sl, st, (size_t)n_seq * n_out, out_logits);
}

// rk_llama_qlm's device memory, grown between calls only: the head's block statistics and label logits (ensure_logits: the buffer
// the sampling head shares, logits_gen counts its moves), the normed label rows, and - once, at the prefill's capacities: a label
// row is a prompt row, so there are fewer than max_tokens of them - the three int buffers of DecIndex.
static int ensure_llama_qlm(rk_engine* e, size_t rows) {
  Slot& sl = e->slots[0];
  int rc = RK_OK;
  if (!sl.idx.d[IX_ROW_MAP]) {
    RC(dalloc(e, &sl.idx.d[IX_ROW_MAP], (size_t)e->ld.max_tokens)); RC(dalloc(e, &sl.idx.d[IX_ROW_LABEL], (size_t)e->ld.max_tokens));
    RC(dalloc(e, &sl.idx.d[IX_ROW_OFF], (size_t)e->ld.max_seqs + 1));
  }
  RC(ensure_logits(e, rows));
  return e->lqlm_x.reserve(e, rows * (size_t)e->ld.hidden);
}

// Query likelihood on a decoder-only model: out_scores[b] = sum over the last n_labels[b] tokens of sequence b of
// log softmax(z[t - 1])[tok[t]] (hf: modeling_llama.py LlamaForCausalLM.forward -> ForCausalLMLoss with labels = -100 on the
// prompt, reduction "none", summed and negated: the decoder-only counterpart of ref: llmrankers/pointwise.py:73-79, which the
// reference has for T5 only).  llama_prefill as every other entry point runs it, then rk_t5_qlm's tail on the rows that predict a
// label: the final norm gathered through IX_ROW_MAP, the head GEMM with the log-sum-exp in its epilogue (the tiled family whatever
// the row count; every tile shape writes the same block statistics), qlm_lse_kernel in its ragged form.  A sequence's score is a
// function of its own tokens and label count, whatever shares the call.
int rk_llama_qlm(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, const int32_t* n_labels, float* out_scores) {
  if (!e) return RK_ERR_INVALID;
  if (!tokens || !seq_offsets || !n_labels || !out_scores) return fail(e, RK_ERR_INVALID, "rk_llama_qlm: tokens, seq_offsets, n_labels or out_scores missing");
  if (e->family != 1) return fail(e, RK_ERR_STATE, "rk_llama_qlm on a T5 engine (rk_t5_qlm)");
  if (e->ls.open) return fail(e, RK_ERR_STATE, "rk_llama_qlm while a decoding session is open (it shares the prefill's buffers): rk_llama_session_close first");
  int rc = check_batch(e, nullptr, tokens, seq_offsets, n_seq);   // before the label counts are held against the lengths
  if (rc) return rc;
  std::vector<int> row_map, row_label, row_off((size_t)n_seq + 1, 0);
  for (int b = 0; b < n_seq; ++b) {
    const int L = seq_offsets[b + 1] - seq_offsets[b], nl = n_labels[b];
    if (nl < 1 || nl >= L) return fail(e, RK_ERR_INVALID, "sequence %d: n_labels %d outside 1..%d (its %d tokens are a prompt of at least one token, then the labels)", b, nl, L - 1, L);
    for (int t = seq_offsets[b + 1] - nl; t < seq_offsets[b + 1]; ++t) { row_map.push_back(t - 1); row_label.push_back(tokens[t]); }
    row_off[b + 1] = (int)row_map.size();
  }
  const int rows = (int)row_map.size();
  if ((rc = set_device(e))) return rc;
  Slot& sl = e->slots[0];
  hipStream_t st = sl.se;
  RC(ensure_llama_qlm(e, (size_t)rows));
  RC(sl.idx.write(e, st, {{IX_ROW_MAP, row_map}, {IX_ROW_LABEL, row_label}, {IX_ROW_OFF, row_off}}));
  RC(llama_prefill(e, tokens, seq_offsets, n_seq));
  int* const* ix = sl.idx.d;
  const int nblk = (e->ld.vocab + 31) / 32, dm = e->ld.hidden;
  rmsnorm(e, st, sl.enc.hidden, e->l_final_ln, e->lqlm_x.p, ix[IX_ROW_MAP], rows);
  float* xlab = e->logits.p + (size_t)rows * nblk * 2;
  RC(gemm(e, st, Gemm(PC_HEAD, EPI_LSE_F32, e->lqlm_x.p, dm, e->lm_head, dm, e->logits.p, nblk, rows, e->ld.vocab, dm).lse(ix[IX_ROW_LABEL], xlab)));
  launch_qlm_lse(st, (const float2*)e->logits.p, nblk, xlab, 0, ix[IX_ROW_OFF], nullptr, sl.d_scores, n_seq);
  return read_scores_blocking(e, sl, st, (size_t)n_seq, out_scores);
}

int rk_llama_set_rope_scaling(rk_engine* e, float factor, float low_freq_factor, float high_freq_factor, int original_max_pos) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "rope scaling applies to Llama engines (rk_llama_create)");
  if (e->finalized) return fail(e, RK_ERR_STATE, "rk_llama_set_rope_scaling must precede rk_engine_finalize (the rotary tables are built there)");
  if (!(factor > 0.f) || !(high_freq_factor > low_freq_factor) || !(low_freq_factor > 0.f) || original_max_pos <= 0)
    return fail(e, RK_ERR_INVALID, "bad llama3 rope scaling (factor %g, low %g, high %g, original_max_position_embeddings %d)", factor, low_freq_factor, high_freq_factor, original_max_pos);
  e->rope_factor = factor; e->rope_low = low_freq_factor; e->rope_high = high_freq_factor; e->rope_orig = original_max_pos;
  return RK_OK;
}

int rk_llama_set_sliding_window(rk_engine* e, int window) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "a sliding window applies to Llama-family engines (rk_llama_create)");
  if (e->finalized) return fail(e, RK_ERR_STATE, "rk_llama_set_sliding_window must precede rk_engine_finalize");
  if (window < 0) return fail(e, RK_ERR_INVALID, "sliding window %d: a positive number of positions, or 0 for none", window);
  e->window = window;
  return RK_OK;
}

int rk_llama_set_qkv_bias(rk_engine* e, int on) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "q / k / v projection biases apply to Llama-family engines (rk_llama_create)");
  if (e->finalized) return fail(e, RK_ERR_STATE, "rk_llama_set_qkv_bias must precede rk_engine_finalize (the bias vectors are uploaded there)");
  e->qkv_bias = on != 0;
  return RK_OK;
}

int rk_llama_set_qk_norm(rk_engine* e, int on) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "the q / k head norm applies to Llama-family engines (rk_llama_create)");
  if (e->finalized) return fail(e, RK_ERR_STATE, "rk_llama_set_qk_norm must precede rk_engine_finalize (the norm weights are uploaded there)");
  e->qk_norm = on != 0;
  return RK_OK;
}

int rk_llama_set_weight_fp8(rk_engine* e, int on) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "FP8 step weights apply to Llama-family engines (rk_llama_create)");
  if (e->finalized) return fail(e, RK_ERR_STATE, "rk_llama_set_weight_fp8 must precede rk_engine_finalize (the matrices are quantised there)");
  e->weight_fp8 = on != 0;
  return RK_OK;
}

int rk_llama_set_kv_fp8(rk_engine* e, int on) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "the FP8 K / V cache applies to Llama-family engines (rk_llama_create)");
  if (e->finalized) return fail(e, RK_ERR_STATE, "rk_llama_set_kv_fp8 must precede rk_engine_finalize (the head width is checked there)");
  e->kv_fp8 = on != 0;
  return RK_OK;
}

int rk_llama_greedy1(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, int32_t* out_tokens) {
  if (!e || !out_tokens) return RK_ERR_INVALID;
  if (e->ls.open) return fail(e, RK_ERR_STATE, "rk_llama_greedy1 while a decoding session is open (it shares the prefill's buffers): rk_llama_session_close first");
  int rc = llama_prefill(e, tokens, seq_offsets, n_seq);
  if (rc) return rc;
  if ((rc = ensure_amax(e, (size_t)n_seq))) return rc;
  Slot& sl = e->slots[0];
  hipStream_t st = sl.se;
  // full-vocabulary head on the n_seq last rows: weight-streaming GEMM, then the first arg-max (torch.argmax tie rule)
  if ((rc = head_argmax(e, st, sl.dlast, n_seq, e->ld.hidden, e->ld.vocab, sl.d_argmax))) return rc;
  return read_argmax(e, st, sl, out_tokens, n_seq);
}

// rk_llama_generate's device memory, grown between calls only (never inside a capture; a move of any of the three changes
// lkv_gen, which is part of the step graph's key: the step holds all three addresses): the K / V cache, the attention partials,
// the call's int block (`ints` of them); once: the step's activation rows.  A decoding session (below) holds the same three.
// step_rows (a drafting session: n_seq * g1 step rows over n_seq cache rows): the rows the partials are sized for, 0 = n_seq
static int ensure_llama_gen(rk_engine* e, int n_seq, int P, size_t ints, int step_rows = 0) {
  const rk_llama_desc& l = e->ld;
  const size_t S = (size_t)l.max_seqs, dm = l.hidden, Q = (size_t)l.n_heads * l.head_dim, KV = (size_t)l.n_kv_heads * l.head_dim, F = l.intermediate;
  const size_t kv = (size_t)l.n_layers * llama_kv_layer_halfs(e, kv8_mode(e), n_seq, P);   // (fp16: n_layers * 2 * n_seq * KV * P)
  const size_t part = (size_t)std::max(n_seq, step_rows) * l.n_heads * ((P + LDC_CHUNK - 1) / LDC_CHUNK) * ldc_pstr(l.head_dim);
  int rc = RK_OK;
  RC(e->lkv.reserve(e, kv, &e->lkv_gen)); RC(e->lpart.reserve(e, part, &e->lkv_gen)); RC(e->lints.reserve(e, ints, &e->lkv_gen));
  if (!e->lg.stream.hidden) {
    RC(dalloc(e, &e->lg.stream.hidden, S * dm)); RC(dalloc(e, &e->lg.stream.xraw[0], S * dm)); RC(dalloc(e, &e->lg.qkv, S * (Q + 2 * KV)));
    RC(dalloc(e, &e->lg.ctx, S * Q)); RC(dalloc(e, &e->lg.ffh, S * F)); RC(dalloc(e, &e->lg.stream.ssq[0], S * ((dm + 31) / 32)));
    RC(dalloc(e, &e->lg.stream.factors, S));
  }
  return ensure_decode_ring(e);
}

// One decoding step over `rows` cache rows of P positions each (rk_llama_generate's rows, a session's slots), up to the final
// norm: the embedding of next[rows], per layer QKV (folded norm) -> attn_dec_cached_kernel at pos[rows] -> o + residual ->
// gate|up + SwiGLU -> down + residual, then the final-normed rows in slots[0].dlast.  The cache, the partials and the activation
// rows are the engine's (ensure_llama_gen).  Nothing here depends on which rows are live: a row's bits follow from its own
// tokens and position.
// g1 > 1 (a drafting session): `rows` = cache rows * g1 step rows, g1 consecutive ones per cache row; live[rows] says whose key
// and value go to the cache (kv_cache_append_kernel), and the attention reads every key from there (launch_llama_dec_attn).
static int llama_step_rows(rk_engine* e, hipStream_t st, int rows, int P, const int* d_next, const int* d_pos, int g1 = 1,
                           const int* d_live = nullptr) {
  const rk_llama_desc& l = e->ld;
  const int dm = l.hidden, Q = l.n_heads * l.head_dim, KV = l.n_kv_heads * l.head_dim, F = l.intermediate, ldq = Q + 2 * KV;
  const LlamaDecAttnPlan ap = plan_llama_dec_attn(e, rows, P, l.n_heads, l.n_kv_heads);
  const float scale_log2e = (1.0f / std::sqrt((float)l.head_dim)) * 1.4426950408889634f;
  const auto& lg = e->lg;
  int rc = RK_OK;
  NormStream ns = lg.stream;
  // the GEMM behind a norm forms its row factors from the producer's block sums in its own epilogue, or - more block sums than
  // that path stages by DMA (64: hidden > 2 048) - takes them from rowscale_kernel in front of it.  A function of the model only.
  auto normed = [&](Gemm c) { return ns.consumer(e, st, nullptr, c.on(GEMM_STREAM), ns.nb <= 64); };
  // FP8 engines: the four projections read the FP8 bytes - by the engine's mode, never by the row count (same bits either way)
  const bool f8 = e->weight_fp8 && e->opt.llama_step_fp8;
  auto b8 = [&](const GemmW8& w8) { return f8 ? w8 : GemmW8{nullptr, nullptr, 0, 0}; };
  ns.begin(e, st, d_next, rows, true);
  for (int i = 0; i < l.n_layers; ++i) {
    const LlamaLayerW& w = e->ll[i];
    RC(gemm(e, st, normed(Gemm(PC_DEC_GEMM, EPI_STORE_F16, ns.x(), dm, w.qkv_f, dm, lg.qkv, ldq, rows, ldq, dm).w8(b8(w.qkv8)))));
    const Kv8Cache cc = llama_kv_layer(e, e->lkv.p, ap.kv8, i, rows / g1, P);
    const LlamaDecAttnArgs aa{lg.qkv, nullptr, nullptr /* kc, vc: cc's, in the launch */, d_pos, e->rope_cos, e->rope_sin, e->lpart.p, lg.ctx,
                              ldq, l.n_heads, l.n_kv_heads, P, ap.nch, scale_log2e, w.qkv_bias, 0, w.qk_norm, l.eps};
    launch_llama_dec_attn(e, st, ap, aa, rows, g1, d_live, cc);
    RC(ns.producer(e, st, Gemm(PC_DEC_GEMM, EPI_RESID_F32, lg.ctx, Q, w.o, Q, ns.hidden, dm, rows, dm, Q).on(GEMM_STREAM).w8(b8(w.o8))));
    RC(gemm(e, st, normed(Gemm(PC_DEC_GEMM, EPI_SWIGLU_F16, ns.x(), dm, w.gu_f, dm, lg.ffh, F, rows, 2 * F, dm).w8(b8(w.gu8)))));
    RC(ns.producer(e, st, Gemm(PC_DEC_GEMM, EPI_RESID_F32, lg.ffh, F, w.down, F, ns.hidden, dm, rows, dm, F).on(GEMM_STREAM).w8(b8(w.down8)), i + 1 < l.n_layers));
  }
  rmsnorm(e, st, ns.hidden, e->l_final_ln, e->slots[0].dlast, nullptr, rows);
  return RK_OK;
}

// The head behind a Llama prefill or step: `rows` final-normed rows of slots[0].dlast -> one token each in slots[0].d_argmax, by
// arg-max, or drawn (head_sample's seed_map, pos and pos_map).  What a call or a session takes was decided before its chain started.
struct HeadHow { bool sample = false; const int *seed_map = nullptr, *pos = nullptr, *pos_map = nullptr; };
static int llama_head(rk_engine* e, hipStream_t st, int rows, const HeadHow& how) {
  Slot& sl = e->slots[0];
  return how.sample ? head_sample(e, st, sl.dlast, rows, e->ld.hidden, e->ld.vocab, e->samp, how.seed_map, how.pos, how.pos_map, sl.d_argmax)
                    : head_argmax(e, st, sl.dlast, rows, e->ld.hidden, e->ld.vocab, sl.d_argmax);
}
// the key of a step graph: everything its launch arguments depend on - the kind of chain, its rows, the cache's P, a session's cap,
// the generation of the head's buffers and of the cache's, a drafting session's Kd
static std::vector<int> llama_step_key(const rk_engine* e, bool session, int rows, int P, int cap, bool sampled, int draft) {
  const int kind = session ? (draft ? GK_LLAMA_SESSION_STEP_DRAFT : sampled ? GK_LLAMA_SESSION_STEP_SAMPLED : GK_LLAMA_SESSION_STEP)
                           : (sampled ? GK_LLAMA_STEP_SAMPLED : GK_LLAMA_STEP);
  std::vector<int> key{kind, 0, rows, P, cap, sampled ? e->logits_gen : e->amax_gen, e->lkv_gen, draft};
  if (!draft) key.pop_back();                              // (Kd stands in a drafting session's key only, cap in a session's only)
  if (!session) key.erase(key.begin() + 4);
  if (e->kv_fp8) key.push_back(kv8_mode(e));               // an FP8-cache engine: which cache layout the step's kernels address
  return key;
}
// the stop ids of rk_llama_generate and of a session: at most INTS_MAX_EOS EOS ids and the pad id, all inside the vocabulary
static int check_stop_ids(rk_engine* e, const int32_t* eos_ids, int n_eos, int pad_id) {
  if (n_eos < 0 || n_eos > INTS_MAX_EOS || (n_eos > 0 && !eos_ids)) return fail(e, RK_ERR_INVALID, "n_eos must be in 0..8 (got %d)", n_eos);
  const int rc = check_ids(e, eos_ids, n_eos, "eos");
  return rc ? rc : check_ids(e, &pad_id, 1, "pad");
}

// Greedy continuation with a K / V cache (hf: generation/utils.py greedy loop over LlamaForCausalLM with use_cache): the prefill
// once, keeping every layer's rotated K and its V; column 0 = the prefill's arg-max (rk_llama_greedy1's token); then ONE new row
// per sequence and step: embedding of the fed-back token, per layer QKV (folded norm) -> attn_dec_cached_kernel -> o + residual
// -> gate|up + SwiGLU -> down + residual, final norm, arg-max head, llama_advance_kernel.  Every projection runs on the
// weight-streaming family (the caller's regime, never the row count: a row's tokens do not depend on what shares the call).  The
// step is one graph per (rows, P, cache generation), replayed; position, finished rows and next ids live on the device; the host
// reads one word per step and keeps one step queued ahead (rk_t5_generate's loop).
// seeds != null (rk_llama_generate_sampled with sampling on): head_sample in head_argmax's place, in the prefill's head and in the
// step - a graph of its own kind, keyed by logits_gen too.  Everything else is the greedy call's.
static int llama_generate(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, int max_new, int max_total,
                          const int32_t* eos_ids, int n_eos, int pad_id, int32_t* out_tokens, int32_t* out_steps, const uint64_t* seeds) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "rk_llama_generate called on a T5 engine (use rk_t5_generate)");
  if (e->ls.open) return fail(e, RK_ERR_STATE, "rk_llama_generate while a decoding session is open (it shares the cache and the step's rows): rk_llama_session_close first");
  if (!out_tokens) return fail(e, RK_ERR_INVALID, "null output");
  if (max_new <= 0) return fail(e, RK_ERR_INVALID, "max_new must be positive (got %d)", max_new);
  int rc;
  if ((rc = check_stop_ids(e, eos_ids, n_eos, pad_id))) return rc;
  if ((rc = set_device(e))) return rc;
  Slot& sl = e->slots[0];
  if ((rc = check_batch(e, &sl, tokens, seq_offsets, n_seq))) return rc;
  const rk_llama_desc& l = e->ld;
  if ((long)sl.maxL + max_new > l.max_tokens)
    return fail(e, RK_ERR_CAPACITY, "longest prompt %d + max_new %d exceeds max_tokens %d (the rotary tables end there)", sl.maxL, max_new, l.max_tokens);
  for (int b = 0; b < n_seq; ++b)
    if (max_total > 0 && seq_offsets[b + 1] - seq_offsets[b] >= max_total)
      return fail(e, RK_ERR_INVALID, "prompt %d has %d tokens: it already reaches max_total %d", b, seq_offsets[b + 1] - seq_offsets[b], max_total);
  const int P = sl.maxL + max_new;
  const GenLayout lay(l.max_seqs, n_seq, max_new);         // the call's int block (decode_ints.h)
  if ((rc = ensure_amax(e, (size_t)n_seq))) return rc;
  if ((rc = ensure_llama_gen(e, n_seq, P, lay.total))) return rc;
  if (seeds && (rc = ensure_sample_head(e, (size_t)n_seq))) return rc;
  hipStream_t st = sl.se;
  const GenInts d = lay.bind(e->lints.p);
  const std::vector<int> init = lay.initial(seq_offsets, max_total, P, eos_ids, n_eos, pad_id);
  HIPCHK(e, hipStreamSynchronize(st));
  HIPCHK(e, hipMemcpy(d.st, init.data(), init.size() * sizeof(int), hipMemcpyHostToDevice));
  if (seeds) HIPCHK(e, hipMemcpy(e->d_seeds, seeds, (size_t)n_seq * sizeof(uint64_t), hipMemcpyHostToDevice));
  const LlamaKeep keep{e->lkv.p, P};
  if ((rc = llama_prefill(e, tokens, seq_offsets, n_seq, &keep))) return rc;
  // the token index of the row's new token = the position of its last token + 1: the prefill's positions at the last rows for
  // column 0, the advance kernel's pos[] (len + column - 1) for the steps
  const bool sampled = seeds != nullptr;
  auto advance = [&]() { Bracket br(e, st, PC_OTHER, 0, 0); launch_llama_advance(st, sl.d_argmax, d, n_seq); };
  if ((rc = llama_head(e, st, n_seq, HeadHow{sampled, nullptr, e->d_pos, sl.idx.d[IX_LAST_ROWS]}))) return rc;
  advance();
  auto step = [&]() -> int {
    int r = llama_step_rows(e, st, n_seq, P, d.next, d.pos);
    if (r || (r = llama_head(e, st, n_seq, HeadHow{sampled, nullptr, d.pos, nullptr}))) return r;
    advance();
    return RK_OK;
  };
  // column 0 is the prefill's: the steps produce columns 1 .. max_new - 1
  if ((rc = decode_loop(e, st, llama_step_key(e, false, n_seq, P, 0, sampled, 0), step, 0, 1, max_new, d.st + GEN_FINISHED, 0))) return rc;
  return decode_result(e, st, n_seq, max_new, d.st + GEN_FINISHED, d.out, out_tokens, out_steps);
}
int rk_llama_generate(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, int max_new, int max_total,
                      const int32_t* eos_ids, int n_eos, int pad_id, int32_t* out_tokens, int32_t* out_steps) {
  return llama_generate(e, tokens, seq_offsets, n_seq, max_new, max_total, eos_ids, n_eos, pad_id, out_tokens, out_steps, nullptr);
}
int rk_llama_generate_sampled(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, int max_new, int max_total,
                              const int32_t* eos_ids, int n_eos, int pad_id, int32_t* out_tokens, int32_t* out_steps, const uint64_t* seeds) {
  if (!e) return RK_ERR_INVALID;
  if (!seeds) return fail(e, RK_ERR_INVALID, "rk_llama_generate_sampled: null seeds");
  return llama_generate(e, tokens, seq_offsets, n_seq, max_new, max_total, eos_ids, n_eos, pad_id, out_tokens, out_steps,
                        e->family == 1 && e->samp.on() ? seeds : nullptr);
}

// temperature 0 = off.  Like an option: the step graphs hold (T, k, p) as launch arguments, so a new graph epoch starts.
int rk_llama_set_sampling(rk_engine* e, float temperature, int top_k, float top_p) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "rk_llama_set_sampling called on a T5 engine (the T5 rankers decode greedily)");
  if (e->ls.open) return fail(e, RK_ERR_STATE, "rk_llama_set_sampling while a decoding session is open (it latched the parameters at its open): rk_llama_session_close first");
  if (!(temperature >= 0.f) || std::isinf(temperature)) return fail(e, RK_ERR_INVALID, "temperature must be finite and >= 0 (got %g; 0 = greedy)", (double)temperature);
  if (top_k < 0) return fail(e, RK_ERR_INVALID, "top_k must be >= 0 (got %d; 0 = off)", top_k);
  if (!(top_p > 0.f && top_p <= 1.f)) return fail(e, RK_ERR_INVALID, "top_p must be in (0, 1] (got %g; 1 = off)", (double)top_p);
  e->samp.T = temperature; e->samp.k = top_k; e->samp.p = top_p;
  e->opt_epoch++;
  return RK_OK;
}

// ---- decoding session: fixed cache slots, prompts admitted while the other slots keep their state, ONE replayed step graph ----
// What vLLM's continuous batching gives the reference's Rank-R1 ranker (ref: llmrankers/setwise.py:406-553): a finished row's place
// goes to the next request.  The session's rows are rk_llama_generate's rows (llama_step_rows, the same launch sequence over all
// n_slots rows, P = max_len), its prefill is llama_prefill with a slot map, and llama_session_advance_kernel keeps every slot's
// own column counter: a prompt's tokens are bit for bit what rk_llama_generate gives for it alone.
// Its int block is decode_ints.h's SessionLayout (ls.lay).
namespace {
SessionInts session_ints(const rk_engine* e) { return e->ls.lay.bind(e->lints.p); }
int session_check(rk_engine* e, const char* who) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "%s called on a T5 engine", who);
  if (!e->ls.open) return fail(e, RK_ERR_STATE, "%s without an open session (rk_llama_session_open)", who);
  return set_device(e);
}
// the session word, every slot's column counter and done flag -> the host mirror; the stream is idle afterwards
int session_read_back(rk_engine* e, hipStream_t st) {
  auto& ls = e->ls;
  const SessionLayout& lay = ls.lay;
  std::vector<int> buf(lay.done.off + lay.done.n);         // head | len | col | max_new | done
  HIPCHK(e, hipMemcpyAsync(buf.data(), e->lints.p, buf.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(e, hipStreamSynchronize(st));
  HIPCHK(e, hipGetLastError());
  ls.seen = buf[SES_FINISHES];
  for (int b = 0; b < ls.n_slots; ++b) { ls.col[b] = buf[lay.col.off + b]; ls.done[b] = buf[lay.done.off + b]; }
  return RK_OK;
}
// behind a head: the session's state machine over the head's tokens and, for a drafting session, the proposer of the next step's
// rows - as a step, or in the admit form
static void session_advance(rk_engine* e, hipStream_t st, const SessionInts& d, const SessionAdmit& a = {}) {
  const auto& ls = e->ls;
  Bracket br(e, st, PC_OTHER, 0, 0);
  if (!ls.draft) { launch_session_advance(st, e->slots[0].d_argmax, d, ls.n_slots, a); return; }
  launch_session_advance_draft(st, e->slots[0].d_argmax, d, ls.n_slots, ls.draft + 1, a);
  launch_draft_lookup(st, d, ls.n_slots, ls.draft + 1);
}
}  // namespace

// draft = Kd > 0 (rk_llama_session_open_draft): Kd extra rows per slot and step, fed with drafted tokens; see the drafting block below
static int session_open(rk_engine* e, int n_slots, int max_len, int max_new_cap, const int32_t* eos_ids, int n_eos, int pad_id,
                        int draft, int ngram_min, int ngram_max) {
  if (!e) return RK_ERR_INVALID;
  if (e->family != 1) return fail(e, RK_ERR_STATE, "rk_llama_session_open called on a T5 engine");
  if (!e->finalized) return fail(e, RK_ERR_STATE, "engine not finalized");
  if (e->ls.open) return fail(e, RK_ERR_STATE, "a decoding session is already open on this engine (rk_llama_session_close first)");
  const rk_llama_desc& l = e->ld;
  if (n_slots <= 0 || max_len <= 1 || max_new_cap <= 0) return fail(e, RK_ERR_INVALID, "n_slots, max_new_cap must be positive and max_len > 1 (got %d, %d, %d)", n_slots, max_new_cap, max_len);
  if (n_slots > l.max_seqs) return fail(e, RK_ERR_CAPACITY, "n_slots %d > max_seqs %d", n_slots, l.max_seqs);
  if (draft && e->samp.on()) return fail(e, RK_ERR_STATE, "rk_llama_session_open_draft while sampling is on: drafting is lossless for greedy decoding only (rk_llama_set_sampling(0, ...) first, or draft = 0)");
  if (draft && (long)n_slots * (draft + 1) > l.max_seqs)
    return fail(e, RK_ERR_CAPACITY, "n_slots %d x (draft %d + 1) = %ld step rows > max_seqs %d (the step's activation rows)", n_slots, draft, (long)n_slots * (draft + 1), l.max_seqs);
  if (max_len > l.max_tokens) return fail(e, RK_ERR_CAPACITY, "max_len %d > max_tokens %d (the rotary tables end there)", max_len, l.max_tokens);
  int rc;
  if ((rc = check_stop_ids(e, eos_ids, n_eos, pad_id))) return rc;
  if ((rc = set_device(e))) return rc;
  const SessionLayout lay(n_slots, max_new_cap, max_len, draft);
  const size_t S = (size_t)n_slots, G1 = (size_t)draft + 1;
  if ((rc = ensure_amax(e, S * G1))) return rc;
  if ((rc = ensure_llama_gen(e, n_slots, max_len, lay.total, (int)(S * G1)))) return rc;
  if (e->samp.on() && (rc = ensure_sample_head(e, S))) return rc;
  auto& ls = e->ls;
  ls.n_slots = n_slots; ls.max_len = max_len; ls.cap = max_new_cap; ls.seen = 0; ls.lay = lay;
  ls.draft = draft; ls.ngram_min = ngram_min; ls.ngram_max = ngram_max; ls.steps = 0; ls.tokens = 0;
  ls.sampled = e->samp.on(); ls.seeds.assign(S, 0);          // latched: rk_llama_set_sampling is refused until the close
  ls.busy.assign(S, 0); ls.told.assign(S, 0); ls.len.assign(S, 0); ls.max_new.assign(S, 0); ls.col.assign(S, 0); ls.done.assign(S, 1);
  const std::vector<int> init = lay.initial(eos_ids, n_eos, pad_id, ngram_min, ngram_max);   // every slot idle
  hipStream_t st = e->slots[0].se;
  HIPCHK(e, hipStreamSynchronize(st));
  HIPCHK(e, hipMemcpy(e->lints.p, init.data(), init.size() * sizeof(int), hipMemcpyHostToDevice));
  ls.open = true;
  return RK_OK;
}

int rk_llama_session_open(rk_engine* e, int n_slots, int max_len, int max_new_cap, const int32_t* eos_ids, int n_eos, int pad_id) {
  return session_open(e, n_slots, max_len, max_new_cap, eos_ids, n_eos, pad_id, 0, 1, 1);
}

// ---- drafting by prompt lookup: the same tokens in fewer steps ----
// A session opened with draft = Kd in 1..7 runs G1 = Kd + 1 rows per slot and step: row (s, 0) is the plain session's row, row (s, j)
// feeds draft token d_j at the next position.  A row's bits follow from its own tokens and position and the key a row leaves in the
// cache is the one any other route writes for that token, so the arg-max of row j IS the plain session's token wherever the drafts
// in front of it were right: llama_session_advance_draft_kernel accepts exactly those, and the tokens of a request are bit for bit
// the plain session's - only the number of steps differs.  Keys a rejected row left beyond the accepted position are overwritten
// by the rows that get there before any row reads them (a row reads keys <= its own position, all written in this step or before
// by accepted rows).  The drafts come from draft_lookup_kernel (n-gram lookup in the slot's own prompt and output).
int rk_llama_session_open_draft(rk_engine* e, int n_slots, int max_len, int max_new_cap, const int32_t* eos_ids, int n_eos, int pad_id,
                                int draft, int ngram_min, int ngram_max) {
  if (!e) return RK_ERR_INVALID;
  if (draft < 0 || draft > 7) return fail(e, RK_ERR_INVALID, "draft must be in 0..7 extra rows per slot (got %d)", draft);
  if (ngram_min < 1 || ngram_max > 8 || ngram_min > ngram_max)
    return fail(e, RK_ERR_INVALID, "ngram_min / ngram_max must satisfy 1 <= min <= max <= 8 (got %d, %d)", ngram_min, ngram_max);
  return session_open(e, n_slots, max_len, max_new_cap, eos_ids, n_eos, pad_id, draft, ngram_min, ngram_max);
}

// seeds: null from rk_llama_session_admit, the prompts' seeds from rk_llama_session_admit_sampled; which of the two a session takes
// was decided at its open
static int session_admit(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, const int32_t* slots, const int32_t* max_new, int n,
                         const uint64_t* seeds, const char* who) {
  int rc = session_check(e, who);
  if (rc) return rc;
  auto& ls = e->ls;
  if (seeds && ls.draft) return fail(e, RK_ERR_STATE, "%s on a drafting session (rk_llama_session_open_draft): drafting decodes greedily, admit with rk_llama_session_admit", who);
  if (seeds && !ls.sampled) return fail(e, RK_ERR_STATE, "%s: the session was opened with sampling off (rk_llama_set_sampling before rk_llama_session_open)", who);
  if (!seeds && ls.sampled) return fail(e, RK_ERR_STATE, "%s: the session was opened with sampling on: every admit is rk_llama_session_admit_sampled", who);
  if (!tokens || !seq_offsets || !slots || !max_new || n <= 0) return fail(e, RK_ERR_INVALID, "empty admit (n=%d)", n);
  // every check before anything is touched: a refused admit leaves the session as it was
  std::vector<char> taken(ls.n_slots, 0);
  for (int b = 0; b < n; ++b) {
    const int s = slots[b];
    if (s < 0 || s >= ls.n_slots) return fail(e, RK_ERR_INVALID, "slot %d out of range (the session has %d)", s, ls.n_slots);
    if (taken[s]) return fail(e, RK_ERR_INVALID, "slot %d named twice in one admit", s);
    if (ls.busy[s]) return fail(e, RK_ERR_STATE, "slot %d is busy (rk_llama_session_read frees it)", s);
    taken[s] = 1;
  }
  Slot& sl = e->slots[0];
  if ((rc = check_batch(e, nullptr, tokens, seq_offsets, n))) return rc;
  for (int b = 0; b < n; ++b) {
    const int L = seq_offsets[b + 1] - seq_offsets[b];
    if (max_new[b] <= 0) return fail(e, RK_ERR_INVALID, "max_new must be positive (prompt %d: %d)", b, max_new[b]);
    if (max_new[b] > ls.cap) return fail(e, RK_ERR_CAPACITY, "prompt %d: max_new %d > the session's max_new_cap %d", b, max_new[b], ls.cap);
    if ((long)L + max_new[b] > ls.max_len) return fail(e, RK_ERR_CAPACITY, "prompt %d: %d tokens + max_new %d exceed the session's max_len %d", b, L, max_new[b], ls.max_len);
  }
  const SessionInts d = session_ints(e);
  hipStream_t st = sl.se;
  std::vector<int> adm(3 * (size_t)n);                     // slot[n] | len[n] | max_new[n]: its head is the cache fill's slot map
  for (int b = 0; b < n; ++b) { adm[b] = slots[b]; adm[n + b] = seq_offsets[b + 1] - seq_offsets[b]; adm[2 * n + b] = max_new[b]; }
  HIPCHK(e, hipStreamSynchronize(st));                     // (nothing is in flight between two session calls)
  HIPCHK(e, hipMemcpy(d.admit, adm.data(), adm.size() * sizeof(int), hipMemcpyHostToDevice));
  if (seeds) {                                             // a slot keeps its seed until its next admit
    for (int b = 0; b < n; ++b) ls.seeds[slots[b]] = seeds[b];
    HIPCHK(e, hipMemcpy(e->d_seeds, ls.seeds.data(), ls.seeds.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  }
  const LlamaKeep keep{e->lkv.p, ls.max_len, d.admit, ls.n_slots};
  if ((rc = llama_prefill(e, tokens, seq_offsets, n, &keep))) return rc;
  // (sampled: row r draws with its slot's seed, admit[r], at the index behind its prompt's last token)
  if ((rc = llama_head(e, st, n, HeadHow{seeds != nullptr, d.admit, e->d_pos, sl.idx.d[IX_LAST_ROWS]}))) return rc;
  session_advance(e, st, d, SessionAdmit{d.admit, n, sl.d_tokens, sl.d_seq_off});   // the prompts' ids and offsets: the prefill's device copies
  for (int b = 0; b < n; ++b) { const int s = slots[b]; ls.busy[s] = 1; ls.told[s] = 0; ls.len[s] = adm[n + b]; ls.max_new[s] = max_new[b]; }
  return session_read_back(e, st);
}
int rk_llama_session_admit(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, const int32_t* slots, const int32_t* max_new, int n) {
  return session_admit(e, tokens, seq_offsets, slots, max_new, n, nullptr, "rk_llama_session_admit");
}
int rk_llama_session_admit_sampled(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, const int32_t* slots, const int32_t* max_new, int n,
                                   const uint64_t* seeds) {
  if (!e) return RK_ERR_INVALID;
  if (!seeds) return fail(e, RK_ERR_INVALID, "rk_llama_session_admit_sampled: null seeds");
  return session_admit(e, tokens, seq_offsets, slots, max_new, n, seeds, "rk_llama_session_admit_sampled");
}

int rk_llama_session_run(rk_engine* e, int max_steps, int32_t* out_finished, int32_t* out_n_finished, int32_t* out_steps) {
  int rc = session_check(e, "rk_llama_session_run");
  if (rc) return rc;
  if (!out_finished || !out_n_finished) return fail(e, RK_ERR_INVALID, "null output");
  auto& ls = e->ls;
  Slot& sl = e->slots[0];
  hipStream_t st = sl.se;
  const SessionInts d = session_ints(e);
  auto untold = [&]() { for (int b = 0; b < ls.n_slots; ++b) if (ls.busy[b] && ls.done[b] && !ls.told[b]) return true; return false; };
  // the steps after which no slot can still be active: a bound on the loop whatever the device says
  int live = 0;
  for (int b = 0; b < ls.n_slots; ++b) if (ls.busy[b] && !ls.done[b]) live = std::max(live, ls.max_new[b] - ls.col[b]);
  int steps = 0;
  if (!untold() && live > 0 && max_steps > 0) {
    // one step: a row per slot fed next[] at pos[], or G1 rows per slot - the drafting session's - fed by the proposer; the head;
    // the state machine (and the proposer)
    const int G1 = ls.draft + 1, rows = ls.n_slots * G1;
    auto step = [&]() -> int {
      int r = llama_step_rows(e, st, rows, ls.max_len, ls.draft ? d.rnext : d.next, ls.draft ? d.rpos : d.pos, G1, d.rlive);
      if (r || (r = llama_head(e, st, rows, HeadHow{ls.sampled, nullptr, d.pos, nullptr}))) return r;
      session_advance(e, st, d);
      return RK_OK;
    };
    // until the session word moves (a finish), one step queued behind it; `live` bounds the loop whatever the device says
    RC(decode_loop(e, st, llama_step_key(e, true, ls.n_slots, ls.max_len, ls.cap, ls.sampled, ls.draft), step, 0, 0, std::min(max_steps, live),
                   d.st + SES_FINISHES, ls.seen, &steps));
    sl.n_seq = rows;                                       // rk_debug_read("llama_last"): the step's final rows
    long long before = 0, after = 0;
    for (int b = 0; b < ls.n_slots; ++b) before += ls.col[b];
    RC(session_read_back(e, st));
    for (int b = 0; b < ls.n_slots; ++b) after += ls.col[b];
    ls.steps += steps; ls.tokens += after - before;        // rk_llama_session_stats
  }
  int nf = 0;
  for (int b = 0; b < ls.n_slots; ++b)
    if (ls.busy[b] && ls.done[b] && !ls.told[b]) { out_finished[nf++] = b; ls.told[b] = 1; }
  *out_n_finished = nf;
  if (out_steps) *out_steps = steps;
  return RK_OK;
}

int rk_llama_session_read(rk_engine* e, int slot, int32_t* out_tokens, int cap, int32_t* out_n) {
  int rc = session_check(e, "rk_llama_session_read");
  if (rc) return rc;
  auto& ls = e->ls;
  if (!out_tokens || !out_n) return fail(e, RK_ERR_INVALID, "null output");
  if (slot < 0 || slot >= ls.n_slots) return fail(e, RK_ERR_INVALID, "slot %d out of range (the session has %d)", slot, ls.n_slots);
  if (!ls.busy[slot] || !ls.done[slot]) return fail(e, RK_ERR_STATE, "slot %d %s", slot, ls.busy[slot] ? "has not finished" : "is idle");
  const int n = ls.col[slot];
  if (cap < n) return fail(e, RK_ERR_CAPACITY, "slot %d holds %d tokens, the caller's buffer %d", slot, n, cap);
  const SessionInts d = session_ints(e);
  HIPCHK(e, hipMemcpy(out_tokens, d.out + (size_t)slot * ls.cap, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  const int zero = 0;                                      // idle again: one key chunk of attention per step
  HIPCHK(e, hipMemcpy(ls.draft ? d.rpos + (size_t)slot * (ls.draft + 1) : d.pos + slot, &zero, sizeof(int), hipMemcpyHostToDevice));
  *out_n = n;
  ls.busy[slot] = 0; ls.told[slot] = 0;
  return RK_OK;
}

// steps issued by rk_llama_session_run since the open and the tokens they emitted (the admits' first tokens not counted); per slot
// (null: not wanted) the steps its current request was active in and its output column.  The host mirror, and for a drafting
// session's slot steps one read of the device counters: the stream is idle between two session calls.
int rk_llama_session_stats(rk_engine* e, int64_t* out_steps, int64_t* out_tokens, int32_t* out_slot_steps, int32_t* out_slot_cols) {
  int rc = session_check(e, "rk_llama_session_stats");
  if (rc) return rc;
  auto& ls = e->ls;
  if (out_steps) *out_steps = ls.steps;
  if (out_tokens) *out_tokens = ls.tokens;
  if (out_slot_cols) for (int b = 0; b < ls.n_slots; ++b) out_slot_cols[b] = ls.busy[b] ? ls.col[b] : 0;
  if (out_slot_steps) {
    if (ls.draft) HIPCHK(e, hipMemcpy(out_slot_steps, session_ints(e).nstep, (size_t)ls.n_slots * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < ls.n_slots; ++b) {
      if (!ls.busy[b]) out_slot_steps[b] = 0;
      else if (!ls.draft) out_slot_steps[b] = ls.col[b] - 1;   // one token per step behind the admit's
    }
  }
  return RK_OK;
}

// debug (tests, tools/bench_llama_draft.py): the slot's proposer takes its drafts from `tokens` [n], indexed by output column
// (d_j = tokens[col + j - 1]: the continuation a caller expects), in place of the lookup - acceptance becomes a function of the
// table whatever a toy model emits.  n = 0 with tokens = null: back to the lookup.  In force from the slot's next admit or step.
int rk_debug_session_drafts(rk_engine* e, int slot, const int32_t* tokens, int n) {
  int rc = session_check(e, "rk_debug_session_drafts");
  if (rc) return rc;
  auto& ls = e->ls;
  if (!ls.draft) return fail(e, RK_ERR_STATE, "rk_debug_session_drafts on a session without drafting (rk_llama_session_open_draft)");
  if (slot < 0 || slot >= ls.n_slots) return fail(e, RK_ERR_INVALID, "slot %d out of range (the session has %d)", slot, ls.n_slots);
  if (n < 0 || n > ls.cap || (n > 0 && !tokens)) return fail(e, RK_ERR_CAPACITY, "a draft table holds 0..max_new_cap = %d tokens (got %d)", ls.cap, n);
  if ((rc = check_ids(e, tokens, n, "draft"))) return rc;
  const SessionInts d = session_ints(e);
  hipStream_t st = e->slots[0].se;
  const int tabn = tokens ? n : -1;
  HIPCHK(e, hipStreamSynchronize(st));
  if (n > 0) HIPCHK(e, hipMemcpy(d.tab + (size_t)slot * ls.cap, tokens, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(d.tabn + slot, &tabn, sizeof(int), hipMemcpyHostToDevice));
  launch_draft_lookup(st, d, ls.n_slots, ls.draft + 1);   // the next step's rows, by the new table
  HIPCHK(e, hipStreamSynchronize(st));
  HIPCHK(e, hipGetLastError());
  return RK_OK;
}

int rk_llama_session_close(rk_engine* e) {
  if (!e) return RK_ERR_INVALID;
  if (!e->ls.open) return RK_OK;
  int rc = set_device(e);
  if (rc) return rc;
  e->ls.open = false;                                      // (the buffers and the step graph stay for the next open of these sizes)
  HIPCHK(e, hipStreamSynchronize(e->slots[0].se));
  return RK_OK;
}

// ---- K9: score collection across the GPUs of a node, RCCL over xGMI, straight from the slot's device score buffer --
int rk_comm_unique_id(uint8_t* out_id, int n_bytes) {
  if (!out_id || n_bytes != RK_COMM_ID_BYTES) return fail(nullptr, RK_ERR_INVALID, "unique id buffer must be %d bytes", RK_COMM_ID_BYTES);
  static_assert(RK_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "rk_engine.h and rccl.h disagree on the id size");
  const RcclApi* r = rccl_api();
  if (!r) return fail(nullptr, RK_ERR_HIP, "%s", g_rccl.err.c_str());
  ncclUniqueId id;
  const ncclResult_t rc = r->GetUniqueId(&id);
  if (rc != ncclSuccess) return fail(nullptr, RK_ERR_HIP, "ncclGetUniqueId: %s", r->GetErrorString(rc));
  memcpy(out_id, id.internal, RK_COMM_ID_BYTES);
  return RK_OK;
}

int rk_comm_init(rk_engine* e, const uint8_t* id_bytes, int n_bytes, int rank, int world, int max_floats_per_rank) {
  if (!e || !id_bytes || n_bytes != RK_COMM_ID_BYTES) return fail(e, RK_ERR_INVALID, "bad unique id");
  if (world < 1 || rank < 0 || rank >= world || max_floats_per_rank <= 0) return fail(e, RK_ERR_INVALID, "bad rank %d / world %d / capacity %d", rank, world, max_floats_per_rank);
  if (!e->finalized) return fail(e, RK_ERR_STATE, "engine not finalized");
  int rc = set_device(e);
  if (rc) return rc;
  const RcclApi* r = rccl_api();
  if (!r) return fail(e, RK_ERR_HIP, "%s", g_rccl.err.c_str());
  comm_release(e);
  ncclUniqueId id;
  memcpy(id.internal, id_bytes, RK_COMM_ID_BYTES);
  const ncclResult_t nrc = r->CommInitRank(&e->comm, world, id, rank);   // collective over all ranks
  if (nrc != ncclSuccess) { e->comm = nullptr; return fail(e, RK_ERR_HIP, "ncclCommInitRank(rank %d of %d): %s", rank, world, r->GetErrorString(nrc)); }
  e->comm_rank = rank; e->comm_world = world; e->gather_cap = (size_t)max_floats_per_rank;
  if ((rc = comm_alloc_buffers(e))) {     // a half-built communicator must not report a capacity: tear it down, keep the message
    const std::string why = e->err;
    comm_release(e);
    e->err = why;
    return rc;
  }
  return RK_OK;
}

int rk_comm_world(const rk_engine* e, int* out_rank, int* out_world) {
  if (!e) return RK_ERR_INVALID;
  if (out_rank) *out_rank = e->comm ? e->comm_rank : 0;
  if (out_world) *out_world = e->comm ? e->comm_world : 1;
  return RK_OK;
}

int rk_comm_capacity(const rk_engine* e) { return (e && e->comm) ? (int)e->gather_cap : 0; }

int rk_comm_library_info(char* buf, int n_bytes) {
  if (!buf || n_bytes <= 1) return RK_ERR_INVALID;
  const RcclApi* r = rccl_api();
  if (!r) return fail(nullptr, RK_ERR_HIP, "%s", g_rccl.err.c_str());
  Dl_info info{};
  const char* path = (dladdr((void*)r->AllGather, &info) && info.dli_fname) ? info.dli_fname : "?";
  int ver = 0;
  if (r->GetVersion) r->GetVersion(&ver);
  const int n = snprintf(buf, (size_t)n_bytes, "%s|%d", path, ver);
  return n < n_bytes ? n : n_bytes - 1;
}

int rk_comm_all_gather_slot(rk_engine* e, int slot, int n_floats) {
  if (!e || slot < 0 || slot >= RK_SLOTS) return RK_ERR_INVALID;
  if (!e->comm) return fail(e, RK_ERR_STATE, "rk_comm_init has not been called");
  if (n_floats <= 0 || (size_t)n_floats > e->gather_cap || (size_t)n_floats > e->scores_cap) return fail(e, RK_ERR_CAPACITY, "n_floats %d out of range (capacity %zu, score buffer %zu)", n_floats, e->gather_cap, e->scores_cap);
  int rc = set_device(e);
  if (rc) return rc;
  Slot& sl = e->slots[slot];
  hipStream_t sd = dec_stream(e, sl);   // the stream the slot's scores are produced on: the gather simply follows them
  if (e->gather_pending[slot]) { HIPCHK(e, hipEventSynchronize(e->ev_gather[slot])); e->gather_pending[slot] = false; }
  const ncclResult_t nrc = rccl_api()->AllGather(sl.d_scores, e->d_gather[slot], (size_t)n_floats, ncclFloat, e->comm, sd);
  if (nrc != ncclSuccess) return fail(e, RK_ERR_HIP, "ncclAllGather: %s", rccl_api()->GetErrorString(nrc));
  HIPCHK(e, hipMemcpyAsync(e->h_gather[slot], e->d_gather[slot], (size_t)n_floats * e->comm_world * sizeof(float), hipMemcpyDeviceToHost, sd));
  HIPCHK(e, hipEventRecord(e->ev_gather[slot], sd));
  e->gather_pending[slot] = true; e->gather_n[slot] = n_floats;
  return mark_decoder_done(e, sl);      // the slot's buffers stay busy until the gather has read them
}

int rk_comm_read_gathered_slot(rk_engine* e, int slot, float* out, int n_floats_total) {
  if (!e || !out || slot < 0 || slot >= RK_SLOTS) return RK_ERR_INVALID;
  if (!e->comm) return fail(e, RK_ERR_STATE, "rk_comm_init has not been called");
  if (n_floats_total != e->gather_n[slot] * e->comm_world) return fail(e, RK_ERR_INVALID, "asked for %d floats, the last gather of slot %d holds %d", n_floats_total, slot, e->gather_n[slot] * e->comm_world);
  if (e->gather_pending[slot]) { HIPCHK(e, hipEventSynchronize(e->ev_gather[slot])); e->gather_pending[slot] = false; }
  memcpy(out, e->h_gather[slot], (size_t)n_floats_total * sizeof(float));
  return RK_OK;
}

// Appended form: a rank whose share of a query's candidates needs several engine calls (more sequences or tokens than one
// call holds) copies each call's scores behind the ones before - device to device, on the stream that produced them - and
// ONE all_gather ships the whole share.  Every rank issues exactly one collective per query whatever its chunk count.
int rk_comm_append_scores_slot(rk_engine* e, int slot, int n_floats, int dst_offset) {
  if (!e || slot < 0 || slot >= RK_SLOTS) return RK_ERR_INVALID;
  if (!e->comm) return fail(e, RK_ERR_STATE, "rk_comm_init has not been called");
  if (n_floats < 0 || dst_offset < 0 || (size_t)n_floats + (size_t)dst_offset > e->gather_cap || (size_t)n_floats > e->scores_cap)
    return fail(e, RK_ERR_CAPACITY, "append of %d floats at %d exceeds the send buffer (%zu) or the score buffer (%zu)", n_floats, dst_offset, e->gather_cap, e->scores_cap);
  int rc = set_device(e);
  if (rc) return rc;
  if (n_floats == 0) return RK_OK;
  Slot& sl = e->slots[slot];
  hipStream_t sd = dec_stream(e, sl);
  // the previous gather still reads the send buffer until its event has passed
  if (e->gall_pending) { HIPCHK(e, hipEventSynchronize(e->ev_gall)); e->gall_pending = false; }
  HIPCHK(e, hipMemcpyAsync(e->d_gsend + dst_offset, sl.d_scores, (size_t)n_floats * sizeof(float), hipMemcpyDeviceToDevice, sd));
  if (sd != dec_stream(e, e->slots[0])) { HIPCHK(e, hipEventRecord(e->ev_append, sd)); e->append_foreign = true; }
  return mark_decoder_done(e, sl);      // the slot's score buffer stays busy until the copy has read it
}

int rk_comm_append_host(rk_engine* e, const float* values, int n_floats, int dst_offset) {
  if (!e || (!values && n_floats > 0)) return RK_ERR_INVALID;
  if (!e->comm) return fail(e, RK_ERR_STATE, "rk_comm_init has not been called");
  if (n_floats < 0 || dst_offset < 0 || (size_t)n_floats + (size_t)dst_offset > e->gather_cap)
    return fail(e, RK_ERR_CAPACITY, "append of %d host floats at %d exceeds the send buffer (%zu)", n_floats, dst_offset, e->gather_cap);
  int rc = set_device(e);
  if (rc) return rc;
  if (n_floats == 0) return RK_OK;
  // the previous gather still reads the send buffer (and its staging copy may be in flight) until its event has passed
  if (e->gall_pending) { HIPCHK(e, hipEventSynchronize(e->ev_gall)); e->gall_pending = false; }
  hipStream_t s0 = dec_stream(e, e->slots[0]);     // the stream rk_comm_all_gather_appended runs on: the copy precedes it in order
  // one staging region per destination range: regions of one query do not overlap, the next query starts behind the gather's event
  memcpy(e->h_gstage + dst_offset, values, (size_t)n_floats * sizeof(float));
  HIPCHK(e, hipMemcpyAsync(e->d_gsend + dst_offset, e->h_gstage + dst_offset, (size_t)n_floats * sizeof(float), hipMemcpyHostToDevice, s0));
  return RK_OK;
}

int rk_comm_all_gather_appended(rk_engine* e, int n_floats) {
  if (!e) return RK_ERR_INVALID;
  if (!e->comm) return fail(e, RK_ERR_STATE, "rk_comm_init has not been called");
  if (n_floats <= 0 || (size_t)n_floats > e->gather_cap) return fail(e, RK_ERR_CAPACITY, "n_floats %d out of range (capacity %zu)", n_floats, e->gather_cap);
  int rc = set_device(e);
  if (rc) return rc;
  hipStream_t s0 = dec_stream(e, e->slots[0]);
  if (e->gall_pending) { HIPCHK(e, hipEventSynchronize(e->ev_gall)); e->gall_pending = false; }
  if (e->append_foreign) { HIPCHK(e, hipStreamWaitEvent(s0, e->ev_append, 0)); e->append_foreign = false; }
  const ncclResult_t nrc = rccl_api()->AllGather(e->d_gsend, e->d_gall, (size_t)n_floats, ncclFloat, e->comm, s0);
  if (nrc != ncclSuccess) return fail(e, RK_ERR_HIP, "ncclAllGather: %s", rccl_api()->GetErrorString(nrc));
  HIPCHK(e, hipMemcpyAsync(e->h_gall, e->d_gall, (size_t)n_floats * e->comm_world * sizeof(float), hipMemcpyDeviceToHost, s0));
  HIPCHK(e, hipEventRecord(e->ev_gall, s0));
  e->gall_pending = true; e->gall_n = n_floats;
  return RK_OK;
}

int rk_comm_read_appended(rk_engine* e, float* out, int n_floats_total) {
  if (!e || !out) return RK_ERR_INVALID;
  if (!e->comm) return fail(e, RK_ERR_STATE, "rk_comm_init has not been called");
  if (n_floats_total != e->gall_n * e->comm_world) return fail(e, RK_ERR_INVALID, "asked for %d floats, the last appended gather holds %d", n_floats_total, e->gall_n * e->comm_world);
  if (e->gall_pending) { HIPCHK(e, hipEventSynchronize(e->ev_gall)); e->gall_pending = false; }
  memcpy(out, e->h_gall, (size_t)n_floats_total * sizeof(float));
  return RK_OK;
}

int rk_comm_destroy(rk_engine* e) {
  if (!e) return RK_ERR_INVALID;
  if (set_device(e) == RK_OK) sync_all(e);
  comm_release(e);
  return RK_OK;
}

int rk_timer_begin(rk_engine* e) {
  if (!e) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  // callers synchronise before a timed region; make every other stream start behind the start event anyway
  hipStream_t s0 = e->slots[0].se;
  HIPCHK(e, hipEventRecord(e->t0, s0));
  for (Slot& sl : e->slots) {
    if (sl.se != s0) HIPCHK(e, hipStreamWaitEvent(sl.se, e->t0, 0));
    HIPCHK(e, hipStreamWaitEvent(sl.sd, e->t0, 0));
  }
  return RK_OK;
}

int rk_timer_end(rk_engine* e, float* out_ms) {
  if (!e || !out_ms) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  // the stop event must follow the work of ALL streams: chain them into slot 0's encoder stream
  hipStream_t s0 = e->slots[0].se;
  for (Slot& sl : e->slots) {
    if (sl.se != s0) { HIPCHK(e, hipEventRecord(e->t_tmp, sl.se)); HIPCHK(e, hipStreamWaitEvent(s0, e->t_tmp, 0)); }
    HIPCHK(e, hipEventRecord(e->t_tmp, sl.sd)); HIPCHK(e, hipStreamWaitEvent(s0, e->t_tmp, 0));
  }
  HIPCHK(e, hipEventRecord(e->t1, s0));
  HIPCHK(e, hipEventSynchronize(e->t1));
  HIPCHK(e, hipEventElapsedTime(out_ms, e->t0, e->t1));
  return RK_OK;
}

int rk_profile_enable(rk_engine* e, int on) { if (!e) return RK_ERR_INVALID; e->prof_on = on != 0; return RK_OK; }

int rk_profile_reset(rk_engine* e) {
  if (!e) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if ((rc = sync_all(e))) return rc;
  e->prof_used = 0;
  for (int c = 0; c < PC_COUNT; ++c) { e->prof_flops[c] = 0; e->prof_bytes[c] = 0; e->prof_n[c] = 0; }
  return RK_OK;
}

int rk_profile_get(rk_engine* e, int cls, double* total_ms, int64_t* launches, double* flops, double* bytes) {
  if (!e || cls < 0 || cls >= PC_COUNT) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if ((rc = sync_all(e))) return rc;
  double ms = 0;
  for (size_t i = 0; i < e->prof_used; ++i) {
    if (e->prof_recs[i].cls != cls) continue;
    float t = 0;
    HIPCHK(e, hipEventElapsedTime(&t, e->prof_recs[i].a, e->prof_recs[i].b));
    ms += t;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = e->prof_n[cls];
  if (flops) *flops = e->prof_flops[cls];
  if (bytes) *bytes = e->prof_bytes[cls];
  return RK_OK;
}

}  // extern "C" (reopened behind the option table)

// Option table: key -> field, the values it accepts (lo..hi, or the listed set), meaning.  A value outside the range is an error
// (RK_ERR_INVALID), as include/rk_engine.h promises - a sweep can never record a value that was not applied.
namespace {
struct OptionDesc { const char* key; int rk_engine::Options::*field; int lo, hi; const char* allowed; const char* what; };
const OptionDesc kOptions[] = {
  {"dec_graph", &rk_engine::Options::dec_graph, 0, 1, nullptr, "decoder chains replayed as HIP graphs (1) or launched eagerly (0)"},
  {"gemm_glds", &rk_engine::Options::glds, 0, 1, nullptr, "128x128 GEMM staging by LDS-DMA (1) or through registers (0); same bits"},
  {"gemm_skinny", &rk_engine::Options::skinny, 0, 0x3F, nullptr, "bit per epilogue kind: few-row GEMMs on the weight-streaming kernel (1 = all)"},
  {"dec_ffn_tiled", &rk_engine::Options::dec_ffn_tiled, 0, 1, nullptr, "one-position decoder: FFN-in on the tiled kernels (1) or the weight-streaming kernel (0)"},
  {"gemm_persistent", &rk_engine::Options::gemm_persistent, 0, 1024, nullptr, "ping-pong GEMM: 1 = one workgroup per CU walks the tiles, 0 = one per tile, n > 1 = n workgroups"},
  {"gemm_s64_stages", &rk_engine::Options::s64_stages, 0, 4, "0,2,3,4", "LDS stages of the 64x64 GEMM (0 = from the tile count); same bits"},
  {"consumer_stats", &rk_engine::Options::consumer_stats, 0, 1, nullptr, "encoder row factors formed by the non-persistent consumer GEMMs themselves (1) or always by rowscale_kernel (0); same bits"},
  {"greedy_spec", &rk_engine::Options::greedy_spec, 0, 65536, nullptr, "rk_t5_greedy2: most decoder rows of a speculative pass; 0 = never speculate; same tokens"},
  {"dec_fold_norm", &rk_engine::Options::dec_fold_norm, 0, 1, nullptr, "decoder RMSNorms folded into the weight-streaming GEMMs (1) or separate kernels (0)"},
  {"fold_norm", &rk_engine::Options::fold_norm, 0, 1, nullptr, "encoder RMSNorm folded into the GEMMs (1) or separate kernels (0)"},
  {"xattn_mfma", &rk_engine::Options::xattn_mfma, 0, 1, nullptr, "query-side cross-attention: weighted sums on the matrix cores (1) or the VALU form (0)"},
  {"attn_heads_per_wg", &rk_engine::Options::attn_heads_per_wg, 0, 4096, nullptr, "short-sequence attention: (sequence, head) items per wave group, 0 = dealt evenly; same bits"},
  {"xattn_direct", &rk_engine::Options::xattn_direct, 0, 1, nullptr, "decoder prefixes <= 16: query-side cross-attention (1) or materialised K / V (0)"},
  {"attn_short", &rk_engine::Options::attn_short, 0, 6, "0,5,6", "sequences <= 192 keys: DMA kernel with two (5) / one (6) wave group per workgroup, or the tiled kernel (0); same bits"},
  {"gemm_variant", &rk_engine::Options::gemm_variant, 0, 120, nullptr, "tile variant: 0 auto, 1..6 see choose_variant; measurement builds: 80+ / 100+ knock-outs"},
  {"dec_fuse_rows", &rk_engine::Options::dec_fuse_rows, 0, 32, nullptr, "rows per workgroup of dec_cross_qk_kernel (0 = auto); same bits"},
  {"dec_fuse", &rk_engine::Options::dec_fuse, 0, 2, nullptr, "few-row decoder: projections around the query-side cross-attention fused at one position (1), always (2), never (0)"},
  {"llama_attn_nw", &rk_engine::Options::llama_attn_nw, 0, 8, "0,4,8", "waves per workgroup of the Llama LDS-DMA attention kernel (0 = default 4); same bits"},
  {"llama_attn_dma", &rk_engine::Options::llama_attn_dma, 0, 1, nullptr, "Llama causal attention: LDS-DMA kernel (1) or the register-staged first kernel (0); differ within fp16 noise"},
  {"attn_long_xcd", &rk_engine::Options::attn_long_xcd, 0, 1, nullptr, "long-sequence attention: workgroups of a (sequence, head) pair on one XCD (1) or dealt over all eight (0); same bits"},
  {"attn_long_nw", &rk_engine::Options::attn_long_nw, 0, 12, "0,3,4,6,12", "waves per workgroup of the long-sequence attention kernel (0 = default 4); same bits"},
  {"attn_long", &rk_engine::Options::attn_long, 0, 1, nullptr, "sequences > 192 keys: the chunked LDS-DMA kernel (1) or the tiled kernel (0)"},
  {"dec_gemv", &rk_engine::Options::dec_gemv, 0, 1, nullptr, "decoder pass of at most 16 rows at >= 2 positions (one setwise compare): plain projections on the wave-per-column GEMV kernel (1) or the weight-streaming MFMA kernel (0); differ within fp32 summation-order noise"},
  {"dec_gemv_rows", &rk_engine::Options::dec_gemv_rows, 1, GEMV_MAX_ROWS, nullptr, "largest row count of a decoder pass that takes the few-row GEMV family (default 4 = the measured cross-over; the kernel takes up to 16)"},
  {"dec_cross_mfma", &rk_engine::Options::dec_cross_mfma, 0, 1, nullptr, "long decoder prefixes (qlm), cross-attention over the materialised K / V: matrix-core kernel for sequences <= 192 keys (1) or the staged fma-chain kernels (0); differ within fp16 noise"},
  {"dec_attn_seq", &rk_engine::Options::dec_attn_seq, 0, 1, nullptr, "decoder attention at several positions: one workgroup per (head, sequence) (1) or per query row (0); same bits"},
  {"gemm_sk", &rk_engine::Options::gemm_sk, 0, 2, nullptr, "ping-pong GEMM, K split of the fp32 epilogues over two workgroups: wherever it fits (2: tests, measurement), else never (0, 1 = default: choose_ksplit - a split chosen from the launch's tile count would make a sequence's bits depend on its batch)"},
  {"dec_cached_attn", &rk_engine::Options::dec_cached_attn, 0, 1, nullptr, "rk_t5_generate's self-attention: attn_dec_cached_kernel (1) or the cache append + attn_dec_kernel's tree form (0); same bits"},
  {"llama_dec_r", &rk_engine::Options::llama_dec_r, 0, 2, nullptr, "rk_llama_generate's attention: query heads per workgroup by plan_llama_dec_attn's rule (0), one (1), or, where a kv head has 7, all seven (2: measurement and tests; every cached K / V byte read once per step); same bits"},
  {"enc_serial", &rk_engine::Options::enc_serial, 0, 1, nullptr, "two slots: an encoder chain starts behind the other slot's (1: one encoder at a time beside the decoder before it) or as soon as it is enqueued (0: two chains interleave); same bits"},
  {"llama_step_fp8", &rk_engine::Options::llama_step_fp8, 0, 1, nullptr, "FP8 engines: the step's projections read the FP8 bytes (1, default) or the dequantised fp16 matrices through the fp16 kernel (0); same bits; no effect on an engine without FP8 weights"},
  {"llama_kv_fp8", &rk_engine::Options::llama_kv_fp8, 0, 1, nullptr, "FP8-cache engines (rk_llama_set_kv_fp8): the step reads the cache's FP8 bytes (1, default) or keeps an fp16-layout cache of the dequantised values and reads it with the fp16 kernels (0); same bits; the cache contents do not survive a change, which is refused while a decoding session is open; no effect on an engine without an FP8 cache"},
  {"gemm_split", &rk_engine::Options::gemm_split, 0, 1, nullptr, "rows beyond the ping-pong kernel's last whole round on a fill-in tile variant (1) or one launch (0); same bits"},
#ifdef RK_MEASURE
  {"attn_ko", &rk_engine::Options::attn_ko, 0, 1 << 20, nullptr, "timing-only knock-outs of the attention kernels (measurement builds)"},
#endif
};
bool option_value_ok(const OptionDesc& o, int value) {
  if (value < o.lo || value > o.hi) return false;
  if (!o.allowed) return true;
  for (const char* p = o.allowed; *p;) {
    if (atoi(p) == value) return true;
    while (*p && *p != ',') ++p;
    if (*p == ',') ++p;
  }
  return false;
}
}  // namespace

extern "C" {

int rk_engine_set_option(rk_engine* e, const char* key, int value) {
  if (!e || !key) return RK_ERR_INVALID;
  if (!strcmp(key, "overlap")) {    // 1: decoder chain on its own stream (default); 0: everything on one stream
    if (value < 0 || value > 1) return fail(e, RK_ERR_INVALID, "option overlap: 0..1");
    if (set_device(e) || sync_all(e)) return RK_ERR_HIP;
    for (Slot& sl : e->slots) sl.dec_pending = false;
    e->opt.overlap = value;
    e->opt_epoch++;
    return RK_OK;
  }
#ifdef RK_MEASURE
  if (!strcmp(key, "attn_trace")) {   // phase time stamps of one workgroup of the DMA attention kernel (attention.h: ATTD_STAMP)
    if (value && !e->attn_trace) { if (hipMalloc(&e->attn_trace, 12 * 16 * 16 * sizeof(float)) != hipSuccess) return RK_ERR_HIP; hipMemset(e->attn_trace, 0, 12 * 16 * 16 * sizeof(float)); }
    if (!value && e->attn_trace) { hipFree(e->attn_trace); e->attn_trace = nullptr; }
    return RK_OK;
  }
#endif
  for (const OptionDesc& o : kOptions) {
    if (strcmp(key, o.key)) continue;
    if (!strcmp(key, "gemm_skinny") && value == 1) value = 0x3F;
    if (!strcmp(key, "llama_kv_fp8") && e->ls.open)           // the open session's cache is laid out for the current value
      return fail(e, RK_ERR_STATE, "option llama_kv_fp8 while a decoding session is open (its cache would change layout): rk_llama_session_close first");
    if (!option_value_ok(o, value))
      return fail(e, RK_ERR_INVALID, "option %s: value %d outside %d..%d%s%s (%s)", key, value, o.lo, o.hi, o.allowed ? ", allowed: " : "", o.allowed ? o.allowed : "", o.what);
    e->opt.*(o.field) = value;
    e->opt_epoch++;                                           // cached decoder graphs were captured under the old options
    return RK_OK;
  }
  return fail(e, RK_ERR_INVALID, "unknown option %s", key);
}

}  // extern "C"

#include "debug_calls.inc"   // the rk_debug_* entry points: one translation unit, a file of their own
