/* rk_engine.h — C ABI of the MI355X-native reranking engine (librk_engine.so, gfx950 only).
 *
 * This is the drop-in boundary for ONE hot path of ielab/llm-rankers: the batched T5 encoder-decoder forward
 * behind PointwiseLlmRanker.rerank and SetwiseLlmRanker.compare.  The reference has no FFI of its own; the
 * inner boundary these entry points replace is exactly three HuggingFace calls plus two attributes
 * (SURVEY.md section 8b):
 *
 *   self.llm(input_ids, attention_mask, decoder_input_ids=...).logits   ref: llmrankers/pointwise.py:117-119,
 *                                                                             llmrankers/setwise.py:184
 *   self.llm(input_ids, attention_mask, labels=...).logits               ref: llmrankers/pointwise.py:73-75
 *   self.llm.generate(input_ids, decoder_input_ids=..., max_new_tokens=2) ref: llmrankers/setwise.py:93-95,128-130
 *   T5ForConditionalGeneration.from_pretrained(...)                       ref: llmrankers/pointwise.py:20-24
 *
 * Conventions: plain C, every function returns 0 on success or a negative rk_status; rk_last_error() gives the
 * message of the last failure on that engine (or of the last failed rk_engine_create when engine == NULL).
 * No exceptions, Python objects or torch types cross this boundary.  Inputs are RAGGED: the B token sequences
 * of a batch are concatenated without padding, seq_offsets[B+1] gives the boundaries (the reference right-pads
 * to the batch's longest sequence and masks; results are identical).  The caller owns all host
 * buffers; the engine owns device memory and one HIP stream.  One engine per device; calls on one engine must
 * be serialised by the caller; different engines may be driven from different threads.
 * There is NO CPU fallback: with no usable gfx950 device rk_engine_create fails with RK_ERR_NO_DEVICE.
 */
#ifndef RK_ENGINE_H
#define RK_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rk_engine rk_engine;

typedef enum rk_status {
  RK_OK = 0,
  RK_ERR_INVALID = -1,    /* bad argument / unsupported model dimensions */
  RK_ERR_NO_DEVICE = -2,  /* no gfx950 GPU visible — the engine never falls back to the CPU */
  RK_ERR_HIP = -3,        /* a HIP runtime call failed */
  RK_ERR_STATE = -4,      /* call order violated (e.g. score before finalize) */
  RK_ERR_MISSING = -5,    /* finalize: a required tensor was never loaded */
  RK_ERR_CAPACITY = -6    /* batch exceeds max_tokens / max_seqs / max_dec_len of the engine */
} rk_status;

typedef enum rk_dtype { RK_F32 = 0, RK_F16 = 1, RK_BF16 = 2 } rk_dtype;

/* Mirrors the fields of HF's T5Config the path depends on (hf: models/t5/configuration_t5.py).
 * d_model is at most 4096 (RK_ERR_INVALID beyond: the RMSNorm kernel holds one row of at most 4096 columns in registers).
 * d_kv is 64 or 128 (RK_ERR_INVALID otherwise).  d_kv = 128 (t5-3b, t5-11b: monoT5-3B, duoT5-3B) is served at ONE decoder position:
 * rk_t5_score with dec_len == 1 (blocking, staged, slots), rk_t5_compare and the rk_comm_* calls behind them.  On such an engine
 * rk_t5_score with dec_len > 1, rk_t5_qlm, rk_t5_qlm_many, rk_t5_greedy, rk_t5_greedy2 and rk_t5_generate return RK_ERR_STATE with a
 * message that names d_kv=128 and the entry point, before anything is launched; so do the one-position calls while an option selects
 * a path without a 128-wide form (xattn_direct = 0, dec_fuse = 2). */
typedef struct rk_model_desc {
  int32_t vocab, d_model, n_heads, d_kv, d_ff;
  int32_t n_enc_layers, n_dec_layers;
  int32_t n_buckets, max_distance;   /* relative_attention_num_buckets / _max_distance */
  int32_t gated_gelu;                /* 1: feed_forward_proj = "gated-gelu" (T5 v1.1 / flan); 0: "relu" */
  int32_t tied_head;                 /* 1: lm_head = shared and logits scaled by d_model^-0.5 (T5 v1.0, monoT5) */
  float eps;                         /* layer_norm_epsilon */
  int32_t max_tokens;                /* capacity: encoder tokens per call (sum over the batch) */
  int32_t max_seqs;                  /* capacity: sequences per call */
  int32_t max_dec_len;               /* capacity: decoder positions per sequence */
} rk_model_desc;

/* ---- lifetime & weights (replaces from_pretrained, ref: pointwise.py:20-24 / setwise.py:46-50) ---- */
int rk_engine_create(const rk_model_desc* desc, int device_ordinal, rk_engine** out);
void rk_engine_destroy(rk_engine* e);
const char* rk_last_error(const rk_engine* e);
/* One call per HF state-dict entry (names as in the checkpoint, e.g. "encoder.block.0.layer.0.SelfAttention.q.weight").
 * Data is converted to fp16 (the reference's accelerator dtype).  Names the path does not need are ignored. */
int rk_engine_load_tensor(rk_engine* e, const char* hf_name, const void* data, int dtype, const int64_t* shape, int ndim);
/* Repack (fused QKV, interleaved wi_0|wi_1, stacked cross K/V, bias tables), upload, free host copies. */
int rk_engine_finalize(rk_engine* e);

/* ---- blocking calls on host buffers: what the Python rankers use ---- */
/* logits of the LAST decoder position for out_token_ids (n_out > 0) -> out_logits[n_seq][n_out] fp32.
 * dec_prefix is shared by all sequences ([0] for yes_no, [0, "Passage"] for setwise likelihood).
 * replaces: self.llm(input_ids, attention_mask, decoder_input_ids).logits[:, -1, ids]  (pointwise.py:117-121, setwise.py:184-186) */
int rk_t5_score(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                const int32_t* dec_prefix, int dec_len, const int32_t* out_token_ids, int n_out, float* out_logits);
/* out_scores[b] = -sum_t CE(logits[b,t,:], labels[t]) with decoder input = shift_right(labels).
 * replaces: self.llm(input_ids, attention_mask, labels=...).logits + CrossEntropyLoss(reduction="none") (pointwise.py:73-79) */
int rk_t5_qlm(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
              const int32_t* labels, int n_labels, float* out_scores);
/* rk_t5_qlm for several queries in one call: sequence b scores ITS OWN labels, labels[label_offsets[b] .. label_offsets[b+1])
 * (label_offsets[n_seq + 1], label_offsets[0] == 0): out_scores[b] = -sum_t CE(logits[b,t,:], labels[label_offsets[b] + t]) with
 * decoder input = shift_right of those labels.  A sequence's score is BIT FOR BIT what rk_t5_qlm gives that sequence with those
 * labels, whatever else shares the call and in whatever order (one encoder run over all sequences, one ragged decoder pass per
 * class of label counts that share their arithmetic; DESIGN.md sections 3 and 4 - the one exception is rk_t5_qlm's own: a decoder
 * pass of at most 4 rows at two or more positions).  Blocking; the scores stay in slot 0's device score buffer in sequence order,
 * so rk_comm_append_scores_slot works behind it as behind rk_t5_qlm.  RK_ERR_CAPACITY for a sequence with 0 or more than
 * max_dec_len labels, RK_ERR_INVALID for ids outside the vocabulary or offsets that do not start at 0 and grow.
 * replaces: one self.llm(input_ids, attention_mask, labels=...) call per query (pointwise.py:73-79) for the queries of a group */
int rk_t5_qlm_many(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                   const int32_t* labels, const int32_t* label_offsets, float* out_scores);
/* Greedy continuation of dec_prefix by up to max_new tokens -> out_tokens[n_seq][max_new] (pad_id after EOS;
 * stops early when every row has finished, remaining columns = pad_id); *out_steps = decoder steps executed.
 * replaces: self.llm.generate(input_ids, decoder_input_ids=..., max_new_tokens=2)  (setwise.py:93-95, 128-130) */
int rk_t5_greedy(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                 const int32_t* dec_prefix, int dec_len, int max_new, int eos_id, int pad_id,
                 int32_t* out_tokens, int32_t* out_steps);

/* rk_t5_greedy with max_new = 2 and a hint: the first new token is expected to be one of cand_ids[n_cand] (the passage
 * labels of a setwise compare).  Both steps then run in ONE decoder pass - the second speculatively for every candidate -
 * and out_tokens[n_seq][2] / *out_steps are bit-identical to rk_t5_greedy's; any other first token, or a batch that does
 * not fit the workspace, falls back to rk_t5_greedy itself.
 * replaces: self.llm.generate(input_ids, decoder_input_ids=..., max_new_tokens=2)  (setwise.py:113-115) */
int rk_t5_greedy2(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                  const int32_t* dec_prefix, int dec_len, const int32_t* cand_ids, int n_cand, int eos_id, int pad_id,
                  int32_t* out_tokens, int32_t* out_steps);

/* rk_t5_greedy's arguments and contract (out_tokens[n_seq][max_new], pad_id after EOS, remaining columns pad_id once every row
 * has finished, *out_steps = the decoder steps rk_t5_greedy would have executed, the same capacity errors), decoded
 * incrementally: each step runs ONE new decoder row per sequence against a self-attention K / V cache, the arg-max is fed back on
 * the device and the step is one replayed graph.  For long continuations (the listwise permutation, up to 20 tokens).
 * replaces: self.llm.generate(input_ids)  (ref: llmrankers/listwise.py:248) */
int rk_t5_generate(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                   const int32_t* dec_prefix, int dec_len, int max_new, int eos_id, int pad_id,
                   int32_t* out_tokens, int32_t* out_steps);

/* The duoT5 compare (ref: llmrankers/pairwise.py:296-352): 2 * n_pairs sequences, pair p = sequences 2p (the A/B prompt) and
 * 2p + 1 (the B/A prompt); one decoder position holding dec_start_id; the logits of false_id / true_id, the two-way softmax and
 * the strict verdict P(true)[2p] > P(true)[2p + 1] are taken on the device (pair_verdict_kernel).  out_logits[2 n_pairs][2] =
 * (false, true) are bit for bit rk_t5_score's with dec_prefix = {dec_start_id}, out_token_ids = {false_id, true_id}; out_p_true
 * [2 n_pairs]; out_first_wins[n_pairs] = 1 / 0 (a tie is 0).  A pair's seven floats do not depend on what shares its call.
 * RK_ERR_INVALID for n_pairs <= 0, an id outside the vocabulary or false_id == true_id; RK_ERR_STATE on a Llama engine; the
 * capacity errors of rk_t5_score; nothing is launched after any of them.
 * replaces: self.llm(input_ids, attention_mask, decoder_input_ids).logits[:, 0, [6136, 1176]] + softmax + compare (pairwise.py:330-343) */
int rk_t5_compare(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_pairs,
                  int dec_start_id, int false_id, int true_id,
                  float* out_logits, float* out_p_true, int32_t* out_first_wins);

/* ---- staged / asynchronous form: inputs resident in HBM, used by bench.py and the multi-GPU driver ---- */
int rk_t5_stage(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq);   /* H2D, synchronous */
/* enqueue encoder + decoder + head on the engine stream for the staged batch; scores land in an engine-owned
 * device buffer and are copied to pinned host memory asynchronously. Returns without synchronising. */
int rk_t5_score_staged(rk_engine* e, const int32_t* dec_prefix, int dec_len, const int32_t* out_token_ids, int n_out);
int rk_engine_sync(rk_engine* e);
int rk_t5_read_scores(rk_engine* e, float* out_logits, int n_floats);   /* waits for the batch's decoder, then copies */
/* The same three calls for batch slot `slot` in [0, rk_engine_num_slots()).  Slots are independent batches in flight:
 * the latency-bound decoder chain of one slot runs on its own high-priority HIP stream while the MFMA-bound encoder
 * of the next slot occupies the chip (events order encoder -> decoder per slot).  The un-suffixed calls use slot 0.
 * A slot may be staged again while its launch is still in flight: the launch keeps the batch it was enqueued with (two
 * generations of the staged arrays), its scores stay readable until the next launch on the slot, and the staging waits for
 * no decoder.  The LAUNCH may: rk_t5_score_slot / rk_t5_compare_slot return without waiting only while the slot's n_seq, dec_prefix
 * and out_token_ids (compare: n_seq and dec_start_id) equal those of the slot's previous launch; when one of them differs the
 * call first blocks the host until the slot's earlier decoders are through (its index buffers are re-uploaded through one
 * pinned staging area), then enqueues and returns. */
int rk_engine_num_slots(void);
int rk_t5_stage_slot(rk_engine* e, int slot, const int32_t* tokens, const int32_t* seq_offsets, int n_seq);
int rk_t5_score_slot(rk_engine* e, int slot, const int32_t* dec_prefix, int dec_len, const int32_t* out_token_ids, int n_out);
int rk_t5_read_scores_slot(rk_engine* e, int slot, float* out_logits, int n_floats);
/* rk_t5_score_slot's twin for the duoT5 compare: after rk_t5_stage_slot of 2 * n_pairs sequences (an odd count: RK_ERR_INVALID;
 * no staged batch: RK_ERR_STATE).  The slot's score buffer then holds 7 * n_pairs floats, read whole by
 * rk_t5_read_scores_slot(e, slot, out, 7 * n_pairs): [0, 4 n_pairs) the logits [n_seq][2] = (false, true) - rk_t5_score_slot's
 * place and layout, so the rk_comm_* calls work behind it -, [4 n_pairs, 6 n_pairs) P(true) per sequence, [6 n_pairs, 7 n_pairs)
 * the verdict per pair as 1.0f / 0.0f. */
int rk_t5_compare_slot(rk_engine* e, int slot, int dec_start_id, int false_id, int true_id);
/* device address of the fp32 score buffer [n_seq][n_out] of the last rk_t5_score_staged (for RCCL gathers) */
int rk_t5_scores_device_ptr(rk_engine* e, void** out_ptr);

/* ---- decoder-only Llama family: the model call of the reference's setwise ranker for `model_type == 'llama'`
 * (ref: llmrankers/setwise.py:60-69, 159-177): self.llm.generate(input_ids, do_sample=False, max_new_tokens=1) = prefill
 * of the prompt + arg-max of the last position's logits; and of its listwise ranker (ref: llmrankers/listwise.py:261-271):
 * self.llm.generate(input_ids) = rk_llama_generate, the prefill once and then one KV-cached row per new token.  hf: models/llama/modeling_llama.py (RMSNorm, RoPE with
 * rope_theta, grouped-query causal attention with head_dim 64 or 128 - RK_ERR_INVALID for any other width -, SwiGLU).  Weights go through rk_engine_load_tensor with
 * the HF Llama names ("model.layers.0.self_attn.q_proj.weight", ...) and rk_engine_finalize; rk_engine_destroy frees. */
typedef struct rk_llama_desc {
  int32_t vocab, hidden, n_heads, n_kv_heads, head_dim, intermediate, n_layers;
  int32_t tied_head;                 /* tie_word_embeddings */
  float eps, rope_theta;             /* rms_norm_eps, rope_theta (default rope type) */
  int32_t max_tokens, max_seqs;      /* capacity: prompt tokens per call (sum), prompts per call */
} rk_llama_desc;
int rk_llama_create(const rk_llama_desc* desc, int device_ordinal, rk_engine** out);
/* rope type "llama3" (Llama-3.1 / 3.2 checkpoints; hf: modeling_rope_utils.py _compute_llama3_parameters, reached through
 * AutoModelForCausalLM.from_pretrained at ref: llmrankers/setwise.py:65-69): inverse frequencies whose wavelength exceeds
 * original_max_pos / low_freq_factor are divided by factor, those between original_max_pos / high_freq_factor and that are
 * interpolated.  Call between rk_llama_create and rk_engine_finalize (the rotary tables are built there); never calling
 * it = the default rope type. */
int rk_llama_set_rope_scaling(rk_engine* e, float factor, float low_freq_factor, float high_freq_factor, int original_max_pos);
/* Qwen2 family (hf: models/qwen2/modeling_qwen2.py; Qwen2.5-Instruct checkpoints, the Rank-R1 rerankers of ref:
 * llmrankers/setwise.py:406-553): the q / k / v projections carry a bias.  on != 0: rk_engine_finalize requires
 * model.layers.N.self_attn.{q,k,v}_proj.bias (shapes n_heads * head_dim, n_kv_heads * head_dim, n_kv_heads * head_dim) and the engine adds them
 * in fp32 to the projections' output before the rotation.  Call between rk_llama_create and the first rk_engine_load_tensor;
 * RK_ERR_STATE on a T5 engine or after finalize.  Never calling it (or on = 0): the bias names are ignored. */
int rk_llama_set_qkv_bias(rk_engine* e, int on);
/* Qwen3 family (hf: models/qwen3/modeling_qwen3.py: Qwen3Attention.q_norm / k_norm; Qwen3-0.6B to 8B, the Rank-R1 v0.2 bases): an
 * RMSNorm over head_dim on every query and key head, behind the projection and in front of the rotation, with a weight [head_dim]
 * per layer for q and for k; its eps is the desc's.  on != 0: rk_engine_finalize requires model.layers.N.self_attn.{q,k}_norm.weight
 * (shape head_dim) and the engine applies them in fp32 in the prefill's rotary kernel and in the cached step's row load - one fp16
 * rounding behind norm and rotation, the step's cached key bit for bit the prefill's.  Call between rk_llama_create and
 * rk_engine_finalize; RK_ERR_STATE on a T5 engine or after finalize.  rk_engine_finalize then refuses (RK_ERR_STATE) head_dim 64, a
 * sliding window and q / k / v biases next to it: no Qwen3 checkpoint has them.  Never calling it (or on = 0): the names are ignored. */
int rk_llama_set_qk_norm(rk_engine* e, int on);
/* FP8 step weights (opt-in, LOSSY: one e4m3 rounding per weight of the matrices the decoding step streams; vLLM's
 * quantization="fp8" is the same option).  on != 0: rk_engine_finalize - behind the norm folding - quantises every layer's fused
 * q|k|v, o, gate|up and down matrix, keeps the bytes and exponents (weights grow to 1.5x) and OVERWRITES the fp16 matrix with the
 * dequantised values: prefill, rk_llama_greedy1, rk_llama_last_logits, the session admit and the step all run one model, which is
 * bit for bit an fp16 engine loaded with the dequantised matrices.  The step (rk_llama_generate, rk_llama_session_*) then reads the
 * bytes - half the weight stream - unless option llama_step_fp8 is 0 (the fp16 kernel on the dequantised matrices: same bits).
 * Embeddings, the head, norm weights, Qwen2 biases and Qwen3 q / k norm weights stay as they are.
 * The engine-private format of a matrix W [N][K] (K % 16):
 *   groups  128 consecutive k of one output row; the last group may be shorter
 *   e       per (row, group) one int8 exponent: the smallest integer with absmax <= 448 * 2^e, clamped to [-15, 7] (all-zero: -15)
 *   q       per weight one OCP e4m3fn byte: w * 2^-e rounded to nearest even, saturating at +-448
 *   d       the dequantised weight q * 2^e - an fp16 number by construction (2^-9 * 2^-15 is the smallest fp16 subnormal, 448 * 2^7 < 65 504)
 * Call between rk_llama_create and rk_engine_finalize; RK_ERR_STATE on a T5 engine or after finalize.  Never calling it (or
 * on = 0) leaves the fp16 engine, byte for byte. */
int rk_llama_set_weight_fp8(rk_engine* e, int on);
/* FP8 K / V cache of the decoding step (opt-in, LOSSY: one e4m3 rounding per cached key and value element; vLLM's
 * kv_cache_dtype="fp8" is the same option).  on != 0: the cache rk_llama_generate and rk_llama_session_* keep holds one byte per value
 * and one exponent per vector - at most 0.52x the fp16 cache for the same (rows, positions >= 16) - and the step reads the bytes:
 * half the step's cache stream.  Head width 128 only: rk_engine_finalize refuses (RK_ERR_STATE) a 64-wide engine.
 * The engine-private format:
 *   group   the 128 values of ONE key or value vector of one (cache row, kv head, position); a key as the fp16 cache holds it (behind
 *           the Qwen2 bias, Qwen3's head norm, the rotation and the one fp16 rounding), a value behind the Qwen2 bias
 *   e       per group one int8 exponent: the smallest integer with absmax <= 448 * 2^e, clamped to [-15, 7] (all-zero: -15)
 *   q       per value one OCP e4m3fn byte: x * 2^-e rounded to nearest even, saturating at +-448
 *   d       the dequantised value q * 2^e - an fp16 number by construction, as for the weights above
 *   layout  per layer K bytes [rows][n_kv][P][128] | V bytes | K exponents [rows][n_kv][P'] | V exponents, P' = P rounded up to 32;
 *           every region starts on a multiple of 32 bytes
 * Every writer - the prefill's and the session admit's fill, the step, a drafting step's append - quantises through one device
 * helper, so the key a step writes is byte for byte the key the fill writes for that token; the step's own row sees its new key and
 * value dequantised, exactly as every later step reads them back, so a drafting session still gives the plain session's tokens.
 * The prefill's own attention reads the un-quantised fp16 K / V of its QKV buffer: rk_llama_greedy1, rk_llama_last_logits and
 * rk_llama_qlm are byte for byte an fp16-cache engine's.  ONLY the steps see quantised keys, so rk_llama_generate's tokens on such
 * an engine need not equal those of a loop of rk_llama_greedy1 re-prefills (on an fp16-cache engine they do).
 * Option llama_kv_fp8 = 0 keeps an fp16-layout cache of the dequantised values, read by the fp16 kernels: same bits in every output.
 * Changing it is refused (RK_ERR_STATE) while a decoding session is open; the cache contents do not survive the change.
 * Option llama_dec_r = 2 falls back to the rule on such an engine (no R = 7 instantiation), as at width 64.
 * Call between rk_llama_create and rk_engine_finalize; RK_ERR_STATE on a T5 engine or after finalize.  Never calling it (or
 * on = 0) leaves the fp16 cache, byte for byte.  Combines freely with rk_llama_set_weight_fp8, drafting and sampling. */
int rk_llama_set_kv_fp8(rk_engine* e, int on);
/* Mistral family (hf: models/mistral/modeling_mistral.py, sliding_window_causal_mask; Zephyr / RankZephyr checkpoints): attention
 * with a sliding window of `window` positions.  In the prefill query position i of a sequence sees keys max(0, i - window + 1) .. i;
 * in the cached step (rk_llama_generate, rk_llama_session_*) the row at pos sees max(0, pos - window + 1) .. pos.  The K / V cache
 * keeps every position (no rolling buffer): the window only limits what is read.  A sequence no longer than `window` gets, bit for
 * bit, what an engine without a window gives on the same weights, whatever shares its call.  Call between rk_llama_create and
 * rk_engine_finalize; window = 0, or never calling it: none.  RK_ERR_STATE on a T5 engine or after finalize, RK_ERR_INVALID for
 * window < 0.  The register-staged 128-wide prefill kernel (option llama_attn_dma = 0) has no windowed form: with that option set a
 * call whose longest sequence exceeds the window is RK_ERR_STATE, nothing launched. */
int rk_llama_set_sliding_window(rk_engine* e, int window);
/* next token of every prompt: first arg-max over the whole vocabulary of the logits at its last position */
int rk_llama_greedy1(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, int32_t* out_tokens);
/* the same logits for a few vocabulary rows only -> out_logits[n_seq][n_out] fp32 (label scoring, tests) */
int rk_llama_last_logits(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                         const int32_t* out_token_ids, int n_out, float* out_logits);
/* Query likelihood (qlm) on a decoder-only model: sequence b is its prompt followed by its labels, the last n_labels[b] tokens
 * being the labels (p = len_b - n_labels[b] prompt tokens).  out_scores[b] = sum over j = 0 .. n_labels[b] - 1 of
 * z[p + j - 1][tok[p + j]] - logsumexp(z[p + j - 1]), z[t] the fp32 logits of position t over the whole vocabulary, natural
 * logarithm, summed in label order: HF's causal-LM loss (shifted labels, -100 on the prompt, reduction "none") summed and negated.
 * The prefill is the one every other rk_llama_* call runs; behind it the final norm of the label-predicting rows, the head GEMM
 * with the log-sum-exp fused into its epilogue and the merge kernel of rk_t5_qlm.  A sequence's score does not depend on what
 * shares its call, bit for bit.  The number of label rows is not bounded by max_seqs.
 * RK_ERR_INVALID for a null pointer, n_labels[b] < 1, n_labels[b] >= len_b (no prompt token in front of the first label) or a
 * token id outside the vocabulary; RK_ERR_STATE on a T5 engine or while a decoding session is open (the session stays intact);
 * RK_ERR_CAPACITY for a batch beyond the prefill's capacities.  A refused call launches nothing.
 * replaces: the decoder-only branch ref: llmrankers/pointwise.py:25-26 refuses ("not supported yet for pointwise"); the T5 form is
 * ref: llmrankers/pointwise.py:73-79 */
int rk_llama_qlm(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq, const int32_t* n_labels,
                 float* out_scores);
/* Greedy continuation of every prompt by up to max_new tokens -> out_tokens[n_seq][max_new].  A row finishes at the
 * first token that is one of eos_ids[n_eos] (n_eos 0..8), or, when max_total > 0, once prompt_len + new == max_total;
 * finished rows emit pad_id; the call stops when every row has finished, remaining columns = pad_id;
 * *out_steps = columns produced.  Prefill once, then ONE new row per sequence and step against a K / V cache (the step is one
 * replayed graph, the arg-max is fed back on the device).  RK_ERR_CAPACITY when the longest prompt + max_new exceeds max_tokens
 * or the batch exceeds the prefill's capacities; RK_ERR_INVALID for max_new <= 0, n_eos outside 0..8, an id outside the
 * vocabulary, a prompt that already reaches max_total; RK_ERR_STATE on a T5 engine.
 * replaces: self.llm.generate(input_ids)  (ref: llmrankers/listwise.py:268) */
int rk_llama_generate(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                      int max_new, int max_total, const int32_t* eos_ids, int n_eos, int pad_id,
                      int32_t* out_tokens, int32_t* out_steps);

/* ---- sampling (hf: generation/logits_process.py TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, softmax, one
 * multinomial draw per token; what the reference's bare self.llm.generate(input_ids), ref: llmrankers/listwise.py:268, does on a
 * checkpoint whose generation_config.json says do_sample: true).  Opt-in: rk_llama_generate and rk_llama_session_admit stay greedy
 * whatever is set here.  temperature 0 = off (greedy), top_k 0 = off, top_p 1 = off.  With temperature > 0 the `_sampled` entry
 * points put a second head between the final norm and the token feedback: the full-vocabulary fp32 logits of the step's rows, then
 * per row z = x / T; keep z >= the min(top_k, vocab)-th largest (ties at the threshold all stay); of those keep id i iff the softmax
 * mass of the kept ids with z_j <= z_i exceeds 1 - top_p (HF's rule on values; the largest always stays); the token is the first kept
 * id in vocabulary order whose running sum of w = exp((x - max x) / T) exceeds u * sum(w), u = (first word of Philox4x32-10 >> 8) *
 * 2^-24 with key = the row's 64-bit seed (low word, high word) and counter = (index of the new token in its sequence, 0, 0, 0).  A
 * row's token is a function of its logit bits, (T, k, p), its seed and that index: not of the batch, the slot, what the slot held
 * before, or whether the step ran eagerly or from a graph (the index is read from the decoders' device positions).  The vocabulary
 * must be a multiple of 4 (the fp32 store of the weight-streaming GEMM; RK_ERR_STATE from the first sampled call otherwise).
 * Distribution parity with HF, not token parity: HF draws from torch's generator.
 * RK_ERR_INVALID for temperature < 0, NaN or infinite, top_k < 0, top_p outside (0, 1]; RK_ERR_STATE on a T5 engine or while a
 * session is open (a session latches the parameters at its open).  May be called after finalize; starts a new graph epoch, as
 * rk_engine_set_option does. */
int rk_llama_set_sampling(rk_engine* e, float temperature, int top_k, float top_p);
/* rk_llama_generate's arguments, checks and contract, plus seeds[n_seq] (null: RK_ERR_INVALID): row b draws its tokens from its own
 * Philox stream seeds[b].  With sampling off: rk_llama_generate bit for bit, the seeds ignored. */
int rk_llama_generate_sampled(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, int n_seq,
                              int max_new, int max_total, const int32_t* eos_ids, int n_eos, int pad_id,
                              int32_t* out_tokens, int32_t* out_steps, const uint64_t* seeds);

/* ---- decoding session: continuous batching for long greedy decodes (the Rank-R1 ranker; the reference serves it through
 * vLLM, ref: llmrankers/setwise.py:406-553, which gives a finished row's place to the next request).  A session has a fixed
 * number of cache slots of max_len positions each; prompts are admitted into free slots while the other slots keep their state;
 * every step decodes one token for all slots through ONE replayed graph.  A prompt's tokens are bit for bit what
 * rk_llama_generate returns for that prompt alone (max_total = 0), whatever shares the session.  One session per engine; while it
 * is open rk_llama_generate, rk_llama_greedy1 and rk_llama_last_logits return RK_ERR_STATE and leave it intact.
 * open: RK_ERR_CAPACITY for n_slots > max_seqs or max_len > max_tokens; RK_ERR_STATE when a session is open.  max_new_cap bounds
 * every request's max_new; eos_ids / pad_id as in rk_llama_generate. */
int rk_llama_session_open(rk_engine* e, int n_slots, int max_len, int max_new_cap, const int32_t* eos_ids, int n_eos, int pad_id);
/* n prompts (ragged, as everywhere) into the free slots slots[n], prompt b to generate up to max_new[b] tokens: ONE prefill,
 * every layer's keys and values to the slots' cache rows, column 0 of each slot = the prefill's arg-max (a slot can finish here:
 * EOS, or max_new 1).  Refused without touching the session: RK_ERR_STATE for a busy slot, RK_ERR_INVALID for a slot out of range
 * or named twice, RK_ERR_CAPACITY for len + max_new > max_len, max_new > max_new_cap or a batch beyond the prefill's capacities. */
int rk_llama_session_admit(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, const int32_t* slots,
                           const int32_t* max_new, int n);
/* rk_llama_session_admit's arguments, checks and contract, plus seeds[n] (null: RK_ERR_INVALID): prompt b draws from seeds[b], in
 * its column 0 and in every later step of its slot; its tokens are bit for bit rk_llama_generate_sampled's for it alone with that
 * seed, whatever shares the session and whatever the slot held before.  A session latches the sampling parameters at
 * rk_llama_session_open: opened with sampling on, every admit is this one and plain rk_llama_session_admit is RK_ERR_STATE; opened
 * with sampling off, this one is RK_ERR_STATE.  A refused admit touches nothing. */
int rk_llama_session_admit_sampled(rk_engine* e, const int32_t* tokens, const int32_t* seq_offsets, const int32_t* slots,
                                   const int32_t* max_new, int n, const uint64_t* seeds);
/* Steps until at least one slot has newly finished, no slot is active, or max_steps steps were issued (one step stays queued
 * ahead of the host's check, so a finish is seen one step late; that step changes nothing for the finished slot).
 * out_finished[n_slots] receives the slots that finished since the last run (at admit included), *out_n_finished their number,
 * *out_steps the steps issued (0 when a finish was already waiting or nothing is active). */
int rk_llama_session_run(rk_engine* e, int max_steps, int32_t* out_finished, int32_t* out_n_finished, int32_t* out_steps);
/* The finished slot's new tokens (the EOS that ended it included) -> out_tokens[*out_n], and the slot is free again.
 * RK_ERR_STATE for a slot that is idle or still decoding, RK_ERR_CAPACITY when cap is too small. */
int rk_llama_session_read(rk_engine* e, int slot, int32_t* out_tokens, int cap, int32_t* out_n);
/* Drains the stream and ends the session (a no-op without one).  Cache and step graph stay for the next open of the same sizes. */
int rk_llama_session_close(rk_engine* e);
/* Drafting by prompt lookup (vLLM's [ngram] speculative mode, hf generate's prompt_lookup_num_tokens): rk_llama_session_open with
 * `draft` = Kd in 1..7 extra rows per slot and step.  Row 0 of a slot is the plain session's row; row j feeds draft token d_j at
 * the next position.  The step's first token is always accepted, the token of row j while d_j equals the token of row j - 1 and no
 * accepted token ended the request (EOS, max_new, max_new_cap).  The drafts are the continuation of the most recent earlier
 * occurrence of the request's last N tokens in its own prompt + output, N from ngram_max down to ngram_min.  The tokens of a
 * request, and where it finishes, are bit for bit the plain session's; only the number of steps differs.  draft = 0 IS
 * rk_llama_session_open.  Every other session call is used as before.
 * RK_ERR_INVALID for draft outside 0..7 or ngram_min / ngram_max outside 1 <= min <= max <= 8; RK_ERR_CAPACITY for
 * n_slots * (draft + 1) > max_seqs (the step's activation rows); RK_ERR_STATE with draft > 0 while sampling is on (greedy only);
 * rk_llama_session_admit_sampled on a drafting session is RK_ERR_STATE. */
int rk_llama_session_open_draft(rk_engine* e, int n_slots, int max_len, int max_new_cap, const int32_t* eos_ids, int n_eos, int pad_id,
                                int draft, int ngram_min, int ngram_max);
/* Any open session.  *out_steps: the steps rk_llama_session_run issued since the open; *out_tokens: the tokens those steps emitted
 * (the admits' first tokens not counted); out_slot_steps[n_slots]: the steps each slot's current request was active in;
 * out_slot_cols[n_slots]: its output column (tokens so far).  0 for an idle slot.  Any pointer may be null. */
int rk_llama_session_stats(rk_engine* e, int64_t* out_steps, int64_t* out_tokens, int32_t* out_slot_steps, int32_t* out_slot_cols);

/* ---- score collection across the GPUs of one node: one process per GPU, one engine per process.
 * The reference has no counterpart (its multi-GPU mode is accelerate's layer placement, ref: pointwise.py:21); this
 * replaces the torch.distributed round trip of a data-parallel caller.  RCCL (librccl.so.1) is dlopen'ed on first use.
 * rank 0 makes the id, the caller ships its 128 bytes to every rank out of band (torchrun's store, a file, MPI ...),
 * then EVERY rank calls rk_comm_init (collective).  max_floats_per_rank bounds the later gathers. */
#define RK_COMM_ID_BYTES 128
int rk_comm_unique_id(uint8_t* out_id, int n_bytes);
int rk_comm_init(rk_engine* e, const uint8_t* id_bytes, int n_bytes, int rank, int world, int max_floats_per_rank);
int rk_comm_world(const rk_engine* e, int* out_rank, int* out_world);
/* max_floats_per_rank of the live communicator (0 without one): the bound every rank checks BEFORE it enters a gather */
int rk_comm_capacity(const rk_engine* e);
/* which RCCL the process bound (dlopen'ed on first use): "<path of the mapped library>|<ncclGetVersion code>" into buf,
 * NUL-terminated; returns the length written or a negative status.  For logs: the torch wheel bundles its own librccl. */
int rk_comm_library_info(char* buf, int n_bytes);
/* ONE ncclAllGather of the slot's device score buffer (the first n_floats fp32 of what rk_t5_score_slot / rk_t5_qlm
 * left there; every rank passes the same n_floats, ranks with fewer scores are read up to their own count by the
 * caller), enqueued on the stream that produces the scores, followed by an async copy to pinned host memory.
 * Returns without synchronising.  rk_comm_read_gathered_slot waits and copies out[world][n_floats]. */
int rk_comm_all_gather_slot(rk_engine* e, int slot, int n_floats);
int rk_comm_read_gathered_slot(rk_engine* e, int slot, float* out, int n_floats_total);
/* Appended form for a rank whose share of the candidates takes several engine calls (more than max_seqs sequences or
 * max_tokens tokens): after each blocking call (rk_t5_score / rk_t5_qlm / rk_t5_qlm_many: scores in slot 0) or rk_t5_score_slot, copy that
 * call's n_floats scores to offset dst_offset of the engine's send buffer (device to device, on the producing stream);
 * then ONE ncclAllGather of the first n_floats of the send buffer (every rank passes the same n_floats = the largest
 * share; capacity = rk_comm_init's max_floats_per_rank); rk_comm_read_appended waits and copies out[world][n_floats].
 * Every rank issues exactly one collective per query, whatever its number of engine calls. */
int rk_comm_append_scores_slot(rk_engine* e, int slot, int n_floats, int dst_offset);
/* the same for n_floats HOST values (small per-passage side data that has to reach every rank with the scores, e.g. the
 * token counts behind the reference's prompt-token counter, ref: llmrankers/pointwise.py:105-114): staged through pinned
 * memory, copied to the send buffer on the stream the gather will run on; the caller's buffer is free on return */
int rk_comm_append_host(rk_engine* e, const float* values, int n_floats, int dst_offset);
int rk_comm_all_gather_appended(rk_engine* e, int n_floats);
int rk_comm_read_appended(rk_engine* e, float* out, int n_floats_total);
int rk_comm_destroy(rk_engine* e);

/* ---- measurement (HIP events on the engine's own stream) ---- */
int rk_timer_begin(rk_engine* e);                 /* record start event on the engine stream */
int rk_timer_end(rk_engine* e, float* out_ms);    /* record stop, synchronise, elapsed ms */
/* per-kernel-class profiling: when enabled every launch is bracketed by an event pair (perturbs throughput;
 * use in a separate pass).  Classes are listed by rk_profile_class_name. */
int rk_profile_enable(rk_engine* e, int on);
int rk_profile_reset(rk_engine* e);
int rk_profile_num_classes(void);
const char* rk_profile_class_name(int cls);
int rk_profile_get(rk_engine* e, int cls, double* total_ms, int64_t* launches, double* flops, double* bytes);
/* Engine options: the defaults are the fast path; every option selects between TESTED implementations of the same arithmetic (the
 * on-device cross-check of a default path: "fold_norm", "gemm_glds", "attn_short", "attn_long", "dec_attn_seq", "dec_cross_mfma",
 * "llama_attn_dma", ...) or is a measurement knob ("overlap", "dec_graph", "gemm_variant", "gemm_split", "gemm_sk", ...).  ONE
 * table holds key, accepted range / set and meaning: kOptions next to rk_engine_set_option in csrc/rk_engine.hip; INTEGRATION.md
 * lists them by purpose.  Returns RK_ERR_INVALID for an unknown key or a value outside the key's range (nothing is applied). */
int rk_engine_set_option(rk_engine* e, const char* key, int value);

/* ---- host-only helpers (no device needed) ---- */
int rk_abi_version(void);
/* T5 relative-position bucket (hf: modeling_t5.py:216-262) as used to build the device bias tables */
int rk_rel_bucket(int relative_position, int bidirectional, int num_buckets, int max_distance);
/* debug: run one GEMM through the engine's kernel on host data (A[M,K] fp16, W[N,K] fp16 -> C[M,N] fp32);
 * use_glds: 1 = tiled kernel with LDS-DMA staging, 0 = register staging, 2 = the weight-streaming (decoder) kernel,
 * 3 = the few-row GEMV kernel (M <= 16, K <= 3072; fails otherwise).  A thin call into rk_debug_gemm_ex. */
int rk_debug_gemm(rk_engine* e, const uint16_t* A, const uint16_t* W, float* C, int M, int N, int K, int use_glds);
/* debug: run ANY call of the engine's GEMM (csrc/rk_engine.hip: struct Gemm -> plan_gemm -> the launchers, nothing of its own)
 * on host data, every output inside guard bands.  The call is described as the engine describes it:
 *   epi     0 store f16, 1 residual f32 (C += acc), 2 GEGLU f16, 3 ReLU f16, 4 store f32, 5 SwiGLU f16 (2 / 5: W rows interleaved
 *           gate / up in groups of 32, N / 2 output columns), 6 argmax blocks (C = float maxima, idx = int first columns, one per
 *           32-column block, ldc = blocks per row), 7 log-sum-exp blocks (C = float2 (max, sum exp(x - max)) per 32-column block,
 *           labels[M] in, xlab[M] out: the label's logit)
 *   family  0 tiled MFMA kernels (engine options gemm_variant / gemm_glds / gemm_sk / gemm_s64_stages / gemm_split choose among
 *           them as they do for the engine), 1 weight-streaming, 2 few-row GEMV
 *   A, W    host fp16, a_elems / w_elems elements; the call reads A[b * bsA + m * lda + k], W[b * bsW + n * ldw + k]
 *   C       host INTERIOR of the output, c_elems elements of the output type (2 bytes for the f16 epilogues, 4 for f32 and argmax,
 *           8 for epi 7), copied to the device as it is (residual input; the caller pre-fills what the call must not touch, e.g.
 *           pad columns of ldc > N); the call's C pointer is interior + c_off
 *   C_out   host, band_rows * ldc + c_elems + band_rows * ldc elements: the WHOLE device allocation after the call - a band in
 *           front and one behind the interior, each band_rows (>= 256, one tile panel) rows of ldc elements, filled with the
 *           byte RK_DEBUG_SENTINEL before the call.  idx_out (epi 6): the same layout in ints.
 *   optional (null / 0 when unused): rowscale[M] or ssq_in[M][nb_in] (folded-RMSNorm consumer; factors_kernel != 0: the engine's
 *           rowscale_kernel turns ssq_in into the row factors in front of the call, as it does for the ping-pong kernel), xraw_out / ssq_out (producer:
 *           fp16 [band | M x N | band] and float [band | M x nb | band] with bands of band_rows rows, sentinel-filled before the call;
 *           ssq_cap = floats ssq_out holds; the plan's nb comes back in out_nb), n_split / split_stride, batch / bsA / bsW / bsC.
 *   plan_only != 0: nothing is allocated or launched, only the out_* fields are filled.
 * Every extent is checked against the sizes given before anything is launched.  A call outside the contract of its kernel family
 * (plan_gemm; DESIGN.md "GEMM contract") fails with RK_ERR_STATE and launches nothing.  out_*: the plan (family, tile variant,
 * rows on the ping-pong kernel, K split, statistics blocks) and what a test needs to predict it (CUs, eps, the xraw scale). */
#define RK_DEBUG_SENTINEL 0xCD
typedef struct rk_debug_gemm_call {
  int epi, family;
  int M, N, K, lda, ldw, ldc;
  const uint16_t* A; int64_t a_elems;
  const uint16_t* W; int64_t w_elems;
  const void* C; int64_t c_elems, c_off;
  void* C_out; int32_t* idx_out;
  int band_rows;
  const float* rowscale;
  const float* ssq_in; int nb_in; int factors_kernel;
  uint16_t* xraw_out; float* ssq_out; int64_t ssq_cap;
  int n_split; int64_t split_stride;
  int batch; int64_t bsA, bsW, bsC;
  const int32_t* labels; float* xlab;
  int plan_only;
  int out_family, out_variant, out_m_pp2, out_ksplit, out_nb, out_n_cu;
  float out_eps, out_xs;
} rk_debug_gemm_call;
int rk_debug_gemm_ex(rk_engine* e, rk_debug_gemm_call* call);
/* debug: the engine's FP8 quantiser (rk_llama_set_weight_fp8: the format) on host data W [N][K] fp16, row stride ldw (K % 16,
 * ldw % 8, ldw >= K).  Any engine.  q_out: the bytes row-major [N][K] (the device order is the engine's own); exp_out: the
 * exponents [N][ceil(K / 128)]; deq_out: the dequantised fp16 matrix [N][K].  Each may be null. */
int rk_debug_quant_fp8(rk_engine* e, const uint16_t* W, int N, int K, int ldw, uint8_t* q_out, int8_t* exp_out, uint16_t* deq_out);
/* debug: rk_debug_gemm_ex with family = 1 (required) on FP8 step weights: W is quantised by the engine's quantiser and the FP8
 * weight-streaming kernel forms the product from the bytes.  Same struct, checks, guard bands and sentinel rules; epilogues 0, 1
 * and 5, one batch (anything else: RK_ERR_STATE, nothing launched).  Its outputs equal, byte for byte, rk_debug_gemm_ex's on
 * rk_debug_quant_fp8's deq_out. */
int rk_debug_gemm_fp8(rk_engine* e, rk_debug_gemm_call* call);
/* debug: n_launch (1 .. 64) launches of ONE described call of the engine's GEMM, back to back on slot 0's encoder stream, with NEW
 * data per launch and optionally beside a background load - what rk_debug_gemm_ex (one launch between host copies on an idle
 * chip) cannot show of the ping-pong kernel's timing-dependent parts: the K-split hand-off (every split launch uses the
 * stream's one workspace: slab and ticket addresses repeat while the data changes) and the row-factor wait.  Same contract as
 * rk_debug_gemm_ex: struct Gemm -> plan_gemm -> the launchers, no kernel and no dispatch of its own; every extent is checked
 * before anything is launched; plan_only != 0 fills the out_* fields only.  No host work, copy or synchronisation between the
 * launches: every operand is uploaded before the first, every output read back after the last.
 *   epi, family, M, N, K, lda, ldw, ldc   the call, as in rk_debug_gemm_call (one batch, no n_split, no producer, epi 0 .. 5)
 *   W        shared, w_elems elements.  A: n_launch x a_elems elements, launch i reads A + i * a_elems.  rowscale (optional):
 *            n_launch x M row factors, launch i reads its own M
 *   C        n_launch interiors of c_elems elements of the output type, copied to the device as they are; C_out: n_launch whole
 *            allocations [band | interior | band] (band_rows >= 256 rows of ldc elements each, RK_DEBUG_SENTINEL-filled before the
 *            first launch): launch i writes its own allocation
 *   accumulate != 0 (epi 1 only, else RK_ERR_INVALID): ONE interior and ONE allocation; every launch adds into it, as successive
 *            layers add into the residual stream
 *   background (bg_per_fg > 0): a second described call (bg_epi 0 / 1 / 3 / 4, bg_family, bg_M, bg_N, bg_K; tight leading
 *            dimensions, operands made up on the host, outputs discarded) whose plan must NOT put rows on the ping-pong kernel
 *            (RK_ERR_INVALID otherwise: the weight-streaming family or another tile variant - the engine's gemm_variant option is
 *            bg_variant for the background's plan and launches); bg_per_fg launches of it go on slot 0's decoder stream per
 *            foreground launch, enqueued in front of it (bg_first != 0) or behind it.  The ping-pong kernel owns whole CUs: a
 *            background grid covering part of the chip delays some of its workgroups.
 * out_*: the foreground's plan, bg_out_*: the background's. */
typedef struct rk_debug_gemm_chain_call {
  int epi, family;
  int M, N, K, lda, ldw, ldc;
  int n_launch, accumulate;
  const uint16_t* A; int64_t a_elems;
  const uint16_t* W; int64_t w_elems;
  const void* C; int64_t c_elems;
  void* C_out;
  int band_rows;
  const float* rowscale;
  int bg_epi, bg_family, bg_M, bg_N, bg_K, bg_variant, bg_per_fg, bg_first;
  int plan_only;
  int out_family, out_variant, out_m_pp2, out_ksplit, out_n_cu;
  int bg_out_family, bg_out_variant, bg_out_m_pp2, bg_out_ksplit;
} rk_debug_gemm_chain_call;
int rk_debug_gemm_chain(rk_engine* e, rk_debug_gemm_chain_call* call);
/* debug: run ANY attention call of the engine (csrc/rk_engine.hip: plan_*attn -> the plan's launcher, no kernel and no dispatch of
 * its own) on host data, every output inside guard bands.  kind selects the plan; heads have the kernels' own width (64 for the T5
 * kinds - 128 on a T5 engine created with d_kv = 128, where kind 1 runs the 128-wide plan (out_kind 3) whatever attn_short / attn_long
 * say, kind 2 is RK_ERR_STATE and kind 3 is unchanged -, the engine's head_dim hd, 64 or 128, for the Llama kinds: a 64-wide Llama engine
 * runs the 64-wide plans, written below with hd = 128); an engine of the other family gets RK_ERR_STATE.
 *   1 T5 encoder         plan_enc_attn: q = packed qkv [T, ldq] (q | k | v at columns 0 | I | 2I, I = 64 H or 128 H), seq_off[n_seq + 1], bias_lut
 *                        [H][257] (entry rel + 128 for rel = key - query clamped to +-128; the table itself, not built from weights),
 *                        out = ctx [T, ldctx].  Options attn_short, attn_heads_per_wg, attn_long, attn_long_nw, attn_long_xcd.
 *   2 T5 decoder         plan_dec_attn.  cross = 0 (causal self-attention): q = fused rows [rows, ldq], keys / values in the same rows
 *                        at columns k_col / v_col, bias_lut or null; rows = n_seq x Ld, or ragged row_off[n_seq + 1] (Ld = the longest),
 *                        or the tree form: tree_rows query rows, row r at position tree_pos[r] sees rows tree_keys[r * Ld + j], j <=
 *                        tree_pos[r].  cross = 1: q [rows, ldq], kv [Tk, ldkv] (k at k_col, v at v_col), seq_off = key offsets, no bias,
 *                        no mask.  out = ctx [rows, ldctx].  Options dec_cross_mfma, dec_attn_seq, xattn_direct.
 *   3 query-side cross   plan_xattn(fuse = false), the chunk kernel and xattn_combine_kernel only (the whole chain, fused form included:
 *                        rk_debug_xattn_chain below): q = qk [M, H, d] (ldq = H d), kv = enc
 *                        [T, d] (ldkv = d), seq_off; query m belongs to sequence row_seq[row0 + m] (n_row_seq entries) or (row0 + m) / Ld;
 *                        out [M, H, d] (ldctx = H d) = sum_t softmax_t(qk_h . enc_t) enc_t.  Option xattn_mfma.
 *   4 Llama prefill      plan_llama_attn: q = rotated qkv [T, ldq] (H query heads, n_kv key heads, n_kv value heads of 128), seq_off,
 *                        out = ctx [T, ldctx].  Options llama_attn_dma, llama_attn_nw (ignored at hd = 64: one kernel, out_kind 2).
 *                        On an engine with a sliding window W (rk_llama_set_sliding_window) the plan is the engine's: a call whose longest
 *                        sequence exceeds W runs the windowed entry of its kernel (out_kind + 4: 5 = LDS-DMA, 6 = 64-wide; with
 *                        llama_attn_dma = 0 at hd = 128 out_kind is 4 and the call is RK_ERR_STATE, nothing launched), any other call the plain one.
 *   5 Llama cached step  plan_llama_dec_attn: q = the step's rows [n_seq, ldq], NOT rotated; cache = K [n_seq][n_kv][P][128] then V, pos[n_seq]
 *                        (< P, < max_pos), cos_t / sin_t [max_pos][64] ([max_pos][32] at hd = 64), qkv_bias [(H + 2 n_kv) 128] fp32 or null; out = ctx [n_seq, H 128]
 *                        (ldctx = H 128); cache_all = the cache afterwards (the row's rotated key and its value appended at pos).  Option llama_dec_r.
 *                        qk_norm (the LAST fields of the call; null = off): Qwen3's q | k head-norm weights [2 x 128] fp32 with qk_eps > 0 - the
 *                        step's entry with the norm (out_kind 2; hd = 128, no window, no qkv_bias: RK_ERR_STATE otherwise).
 *                        On an engine with a sliding window W every call runs the windowed entries (out_kind 1, else 0): row b reads keys
 *                        max(0, pos[b] - W + 1) .. pos[b] and the cache below them is neither read into the result nor written.
 *                        g1 / live (the LAST fields of the call, behind qk_norm / qk_eps; g1 = 0 or 1: the plain call, unchanged): a drafting
 *                        session's step, plan_llama_dec_attn over the n_seq step rows and launch_llama_dec_attn (with g1 / live) as llama_step_rows calls
 *                        them.  n_seq = g1 x the cache's rows (cache = K [n_seq / g1][n_kv][P][hd] then V), step row b belongs to cache row
 *                        b / g1 at pos[b]; live[n_seq]: 1 = the row's rotated key and its value are appended at pos[b] in front of the
 *                        attention, 0 = a dead row (nothing written, its context unspecified).  Every row reads keys <= pos[b] of its cache
 *                        row.  The same out_* fields.  g1 > 8, g1 < 0, n_seq not a multiple of g1 or live = null: RK_ERR_INVALID; the qk_norm /
 *                        window / bias combinations as above.
 *   6 T5 cached step     the self-attention of rk_t5_generate's step, through the launcher run_decoder's cached branch calls: q = the step's
 *                        fused rows [n_seq, ldq] (q | k | v at columns 0 | 64 H | 128 H), cache [n_seq][P][2 x 64 H] (k | v per position),
 *                        pos: ONE value (the kernel reads one device word; outside [0, P): RK_ERR_INVALID, nothing launched), bias_lut;
 *                        out = ctx [n_seq, ldctx]; cache_all = the cache afterwards (row pos holds the step's k and v), bands of
 *                        band_rows x 64 elements.  Option dec_cached_attn: attn_dec_cached_kernel (1, out_kind 1) or kv_append_kernel +
 *                        attn_dec_kernel's tree form (0, out_kind 0, out_grid2 the tree form's).  P <= 8192.  RK_ERR_STATE on a d_kv = 128 engine.
 * Inputs q / kv: host fp16, the WHOLE allocation: band_rows rows in front of and behind the q_rows / kv_rows interior rows, all of ldq /
 * ldkv elements; the caller fills the bands (finite values: a kernel may load a masked row and give it weight 0); the call's pointer is
 * the first interior row.  out: the interior, out_rows x ldctx elements, copied to the device as it is (the caller pre-fills what no
 * kernel may touch); out_all: (out_rows + 2 band_rows) x ldctx elements, the whole device allocation after the call, the bands filled
 * with the byte RK_DEBUG_SENTINEL before it.  cache / cache_all: the same with bands of band_rows x hd elements.
 * plan_only != 0: nothing is allocated or launched, only the out_* fields are filled: out_kind (1: DMA 0 / LONG 1 / TILED 2 / D128 3; 2: the
 * staged kernel NONE 0 / SEQ 1 / ROW 2; 3: part MFMA_FEW 0 / MFMA 1 / VALU16 2 / VALU4 3; 4: dma 0 / 1, or 2 = the 64-wide kernel, + 4 = its windowed entry; 5: 0, or 1 = the windowed entries), out_tparam (the kernel's template
 * parameter: wave groups, waves, heads per workgroup or R), out_grid (the first kernel's), out_grid2 (the tiled / staged / merge
 * kernel's), out_lds, out_staged, out_mfma, out_part, out_R, out_nch, out_skip_long, out_heads_per_wg, out_n_cu.
 * Every extent is checked against the sizes given before anything is launched (RK_ERR_INVALID); a shape no kernel of the plan takes
 * fails with RK_ERR_STATE and launches nothing. */
typedef struct rk_debug_attn_call {
  int kind;
  int n_seq, H, n_kv, Ld, cross, M, row0, d, P;
  int ldq, ldkv, ldctx, k_col, v_col, band_rows;
  const uint16_t* q; int64_t q_rows;
  const uint16_t* kv; int64_t kv_rows;
  const int32_t* seq_off; const int32_t* row_off;
  const int32_t* tree_keys; const int32_t* tree_pos; int tree_rows;
  const int32_t* row_seq; int n_row_seq;
  const int32_t* pos;
  const float* bias_lut;
  const float* cos_t; const float* sin_t; int max_pos;
  const float* qkv_bias;
  const uint16_t* out; int64_t out_rows; uint16_t* out_all;
  const uint16_t* cache; uint16_t* cache_all;
  int plan_only;
  int out_kind, out_tparam, out_grid[3], out_grid2[3], out_lds, out_staged, out_mfma, out_part, out_R, out_nch, out_skip_long,
      out_heads_per_wg, out_n_cu;
  const float* qk_norm; float qk_eps;
  int g1; const int32_t* live;
} rk_debug_attn_call;
int rk_debug_attn(rk_engine* e, rk_debug_attn_call* call);
/* debug: the WHOLE query-side cross-attention chain of one T5 decoder layer on host data (csrc/rk_engine.hip: struct XAttnChain ->
 * run_xattn_chain, the function run_decoder calls: the fuse decision, the q projection, the loop over blocks of rows, plan_xattn
 * and the launches of every block; no kernel and no dispatch of its own).  Fused (fuse_asked != 0 and d % 128 == 0): dec_cross_qk_kernel,
 * the chunk kernel, dec_cross_cv_kernel (beyond DECV_MAXCH chunks: xattn_combine_kernel + the W_v GEMM per head); else the five-launch
 * form (q GEMM, W_k^T GEMM per head, chunk kernel, xattn_combine_kernel, W_v GEMM per head) - out_fused says which ran.
 *   x [M, ldx] fp16, wq / wk / wv [H 64, d] fp16 in HF layout ([H 128, d] on an engine created with d_kv = 128, which always runs the
 *   five-launch form - out_fused = 0 whatever fuse_asked says - and takes ldo >= 128 H) (the call regroups W_k as rk_engine_finalize does), enc: the WHOLE
 *   allocation, band_rows rows in front of and behind the enc_rows interior rows of d elements, bands filled by the caller with finite
 *   values; seq_off[n_seq + 1]; decoder row m belongs to sequence row_seq[row0 + m] (n_row_seq entries) or (row0 + m) / Ld.
 *   Norm fold of the q projection: rowscale[M], or ssq_in[M][nb_in] (block sums of squares of x / out_xs: the factor is
 *   rsqrt(sum / d + out_eps) / out_xs, out_eps = the engine's layer_norm_epsilon), or neither: factor 1.
 *   ctx: optional interior [M, ldo] the output starts from (ldo >= 64 H: pad columns are the caller's), else sentinel bytes.
 * Outputs, each the whole device allocation after the call, filled with the byte RK_DEBUG_SENTINEL before it, a band in front and behind:
 *   qk_all   (band_rows + M + band_rows) x H d fp16
 *   part_all out_n_blocks x (band_rows H d + R nch H d + band_rows H d) fp32, stat_all out_n_blocks x (band_rows H 2 + R nch H 2 + band_rows H 2)
 *            fp32, xctx_all out_n_blocks x (band_rows + R + band_rows) x H d fp16, R = min(out_block_rows, M): the workspaces have the size
 *            of one block of the row loop, are refilled with the sentinel in front of every block and copied out behind it; ws_fill != 0:
 *            the interiors of part and stat are refilled with this 32-bit pattern instead (0x7F800000, +inf: a chunk no kernel may read
 *            turns its row into NaN if one does - the engine's workspaces are never initialised)
 *   ctx_all  (band_rows + M + band_rows) x ldo fp16
 * plan_only != 0: nothing is allocated or launched, only the out_* fields are filled: out_fused, out_block_rows / out_n_blocks (the row
 * loop), out_nch, out_n_cu, out_eps / out_xs, and per [first block, last block]: out_qk_R, out_qk_CS (0 when the W_k^T GEMM runs), out_part_kind
 * (MFMA_FEW 0 / MFMA 1 / VALU16 2 / VALU4 3), out_part_grid, out_fuse_cv, out_cv_R (0 when the merge is not fused).
 * The five-launch form's q GEMM runs on the weight-streaming family for Ld <= 4 and on the tiled family beyond, as run_decoder's does
 * (its few-row GEMV family, a choice of the whole decoder pass, is not reachable here); where that GEMM plans onto the persistent
 * ping-pong kernel, which takes ready-made row factors, ssq_in is refused with RK_ERR_STATE: pass rowscale.
 * Every extent is checked before anything is launched: RK_ERR_INVALID for d not a multiple of 32, a row whose sequence index is out of
 * range, leading dimensions or enc_rows too small; RK_ERR_STATE for more than 65536 keys in a sequence or a GEMM of the unfused form
 * outside its kernel family's contract; nothing is launched after any of them. */
typedef struct rk_debug_xattn_chain_call {
  int M, Ld, H, d, n_seq, row0, ldx, ldo, band_rows, fuse_asked;
  const uint16_t* x;
  const uint16_t* wq; const uint16_t* wk; const uint16_t* wv;
  const uint16_t* enc; int64_t enc_rows;
  const int32_t* seq_off; const int32_t* row_seq; int n_row_seq;
  const float* rowscale; const float* ssq_in; int nb_in;
  const uint16_t* ctx;
  uint16_t* qk_all; float* part_all; float* stat_all; uint16_t* xctx_all; uint16_t* ctx_all;
  uint32_t ws_fill;
  int plan_only;
  int out_fused, out_block_rows, out_n_blocks, out_nch, out_n_cu;
  int out_qk_R[2], out_qk_CS[2], out_part_kind[2], out_part_grid[2][3], out_fuse_cv[2], out_cv_R[2];
  float out_eps, out_xs;
} rk_debug_xattn_chain_call;
int rk_debug_xattn_chain(rk_engine* e, rk_debug_xattn_chain_call* call);
/* debug: run ONE launch of a row kernel or device state machine (csrc/misc_kernels.h, the rope and cache-fill kernels of
 * csrc/llama_kernels*.h) on host data through the launcher the production path calls (csrc/rk_engine.hip: launch_rmsnorm, launch_embed,
 * launch_rope, launch_kv_fill, ...; no kernel, grid rule or dispatch of its own), every output inside guard bands.  Works on an engine
 * of either family: every width comes from the call, none from the engine.
 *   in[i]   an input: data = the WHOLE allocation of `bytes` bytes, the kernel's pointer = data + off (off a multiple of 16).  What lies
 *           in front of off and behind the interior is the caller's band (finite values): a table gets a band row in front and behind.
 *           data = null: the kernel gets a null pointer (optional operands only).
 *   out[i]  an output: interior = `bytes` bytes copied to the device as they are (the caller pre-fills what the kernel must not
 *           touch; for an in-place operand or a state word this is the input); all = n_steps x (band + bytes + band) bytes, the WHOLE
 *           device allocation after each launch, the two bands (band bytes each, a multiple of 16, >= 64) filled with the byte
 *           RK_DEBUG_SENTINEL before the first launch.  n_steps is 1 except for op 10.
 * op and operands (fp16 = uint16 bit patterns, f32 = float, i32 = int32):
 *   1 embed          rows, d (multiple of 8), vocab, kind = 1 folded-norm form / 0 plain, eps, xs.  in0 ids i32[rows] (any value: the kernel
 *                    clamps), in1 table fp16 [vocab][d].  out0 out f32 [rows][d], out1 xraw fp16 [rows][d], out2 rowscale f32 [rows]
 *                    (kind 0: the kernel gets null for both and they keep their pre-fill).
 *   2 rowscale       rows, nb, d, eps, xs.  in0 ssq f32 [rows][nb].  out0 f32 [rows].
 *   3 rmsnorm        rows, d (multiple of 4, <= 4096), src_rows, eps, out_scale.  in0 x f32 [src_rows][d], in1 w f32 [d], in2 row_map
 *                    i32[rows] (each in [0, src_rows)) or null.  out0 fp16 [rows][d].  out_tparam = NV.
 *   4 head_rows      rows (= n_seq), n_out, d (multiple of 8), vocab.  in0 x fp16 [rows][d], in1 head fp16 [vocab][d], in2 out_ids
 *                    i32[n_out] (each in [0, vocab)).  out0 f32 [rows][n_out].
 *   5 pair_verdict   rows (= n_seq >= 2), d, vocab, false_id, true_id.  in0 x, in1 head as for 4.  out0 f32 [3 rows + rows / 2].
 *   6 argmax_blocks  rows, nb (= n_blocks).  in0 bval f32 [rows][nb], in1 bidx i32 [rows][nb].  out0 i32 [rows].
 *   7 qlm_lse        rows (= n_seq), nb (= nblk), n_pos.  in0 stats f32 [R][nb][2], in1 xlab f32 [R], in2 row_off i32[rows + 1] (growing
 *                    from >= 0; R = row_off[rows]) or null (R = rows n_pos), in3 out_idx i32[rows] (each in [0, rows)) or null.  out0 f32 [rows].
 *   8 rope           rows (= T), H, n_kv, hd (64 or 128), ld (multiple of 8, >= (H + 2 n_kv) hd), max_pos.  in0 pos i32[T] (each in
 *                    [0, max_pos)), in1 cos_t f32 [max_pos][hd / 2], in2 sin_t, in3 bias f32 [(H + 2 n_kv) hd] or null.  out0 qkv fp16
 *                    [T][ld], rotated in place.  out_tparam = hd, out_variant = 1 with bias.
 *   9 kv_fill        rows (= n_seq), H, n_kv, hd, ld, P, n_slots.  in0 qkv fp16 [T][ld], in1 seq_off i32[rows + 1] (growing from 0, T =
 *                    seq_off[rows], the longest sequence >= 1), in2 slots i32[rows] (any value: the kernel skips what is outside [0, n_slots))
 *                    or null (then the cache has `rows` rows).  out0 cache fp16: K [cache rows][n_kv][P][hd], then V.  out_tparam = hd,
 *                    out_variant = 1 with a slot map.
 *  11 rope_qkn       op 8 with Qwen3's q / k head norm (rope128_qkn_kernel): hd = 128, eps > 0, in3 norm weights f32 [2 x 128] (q | k,
 *                    required); the value heads stay as they are.  out_tparam = 128, out_variant = 2.
 *  10 advance        kind 0 greedy_advance_kernel, 1 llama_advance_kernel, 2 llama_session_advance_kernel; rows (= n_seq / n_slots),
 *                    n_steps >= 1 launches, one per scripted arg-max row: in0 argmax i32 [n_steps][R], R = rows (kind 2: max(rows, max_admit)).
 *                    The interiors are the initial state; all[s] is the complete state after launch s.
 *                    kind 0: dec_len, max_new; in1 prefix i32[dec_len]; out0 st i32[4] (st[0] >= 0), out1 done i32[rows], out2 out
 *                            i32 [rows][max_new], out3 next_ids i32[rows].
 *                    kind 1: in1 len i32[rows]; out0 st i32[16] (st[0] >= 0, n_eos = st[3] in 0..8, max_new = st[4] > 0), out1 done, out2 pos,
 *                            out3 out i32 [rows][st[4]], out4 next_ids.
 *                    kind 2: in1 admit script i32 [n_steps][1 + 3 max_admit] or null: per step n_admit (-1: a plain step, the kernel gets
 *                            null; else 0..max_admit) and then slot[n_admit] | len[n_admit] | max_new[n_admit] packed; out0 st i32[16]
 *                            (n_eos = st[2] in 0..8, cap = st[4] > 0), out1 len, out2 col (each >= 0), out3 max_new, out4 done, out5 pos,
 *                            out6 out i32 [rows][cap], out7 next_ids (all i32[rows]).
 * plan_only != 0: nothing is allocated or launched, only out_grid, out_tparam and out_variant are filled (from the launchers' own grid
 * functions).  Every extent is checked against the sizes given before anything is launched: RK_ERR_INVALID, nothing launched. */
typedef struct rk_debug_rows_in { const void* data; int64_t bytes, off; } rk_debug_rows_in;
typedef struct rk_debug_rows_out { const void* interior; int64_t bytes, band; void* all; } rk_debug_rows_out;
typedef struct rk_debug_rows_call {
  int op, kind;
  int rows, d, vocab, src_rows, n_out, nb, n_pos, H, n_kv, hd, ld, P, n_slots, max_pos, false_id, true_id, dec_len, max_new, n_steps, max_admit;
  float eps, xs, out_scale;
  rk_debug_rows_in in[4];
  rk_debug_rows_out out[8];
  int plan_only;
  int out_grid[3], out_tparam, out_variant;
} rk_debug_rows_call;
int rk_debug_rows(rk_engine* e, rk_debug_rows_call* call);
/* debug: the two state kernels of a DRAFTING session (csrc/misc_kernels.h: llama_session_advance_draft_kernel, the accept machine, and
 * draft_lookup_kernel, the proposer) on host state, through launch_session_advance_draft and launch_draft_lookup in the order the
 * session calls them; no kernel, grid rule or dispatch of its own.  Works on an engine of either family.
 *   state[i]  the session's int arrays, each a device allocation of its own between sentinel bands (rk_debug_rows' out[i]: interior = the
 *             initial state, all = n_steps x (band + bytes + band) bytes, the whole allocation after every step), in this order:
 *             st[16] (finishes, pad, n_eos, max_len, cap, ngram_min, ngram_max, 0, eos[8]), len, col, max_new, done (all [n_slots]),
 *             out [n_slots][cap], rnext, rpos, rlive (all [n_slots][g1]), dlen, nstep, tabn (all [n_slots]), tab [n_slots][cap],
 *             hist [n_slots][max_len].  bytes is exactly the array's size.
 *   script    i32 [n_steps][rec], rec = 4 + A + 3 max_admit + (max_admit + 1) + max_tokens, A = max(n_slots g1, max_admit); a record is
 *             kind | n | slot | 0 | argmax[A] | admit[3 max_admit] | seq_off[max_admit + 1] | tokens[max_tokens]:
 *             kind 0, a step: argmax[n_slots g1]; the accept machine without an admit list, then the proposer.
 *             kind 1, an admit: n = n_admit in 0..max_admit, admit = slot[n] | len[n] | max_new[n] packed, prompt r = tokens[seq_off[r] ..
 *                     seq_off[r] + len[r]), argmax[n_admit]; the accept machine with the list, then the proposer (session_admit's pair).
 *             kind 2, a table change: tab[slot] = tokens[0, n) and tabn[slot] = n (n = -1: back to the lookup), then the proposer alone
 *                     (rk_debug_session_drafts).
 * Checked before anything is allocated or launched (RK_ERR_INVALID): n_eos <= 8, 1 <= ngram_min <= ngram_max <= 8, 1 <= g1 <= 8; for every
 * active slot of the initial state and every entry of every admit len >= 1, 1 <= max_new <= cap, len + max_new <= max_len (initially
 * also 0 <= col < max_new, 0 <= dlen < g1, tabn in -1..cap); a prompt inside the record's tokens; no slot twice in one admit; a table of
 * at most min(cap, max_tokens) tokens for a slot in range.  An admitted slot id outside [0, n_slots) is allowed: the kernels skip it. */
#define RK_DEBUG_DRAFT_ARRAYS 14
typedef struct rk_debug_draft_steps_call {
  int n_slots, g1, n_steps, max_admit, max_tokens;
  const int32_t* script; int64_t script_ints;
  rk_debug_rows_out state[RK_DEBUG_DRAFT_ARRAYS];
} rk_debug_draft_steps_call;
int rk_debug_draft_steps(rk_engine* e, rk_debug_draft_steps_call* call);
/* debug: the FP8 K / V cache's quantiser (rk_llama_set_kv_fp8: the format) on n host vectors x [n][128] fp16, through the device
 * helper every cache writer calls: q_out [n][128] bytes, exp_out [n] exponents, deq_out [n][128] the dequantised fp16 values (null:
 * not wanted).  A finalized Llama-family engine. */
int rk_debug_kv8_quant(rk_engine* e, const uint16_t* x, int n, uint8_t* q_out, int8_t* exp_out, uint16_t* deq_out);
/* debug: one decoding step's attention on an FP8-cache engine (rk_llama_set_kv_fp8; RK_ERR_STATE on another) on host operands, beside
 * rk_debug_attn kind 5 and with its operands: qkv [n_seq][ld] the step's fused rows (not rotated), pos [n_seq], cos_t / sin_t
 * [max_pos][64], qkv_bias / qk_norm (+ qk_eps) or null, g1 / live as there (g1 > 1: the drafting step - append, then the KEYS form),
 * the window the engine's.  cache: an fp16 cache [2][n_seq / g1][n_kv][P][128] (K then V) that the engine's quantiser converts
 * into the layout of `mode` before the step: 0 = bytes and exponents, 1 = the fp16 layout holding the dequantised values (option
 * llama_kv_fp8 = 0's cache).  No launch code of its own: plan_llama_dec_attn and the production launchers.
 * Outputs, each between guard bands by rk_debug_rows_out's rule (bytes exact): ctx fp16 [n_seq][H 128]; part fp32
 * [n_seq][H][out_nch][132], the chunk partials (132 = 128 accumulators, maximum, sum, 2 unused; a chunk no workgroup wrote keeps
 * its pre-fill); cache_out, the cache as the step left it - mode 0: K bytes | V bytes | K exponents [..][out_pe] | V exponents
 * (2 plane + 2 rows n_kv out_pe bytes, plane = rows n_kv P 128), mode 1: the fp16 cache (4 plane bytes).
 * plan_only != 0: only out_R, out_nch and out_pe are filled. */
typedef struct rk_debug_kv8_step_call {
  int n_seq, H, n_kv, P, ld, max_pos, g1, mode, plan_only;
  float qk_eps;
  const uint16_t* qkv; const int32_t* pos; const float* cos_t; const float* sin_t; const float* qkv_bias; const float* qk_norm;
  const int32_t* live; const uint16_t* cache;
  rk_debug_rows_out ctx, part, cache_out;
  int out_R, out_nch, out_pe;
} rk_debug_kv8_step_call;
int rk_debug_kv8_step(rk_engine* e, rk_debug_kv8_step_call* call);
/* measurement: average ms per launch of the engine's GEMM kernel at one shape (epi = 0 store f16, 1 residual f32,
 * 2 GEGLU, 3 ReLU, 4 store f32), random operands, `iters` back-to-back launches timed with HIP events */
int rk_debug_gemm_bench(rk_engine* e, int M, int N, int K, int epi, int iters, float* out_ms);
/* debug: copy an internal activation buffer to the host as fp32. name: "enc_hidden" [T,d], "enc_out" [T,d],
 * "qkv" [T,3I], "ctx" [T,I], "dec_hidden" [B*Ld,d], "llama_last" [n_seq,hidden] (the final-normed last rows of the most recent
 * Llama call: after rk_llama_generate, the rows the last step's head read; after rk_llama_session_run, its n_slots rows),
 * "lkv" (RAW, no conversion: the bytes of the Llama K / V cache as it lies on the device, four per float slot - fp16 planes, or on
 * an FP8-cache engine the layout at rk_llama_set_kv_fp8; rk_debug_buffers gives its capacity in 2-byte elements). Returns number of floats written or a negative status. */
int64_t rk_debug_read(rk_engine* e, const char* name, float* out, int64_t max_floats);
/* debug: the table of decoder graphs and what became of every decoder chain since the engine was created (csrc/rk_engine.hip:
 * run_graphed, the one function every chain of rk_t5_score / _compare / _greedy / _greedy2 / _generate, rk_llama_generate and
 * rk_llama_session_run goes through; rk_t5_qlm and rk_t5_qlm_many launch outside it and count nowhere).  A chain is keyed by its
 * kind, slot, shapes, buffer generations and the options epoch (every rk_engine_set_option starts a new epoch: no graph captured
 * under other options is ever replayed).  Per key: the first sighting runs eagerly, the second is captured, instantiated and
 * launched, later ones replay; a key whose capture fails runs eagerly from then on.  Every call is exactly one of
 *   eager      the chain's kernels were launched one by one: dec_graph = 0, profiling on, a first sighting, a failed key
 *   captures   the chain was captured, instantiated and launched as a graph
 *   replays    the key's graph was launched
 * and failed counts the keys marked failed (each also ran eagerly, unless the chain itself returned an error).
 * The table holds at most RK_GRAPH_CACHE_KEYS keys: the new key that would pass the bound erases every other entry, after
 * draining the streams a graph may be replaying on; evictions counts the instantiated graphs destroyed that way.  n_keys = entries
 * in the table (<= max_keys = RK_GRAPH_CACHE_KEYS at every return), n_ready = entries that hold an instantiated graph.
 * Host state only: nothing is launched or waited for. */
#define RK_GRAPH_CACHE_KEYS 256
typedef struct rk_debug_graph_stats_t {
  int n_keys, n_ready, max_keys;
  int64_t eager, captures, replays, failed, evictions;
} rk_debug_graph_stats_t;
int rk_debug_graph_stats(rk_engine* e, rk_debug_graph_stats_t* out);
/* debug (tests, tools/bench_llama_draft.py): the proposer of `slot` of the open drafting session takes its drafts from the caller's
 * continuation table tokens[n], indexed by output column (the draft for column c is tokens[c]), in place of the n-gram lookup, so
 * that acceptance is a function of the table whatever a toy model emits.  It holds until it is replaced; tokens = null, n = 0:
 * back to the lookup.  In force from the slot's next admit or step.  RK_ERR_STATE without a drafting session, RK_ERR_CAPACITY for
 * n > max_new_cap. */
int rk_debug_session_drafts(rk_engine* e, int slot, const int32_t* tokens, int n);
/* debug: the engine's grown buffers - device memory that is freed and reallocated between calls when a call needs more of it
 * (csrc/rk_engine.hip: Grown<T>::reserve) - and the move counters that stand in the graph keys.  Per buffer its device address
 * (0: never allocated) and its capacity in elements, in the order of RK_DEBUG_BUFFER_NAMES; amax_gen counts the moves of amax_val
 * and amax_idx (two per growth), kv_gen those of kv_cache, lkv_gen those of lkv, lpart and lints; logits and gen_buf have no
 * counter here (the graphs of the sampled Llama steps hold logits and carry an internal counter of its moves in their keys; a move
 * shows as a new address; gen_buf is sized by the engine's capacities alone and is allocated once).  With it a test can
 * say which buffer a call moved.  Host state only: nothing is launched or waited for. */
#define RK_DEBUG_N_BUFFERS 8
#define RK_DEBUG_BUFFER_NAMES "logits amax_val amax_idx kv_cache gen_buf lkv lpart lints"
typedef struct rk_debug_buffers_t {
  uint64_t addr[RK_DEBUG_N_BUFFERS];
  uint64_t cap[RK_DEBUG_N_BUFFERS];
  int amax_gen, kv_gen, lkv_gen;
} rk_debug_buffers_t;
int rk_debug_buffers(rk_engine* e, rk_debug_buffers_t* out);
/* debug: sample_rows_kernel (csrc/sampling_kernels.h) alone, through the launcher the sampling head calls, on host data.  Works on
 * an engine of either family and needs no rk_llama_set_sampling: everything comes from the call.
 *   logits      host fp32 [logit_rows][V], 1 <= V <= 2^23 (any such V: the kernel itself has no multiple-of-4 rule); row r of the call reads logits
 *               row r % logit_rows, so many (seed, index) pairs can be drawn from a few rows in one launch (1 <= logit_rows <= rows)
 *   temperature > 0, top_k >= 0 (0 or >= V: off), top_p in (0, 1] (1: off)
 *   seeds[rows], index[rows] (>= 0): the row's Philox key and counter word
 *   out_token[rows]; out_kept_k[rows], out_kept_p[rows] (optional): the ids kept after top-k, and after top-p
 * RK_ERR_INVALID for anything outside that, nothing launched. */
typedef struct rk_debug_sample_call {
  int rows, logit_rows, V;
  float temperature; int top_k; float top_p;
  const float* logits;
  const uint64_t* seeds; const int32_t* index;
  int32_t* out_token; int32_t* out_kept_k; int32_t* out_kept_p;
} rk_debug_sample_call;
int rk_debug_sample(rk_engine* e, rk_debug_sample_call* call);

#ifdef __cplusplus
}
#endif
#endif /* RK_ENGINE_H */
