// The rk_debug_* entry points (include/rk_engine.h): the tests' way to the device.  Part of rk_engine.hip's translation unit
// (included at its end): no kernel, plan or launcher of their own - they upload host operands, call the engine's own plan_* /
// launch_* / gemm() / run_xattn_chain and copy the outputs back with their guard bands (debug_bands.h).
#include "debug_bands.h"

namespace {

// a device allocation [band | interior | band] of a DebugScratch: sentinel bytes everywhere, the interior optionally from the host
struct Banded {
  char* all = nullptr;
  BandSpan span{0, 0};
  template <class T = char> T* interior() const { return all ? (T*)(all + span.interior()) : nullptr; }
  size_t total() const { return span.all(); }
  hipError_t refill(hipStream_t st) const { return hipMemsetAsync(all, RK_DEBUG_SENTINEL, total(), st); }
  hipError_t read_back(void* host_dst) const { return hipMemcpy(host_dst, all, total(), hipMemcpyDeviceToHost); }
};

// The device memory of ONE debug call.  Everything alloc / up / banded hand out, and every engine-owned allocation made while
// the owner lives (the FP8 quantiser's), is given back by the destructor, after the device has gone idle: a plain return is
// right on every path.  The first failed allocation or upload is kept: failed() after a block of them, before any pointer is used.
struct DebugScratch {
  rk_engine* const e;
  const char* const name;                                  // the call's name, the prefix of its RK_ERR_HIP messages
  DebugScratch(rk_engine* e, const char* name) : e(e), name(name), n_own(e->allocs.size()) {}
  DebugScratch(const DebugScratch&) = delete;
  DebugScratch& operator=(const DebugScratch&) = delete;
  ~DebugScratch() {
    hipDeviceSynchronize();
    for (void* p : dev) hipFree(p);
    while (e->allocs.size() > n_own) { hipFree(e->allocs.back()); e->allocs.pop_back(); }
  }
  // n elements; fill >= 0: that byte all over them
  template <class T>
  T* alloc(size_t n, int fill = -1) {
    void* p = nullptr;
    if (bad || hipMalloc(&p, n ? n * sizeof(T) : 16) != hipSuccess) { bad = true; return nullptr; }
    dev.push_back(p);
    if (fill >= 0 && hipMemset(p, fill, n * sizeof(T)) != hipSuccess) { bad = true; return nullptr; }
    return (T*)p;
  }
  // n elements of T from the host (the call structs hand fp16 operands over as uint16_t or void)
  template <class T>
  T* up(const void* src, size_t n) {
    T* p = alloc<T>(n);
    if (p && hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { bad = true; return nullptr; }
    return p;
  }
  Banded banded(BandSpan span, const void* host_interior = nullptr) {
    Banded b{alloc<char>(span.all(), RK_DEBUG_SENTINEL), span};
    if (b.all && host_interior && hipMemcpy(b.interior(), host_interior, span.bytes, hipMemcpyHostToDevice) != hipSuccess) { bad = true; b.all = nullptr; }
    return b;
  }
  Banded banded(const rk_debug_rows_out& o) { return banded(BandSpan{(size_t)o.bytes, (size_t)o.band}, o.interior); }
  // RK_OK, or the call's RK_ERR_HIP when an allocation or upload since the construction failed
  int failed() const { return bad ? fail(e, RK_ERR_HIP, "%s: device allocation or upload failed", name) : RK_OK; }
  // failed(), and the device idle behind the (synchronous) uploads and fills: what stands in front of the first launch
  int ready() const { return bad ? failed() : (hipDeviceSynchronize() != hipSuccess ? hip_failed("hipDeviceSynchronize()") : RK_OK); }
  int hip_failed(const char* what) const { return fail(e, RK_ERR_HIP, "%s: %s", name, what); }

 private:
  std::vector<void*> dev;
  const size_t n_own;
  bool bad = false;
};
#define DBG_HIP(ds, x) do { if ((x) != hipSuccess) return (ds).hip_failed(#x); } while (0)

// step s of a call's rk_debug_rows_out array: every allocation that is there, whole, into its `all`
hipError_t read_back_step(const Banded* dev, const rk_debug_rows_out* out, int n, int s) {
  for (int i = 0; i < n; ++i) {
    if (!dev[i].all) continue;
    const hipError_t rc = dev[i].read_back((char*)out[i].all + (size_t)s * dev[i].total());
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}

// what a Gemm is planned with before anything is allocated: a pointer only counts as aligned / present in plan_gemm
half_t* const plan_dummy = (half_t*)(uintptr_t)256;

GemmFamily family_of(int f) { return f == 2 ? GEMM_GEMV : (f == 1 ? GEMM_STREAM : GEMM_TILED); }

// a plan's family, tile variant, rows on the ping-pong kernel and K split, as the out_* ints of a call report them
void plan_out_ints(const GemmPlan& p, int* family, int* variant, int* m_pp2, int* ksplit) {
  *family = (int)p.family; *variant = p.variant; *m_pp2 = p.m_pp2; *ksplit = p.m_pp2 > 0 ? p.ks_pp2 : p.ksplit;
}

// n fp16 test operands in [-1, 1] from a linear congruential generator
std::vector<half_t> lcg_halfs(size_t n, uint32_t x) {
  std::vector<half_t> h(n);
  for (size_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; h[i] = (half_t)(((int)(x >> 16) % 2001 - 1000) * 1e-3f); }
  return h;
}

}  // namespace

extern "C" {

// debug: one Gemm call on host data, every output between sentinel bands (include/rk_engine.h).  No launch code of its own: it
// builds the Gemm and calls gemm().  fp8 (rk_debug_gemm_fp8): W also goes through the engine's quantiser and the call carries the bytes.
static int debug_gemm(rk_engine* e, rk_debug_gemm_call* q, bool fp8) {
  if (!e || !q) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if (fp8 && q->family != 1) return fail(e, RK_ERR_INVALID, "debug gemm fp8: family must be 1 (the weight-streaming kernels read FP8 step weights)");
  const int epi = q->epi, M = q->M, N = q->N, K = q->K, batch = q->batch > 0 ? q->batch : 1;
  if (epi < 0 || epi > EPI_LSE_F32 || q->family < 0 || q->family > 2 || M <= 0 || N <= 0 || K <= 0 || q->lda <= 0 || q->ldw <= 0 || q->ldc <= 0 ||
      q->n_split < 0 || q->split_stride < 0 || q->bsA < 0 || q->bsW < 0 || q->bsC < 0 || q->c_off < 0 || (long)M * batch > (1 << 22))
    return fail(e, RK_ERR_INVALID, "debug gemm: bad shape");
  const bool gated = EPI_IS_GATED(epi), blocks = epi == EPI_ARGMAX_F32 || epi == EPI_LSE_F32;
  const bool f16 = epi == EPI_STORE_F16 || epi == EPI_RELU_F16 || gated;
  const size_t celt = f16 ? 2 : (epi == EPI_LSE_F32 ? 8 : 4);
  const GemmFamily fam = family_of(q->family);
  const bool producer = q->xraw_out || q->ssq_out, planning = q->plan_only != 0;
  // the plan first (pointers only count as aligned / present): a call outside the contract stops here, before any allocation
  half_t* const dummy = plan_dummy;
  Gemm c(PC_OTHER, epi, dummy, q->lda, dummy, q->ldw, (char*)dummy + (size_t)q->c_off * celt, q->ldc, M, N, K);
  c.on(fam).heads(batch, q->bsA, q->bsW, q->bsC).split(q->n_split, q->split_stride);
  if (q->rowscale || (q->ssq_in && q->factors_kernel)) c.fold.rowscale = (const float*)dummy;
  else if (q->ssq_in) { c.fold.ssq_in = (const float*)dummy; c.fold.nb_in = q->nb_in; }
  if (q->ssq_in && q->nb_in <= 0) return fail(e, RK_ERR_INVALID, "debug gemm: ssq_in without nb_in");
  if (producer) { c.fold.xraw = dummy; c.fold.ssq = (float*)dummy; }
  c.lse((const int*)dummy, (float*)dummy).argmax((int*)dummy);
  if (fp8) c.w8(GemmW8{(const uint8_t*)dummy, (const int8_t*)dummy, fp8_ldq(K), fp8_lde(K)});
  hipStream_t st = e->slots[0].se;
  const GemmPlan p = plan_gemm(e, c, st);
  plan_out_ints(p, &q->out_family, &q->out_variant, &q->out_m_pp2, &q->out_ksplit);
  q->out_nb = p.nb; q->out_n_cu = e->n_cu; q->out_eps = e->d.eps; q->out_xs = RK_XRAW_SCALE;
  if (p.family == GEMM_NONE)
    return fail(e, RK_ERR_STATE, "no kernel of family %d takes the GEMM M=%d N=%d K=%d (epilogue %d, batch %d): %s", (int)fam, M, N, K, epi, batch, p.why ? p.why : "");
  if (fp8 && !p.w8) return fail(e, RK_ERR_STATE, "debug gemm fp8: the plan does not put the call on the weight-streaming family (option gemm_skinny)");
  if (planning) return RK_OK;
  // extents, from the addressing of the call, against what the caller gave
  if (!q->A || !q->W || !q->C || !q->C_out || q->band_rows < 256) return fail(e, RK_ERR_INVALID, "debug gemm: A, W, C, C_out and band_rows >= 256");
  const long nsb = q->n_split > 0 ? (N + q->n_split - 1) / q->n_split : 1;
  const long width = blocks ? (N + 31) / 32 : (q->n_split > 0 ? q->n_split : (gated ? N / 2 : N));
  const long a_need = (long)(batch - 1) * q->bsA + (long)(M - 1) * q->lda + K, w_need = (long)(batch - 1) * q->bsW + (long)(N - 1) * q->ldw + K;
  const long c_need = q->c_off + (long)(batch - 1) * q->bsC + (nsb - 1) * q->split_stride + (long)(M - 1) * q->ldc + width;
  if (a_need > q->a_elems || w_need > q->w_elems || c_need > q->c_elems)
    return fail(e, RK_ERR_INVALID, "debug gemm: the call reaches beyond A (%ld of %ld), W (%ld of %ld) or C (%ld of %ld)", a_need, (long)q->a_elems, w_need, (long)q->w_elems, c_need, (long)q->c_elems);
  if (epi == EPI_ARGMAX_F32 && !q->idx_out) return fail(e, RK_ERR_INVALID, "debug gemm: argmax needs idx_out");
  if (epi == EPI_LSE_F32 && (!q->labels || !q->xlab)) return fail(e, RK_ERR_INVALID, "debug gemm: LSE needs labels and xlab");
  if (producer && (!q->xraw_out || !q->ssq_out || (long)(M + 2 * q->band_rows) * p.nb > q->ssq_cap))
    return fail(e, RK_ERR_INVALID, "debug gemm: producer needs xraw_out and ssq_out of (M + 2 band_rows) x %d floats", p.nb);
  const size_t m_pad = ((size_t)M + 255) / 256 * 256 + 256;     // the ping-pong kernel reads the row factors of whole 256-row panels
  const bool factors = q->rowscale || q->ssq_in, lse = epi == EPI_LSE_F32;
  DebugScratch ds(e, "debug gemm");
  half_t* dA = ds.up<half_t>(q->A, (size_t)q->a_elems);
  half_t* dW = ds.up<half_t>(q->W, (size_t)q->w_elems);
  const Banded C = ds.banded(band_rows_span((size_t)q->c_elems, q->band_rows, q->ldc, celt), q->C);
  const Banded I = epi == EPI_ARGMAX_F32 ? ds.banded(band_rows_span((size_t)q->c_elems, q->band_rows, q->ldc, 4)) : Banded();
  const Banded X = producer ? ds.banded(band_rows_span((size_t)M * N, q->band_rows, N, 2)) : Banded();
  const Banded S = producer ? ds.banded(band_rows_span((size_t)M * p.nb, q->band_rows, p.nb, 4)) : Banded();
  float* dR = factors ? ds.alloc<float>(m_pad, 0) : nullptr;
  float* dQ = q->ssq_in ? ds.up<float>(q->ssq_in, (size_t)M * q->nb_in) : nullptr;
  int* dL = lse ? ds.up<int>(q->labels, (size_t)M) : nullptr;
  float* dXl = lse ? ds.up<float>(q->xlab, (size_t)M) : nullptr;
  if ((rc = ds.failed())) return rc;
  if (q->rowscale) DBG_HIP(ds, hipMemcpy(dR, q->rowscale, (size_t)M * 4, hipMemcpyHostToDevice));
  DBG_HIP(ds, hipDeviceSynchronize());
  c.A = dA; c.W = dW; c.C = C.interior() + (size_t)q->c_off * celt;
  c.fold = GemmFold();
  if (q->rowscale) c.fold.rowscale = dR;
  else if (q->ssq_in && q->factors_kernel) {
    launch_rowscale(st, dQ, dR, M, q->nb_in, K, e->d.eps, RK_XRAW_SCALE);
    c.fold.rowscale = dR;
  } else if (q->ssq_in) { c.fold.ssq_in = dQ; c.fold.nb_in = q->nb_in; }
  if (producer) { c.fold.xraw = X.interior<half_t>(); c.fold.ssq = S.interior<float>(); }
  c.lse(dL, dXl).argmax(I.all ? I.interior<int>() + q->c_off : nullptr);
  if (fp8) {                                             // (the quantiser's buffers are engine-owned: the owner gives them back)
    GemmW8 w8{nullptr, nullptr, 0, 0};
    if ((rc = quant_fp8(e, st, dW, N, K, q->ldw, &w8, nullptr, nullptr))) return rc;
    c.w8(w8);
  }
  int nb = 0;
  if ((rc = gemm(e, st, c, &nb))) return rc;
  DBG_HIP(ds, hipStreamSynchronize(st));
  DBG_HIP(ds, hipGetLastError());
  q->out_nb = nb;
  DBG_HIP(ds, C.read_back(q->C_out));
  if (I.all) DBG_HIP(ds, I.read_back(q->idx_out));
  if (producer) { DBG_HIP(ds, X.read_back(q->xraw_out)); DBG_HIP(ds, S.read_back(q->ssq_out)); }
  if (dXl) DBG_HIP(ds, hipMemcpy(q->xlab, dXl, (size_t)M * 4, hipMemcpyDeviceToHost));
  return RK_OK;
}
int rk_debug_gemm_ex(rk_engine* e, rk_debug_gemm_call* q) { return debug_gemm(e, q, false); }
int rk_debug_gemm_fp8(rk_engine* e, rk_debug_gemm_call* q) { return debug_gemm(e, q, true); }

// debug: the engine's FP8 quantiser on host data (include/rk_engine.h): quant_fp8, the read-backs, nothing of its own
int rk_debug_quant_fp8(rk_engine* e, const uint16_t* W, int N, int K, int ldw, uint8_t* q_out, int8_t* exp_out, uint16_t* deq_out) {
  if (!e || !W) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if (N <= 0 || K <= 0 || K % 16 || ldw < K || ldw % 8 || (long)N * ldw > (1L << 30)) return fail(e, RK_ERR_INVALID, "debug quant fp8: K %% 16, ldw >= K, ldw %% 8");
  hipStream_t st = e->slots[0].se;
  DebugScratch ds(e, "debug quant fp8");                  // (the quantiser's exponents are engine-owned: the owner gives them back)
  half_t* dW = ds.up<half_t>(W, (size_t)N * ldw);
  uint8_t* dQ = ds.alloc<uint8_t>((size_t)N * K);
  if ((rc = ds.failed())) return rc;
  GemmW8 w8{nullptr, nullptr, 0, 0};
  if ((rc = quant_fp8(e, st, dW, N, K, ldw, &w8, dQ, dW))) return rc;
  DBG_HIP(ds, hipStreamSynchronize(st));
  DBG_HIP(ds, hipGetLastError());
  const int groups = fp8_groups(K);
  if (q_out) DBG_HIP(ds, hipMemcpy(q_out, dQ, (size_t)N * K, hipMemcpyDeviceToHost));
  if (exp_out) DBG_HIP(ds, hipMemcpy2D(exp_out, groups, w8.exps, w8.lde, groups, N, hipMemcpyDeviceToHost));
  if (deq_out) DBG_HIP(ds, hipMemcpy2D(deq_out, (size_t)K * 2, dW, (size_t)ldw * 2, (size_t)K * 2, N, hipMemcpyDeviceToHost));
  return RK_OK;
}

// debug: n_launch back-to-back launches of one Gemm call with new data per launch, optionally beside a background call on the
// slot's decoder stream (include/rk_engine.h).  No launch code of its own: it builds the Gemms and calls gemm().
int rk_debug_gemm_chain(rk_engine* e, rk_debug_gemm_chain_call* q) {
  if (!e || !q) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  const int epi = q->epi, M = q->M, N = q->N, K = q->K, nl = q->n_launch;
  if (epi < 0 || epi > EPI_SWIGLU_F16 || q->family < 0 || q->family > 2 || M <= 0 || N <= 0 || K <= 0 || q->lda <= 0 || q->ldw <= 0 || q->ldc <= 0 ||
      M > (1 << 22))
    return fail(e, RK_ERR_INVALID, "debug gemm chain: bad shape");
  if (nl < 1 || nl > 64) return fail(e, RK_ERR_INVALID, "debug gemm chain: n_launch 1..64");
  if (q->accumulate && epi != EPI_RESID_F32) return fail(e, RK_ERR_INVALID, "debug gemm chain: accumulate is the fp32 residual epilogue's");
  const bool bg = q->bg_per_fg > 0;
  if (q->bg_per_fg < 0 || q->bg_per_fg > 16) return fail(e, RK_ERR_INVALID, "debug gemm chain: bg_per_fg 0..16");
  if (bg && (q->bg_M <= 0 || q->bg_N <= 0 || q->bg_K <= 0 || q->bg_M > (1 << 16) || q->bg_N > (1 << 16) || q->bg_K > (1 << 16) || q->bg_family < 0 ||
             q->bg_family > 2 || q->bg_variant < 0 || q->bg_variant > 6 ||
             !(q->bg_epi == EPI_STORE_F16 || q->bg_epi == EPI_RESID_F32 || q->bg_epi == EPI_RELU_F16 || q->bg_epi == EPI_STORE_F32)))
    return fail(e, RK_ERR_INVALID, "debug gemm chain: bad background call");
  const bool gated = EPI_IS_GATED(epi), f16 = epi == EPI_STORE_F16 || epi == EPI_RELU_F16 || gated;
  const size_t celt = f16 ? 2 : 4;
  // the plans first (pointers only count as aligned / present): a call outside the contract stops here, before any allocation
  half_t* const dummy = plan_dummy;
  hipStream_t st = e->slots[0].se, sb = e->slots[0].sd;
  Gemm c(PC_OTHER, epi, dummy, q->lda, dummy, q->ldw, dummy, q->ldc, M, N, K);
  c.on(family_of(q->family));
  if (q->rowscale) c.fold.rowscale = (const float*)dummy;
  const GemmPlan p = plan_gemm(e, c, st);
  plan_out_ints(p, &q->out_family, &q->out_variant, &q->out_m_pp2, &q->out_ksplit);
  q->out_n_cu = e->n_cu;
  q->bg_out_family = GEMM_NONE; q->bg_out_variant = q->bg_out_m_pp2 = 0; q->bg_out_ksplit = 1;
  if (p.family == GEMM_NONE)
    return fail(e, RK_ERR_STATE, "no kernel of family %d takes the GEMM M=%d N=%d K=%d (epilogue %d, batch 1): %s", q->family, M, N, K, epi, p.why ? p.why : "");
  // the background's plan and launches see bg_variant as the engine's gemm_variant option (the foreground keeps the engine's own)
  const int fg_variant = e->opt.gemm_variant;
  Gemm b(PC_OTHER, bg ? q->bg_epi : EPI_STORE_F16, dummy, q->bg_K, dummy, q->bg_K, dummy, q->bg_N, q->bg_M, q->bg_N, q->bg_K);
  if (bg) {
    b.on(family_of(q->bg_family));
    e->opt.gemm_variant = q->bg_variant;
    const GemmPlan pb = plan_gemm(e, b, sb);
    e->opt.gemm_variant = fg_variant;
    plan_out_ints(pb, &q->bg_out_family, &q->bg_out_variant, &q->bg_out_m_pp2, &q->bg_out_ksplit);
    if (pb.family == GEMM_NONE)
      return fail(e, RK_ERR_STATE, "no kernel of family %d takes the background GEMM M=%d N=%d K=%d (epilogue %d): %s", q->bg_family, q->bg_M, q->bg_N, q->bg_K, q->bg_epi, pb.why ? pb.why : "");
    if (pb.pp2()) return fail(e, RK_ERR_INVALID, "debug gemm chain: the background's plan puts rows on the ping-pong kernel");
  }
  if (q->plan_only) return RK_OK;
  // extents, from the addressing of the call, against what the caller gave
  if (!q->A || !q->W || !q->C || !q->C_out || q->band_rows < 256) return fail(e, RK_ERR_INVALID, "debug gemm chain: A, W, C, C_out and band_rows >= 256");
  const long width = gated ? N / 2 : N;
  const long a_need = (long)(M - 1) * q->lda + K, w_need = (long)(N - 1) * q->ldw + K, c_need = (long)(M - 1) * q->ldc + width;
  if (a_need > q->a_elems || w_need > q->w_elems || c_need > q->c_elems)
    return fail(e, RK_ERR_INVALID, "debug gemm chain: the call reaches beyond A (%ld of %ld), W (%ld of %ld) or C (%ld of %ld)", a_need, (long)q->a_elems, w_need, (long)q->w_elems, c_need, (long)q->c_elems);
  const int n_out = q->accumulate ? 1 : nl;
  const size_t m_pad = ((size_t)M + 255) / 256 * 256 + 256;     // the ping-pong kernel reads the row factors of whole 256-row panels
  const size_t bga = (size_t)q->bg_M * q->bg_K, bgw = (size_t)q->bg_N * q->bg_K, bgc = (size_t)q->bg_M * q->bg_N;
  DebugScratch ds(e, "debug gemm chain");
  half_t* dA = ds.up<half_t>(q->A, (size_t)nl * q->a_elems);
  c.W = ds.up<half_t>(q->W, (size_t)q->w_elems);
  std::vector<Banded> C(n_out);                            // every output an allocation [band | interior | band] of its own
  for (int i = 0; i < n_out; ++i)
    C[i] = ds.banded(band_rows_span((size_t)q->c_elems, q->band_rows, q->ldc, celt), (const char*)q->C + (size_t)i * q->c_elems * celt);
  float* dR = q->rowscale ? ds.alloc<float>((size_t)nl * m_pad, 0) : nullptr;
  if (bg) {
    const std::vector<half_t> h = lcg_halfs(std::max(bga, bgw), 2463534242u);
    b.A = ds.up<half_t>(h.data(), bga); b.W = ds.up<half_t>(h.data(), bgw); b.C = ds.alloc<float>(bgc, 0);
  }
  if ((rc = ds.failed())) return rc;
  for (int i = 0; q->rowscale && i < nl; ++i)
    DBG_HIP(ds, hipMemcpy(dR + (size_t)i * m_pad, q->rowscale + (size_t)i * M, (size_t)M * 4, hipMemcpyHostToDevice));
  DBG_HIP(ds, hipDeviceSynchronize());
  auto background = [&]() {
    e->opt.gemm_variant = q->bg_variant;
    int r = RK_OK;
    for (int j = 0; r == RK_OK && j < q->bg_per_fg; ++j) r = gemm(e, sb, b);
    e->opt.gemm_variant = fg_variant;
    return r;
  };
  for (int i = 0; rc == RK_OK && i < nl; ++i) {
    c.A = dA + (size_t)i * q->a_elems;
    c.C = C[q->accumulate ? 0 : i].interior();
    c.fold = GemmFold();
    if (q->rowscale) c.fold.rowscale = dR + (size_t)i * m_pad;
    if (bg && q->bg_first) rc = background();
    if (rc == RK_OK) rc = gemm(e, st, c);
    if (rc == RK_OK && bg && !q->bg_first) rc = background();
  }
  if (rc) return rc;                                       // (whatever was enqueued is waited for by the owner)
  DBG_HIP(ds, hipStreamSynchronize(st)); DBG_HIP(ds, hipStreamSynchronize(sb));
  DBG_HIP(ds, hipGetLastError());
  for (int i = 0; i < n_out; ++i) DBG_HIP(ds, C[i].read_back((char*)q->C_out + (size_t)i * C[i].total()));
  return RK_OK;
}

// debug: one attention call on host data, every output between sentinel bands (include/rk_engine.h).  No kernel and no dispatch of
// its own: it uploads the operands, asks the plan_*attn function of the kind and hands the plan to that plan's launcher.
int rk_debug_attn(rk_engine* e, rk_debug_attn_call* q) {
  if (!e || !q) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if (!e->finalized) return fail(e, RK_ERR_STATE, "debug attn: engine not finalized");
  const int kind = q->kind, B = q->n_seq, H = q->H;
  if (kind < 1 || kind > 6) return fail(e, RK_ERR_INVALID, "debug attn: kind 1..6");
  const bool llama_kind = kind == 4 || kind == 5;
  if (e->family != (llama_kind ? 1 : 0)) return fail(e, RK_ERR_STATE, "debug attn: kind %d needs a %s engine", kind, llama_kind ? "Llama" : "T5");
  if (B <= 0 || B > (1 << 16) || H <= 0 || H > 1024) return fail(e, RK_ERR_INVALID, "debug attn: n_seq and H");
  const bool planning = q->plan_only != 0;
  const int hd = head_width(e), band = q->band_rows;   // (kinds 4 and 5: the Llama engine's head_dim, 64 or 128)
  if ((kind == 2 || kind == 6) && hd != 64) return refuse_wide(e, "debug attn", "kinds 2 and 6 (the decoder kernels) have no 128-wide form");
  if (!planning && (!q->q || !q->out || !q->out_all || band < 1)) return fail(e, RK_ERR_INVALID, "debug attn: q, out, out_all and band_rows >= 1");
  // ---- the offsets: lengths, the longest and the shortest ----
  int maxL = 0, minL = 1 << 30, T = 0;
  const bool has_off = kind == 1 || kind == 3 || kind == 4 || (kind == 2 && q->cross);
  if (has_off) {
    if (!q->seq_off || q->seq_off[0] != 0) return fail(e, RK_ERR_INVALID, "debug attn: seq_off[n_seq + 1] starting at 0");
    for (int b = 0; b < B; ++b) {
      const int L = q->seq_off[b + 1] - q->seq_off[b];
      if (L <= 0 || L > (1 << 20)) return fail(e, RK_ERR_INVALID, "debug attn: sequence %d has %d keys", b, L);
      maxL = std::max(maxL, L); minL = std::min(minL, L);
    }
    T = q->seq_off[B];
  }
  long q_rows_need = 0, kv_rows_need = 0, out_rows_need = 0;   // interior rows the call addresses
  long ldq_min = 0, ldkv_min = 0, ldctx_min = 0;
  auto plan_out = [&](int k, int tp, dim3 g1, dim3 g2, int lds) {
    q->out_kind = k; q->out_tparam = tp; q->out_lds = lds; q->out_n_cu = e->n_cu;
    q->out_grid[0] = (int)g1.x; q->out_grid[1] = (int)g1.y; q->out_grid[2] = (int)g1.z;
    q->out_grid2[0] = (int)g2.x; q->out_grid2[1] = (int)g2.y; q->out_grid2[2] = (int)g2.z;
  };
  q->out_staged = q->out_mfma = q->out_part = q->out_R = q->out_nch = q->out_skip_long = q->out_heads_per_wg = 0;
  EncAttnPlan ep; DecAttnPlan dp; XAttnPlan xp; CausalAttnPlan cp; LlamaDecAttnPlan lp;
  int dec_rows = 0, dec_keys = 0;
  if (kind == 1) {
    const int I = H * hd;
    ldq_min = 3L * I; ldctx_min = I; q_rows_need = out_rows_need = T;
    if (!planning && !q->bias_lut) return fail(e, RK_ERR_INVALID, "debug attn: the encoder needs bias_lut");
    ep = plan_enc_attn(e, B, maxL, minL, H);
    plan_out((int)ep.kind, ep.kind == EncAttnPlan::DMA ? ep.ng : ep.nw, ep.grid, ep.tiled_grid, ep.lds);
    q->out_skip_long = ep.skip_long; q->out_heads_per_wg = ep.heads_per_wg;
  } else if (kind == 2) {
    const int Ld = q->Ld;
    if (Ld <= 0 || Ld > (1 << 16) || q->k_col < 0 || q->v_col < 0) return fail(e, RK_ERR_INVALID, "debug attn: Ld, k_col, v_col");
    const bool tree = q->tree_rows > 0;
    if (tree && (q->cross || q->row_off || !q->tree_keys || !q->tree_pos)) return fail(e, RK_ERR_INVALID, "debug attn: the tree form is the self-attention's, with tree_keys and tree_pos, without row_off");
    if (q->row_off) {
      if (q->row_off[0] != 0) return fail(e, RK_ERR_INVALID, "debug attn: row_off starts at 0");
      int longest = 0;
      for (int b = 0; b < B; ++b) {
        const int n = q->row_off[b + 1] - q->row_off[b];
        if (n <= 0) return fail(e, RK_ERR_INVALID, "debug attn: sequence %d has %d rows", b, n);
        longest = std::max(longest, n);
      }
      if (longest != Ld) return fail(e, RK_ERR_INVALID, "debug attn: Ld = %d is not the longest row count %d", Ld, longest);
      dec_rows = q->row_off[B];
    } else dec_rows = tree ? q->tree_rows : B * Ld;
    dec_keys = q->cross ? maxL : Ld;
    ldq_min = H * 64; ldctx_min = H * 64; out_rows_need = dec_rows;
    q_rows_need = tree ? 0 : dec_rows;                       // (tree: the rows tree_keys names, checked below)
    if (q->cross) { ldkv_min = std::max(q->k_col, q->v_col) + H * 64; kv_rows_need = T; }
    else ldq_min = std::max<long>(ldq_min, std::max(q->k_col, q->v_col) + H * 64);
    if (tree) {
      q_rows_need = q->tree_rows;
      for (int r = 0; r < q->tree_rows; ++r) {
        if (q->tree_pos[r] < 0 || q->tree_pos[r] >= Ld) return fail(e, RK_ERR_INVALID, "debug attn: tree_pos[%d] outside 0..Ld-1", r);
        for (int j = 0; j <= q->tree_pos[r]; ++j) {
          const int k = q->tree_keys[(size_t)r * Ld + j];
          if (k < 0) return fail(e, RK_ERR_INVALID, "debug attn: tree_keys[%d][%d] negative", r, j);
          q_rows_need = std::max<long>(q_rows_need, k + 1L);
        }
      }
    }
    dp = plan_dec_attn(e, q->cross != 0, B, Ld, dec_keys, H, tree ? q->tree_rows : 0);
    plan_out((int)dp.staged, 0, dp.mfma_grid, dp.grid, (int)dp.lds);
    q->out_staged = (int)dp.staged; q->out_mfma = dp.mfma;
    // the staged kernels' dynamic LDS is opted in at finalize for the engine's capacities (the MFMA kernel's is fixed)
    const size_t lds_cap = dp.staged == DecAttnPlan::SEQ ? 160 * 1024 : std::min<size_t>(attn_dec_lds(std::max(e->d.max_tokens, e->d.max_dec_len)), 160 * 1024);
    if (dp.staged != DecAttnPlan::NONE && dp.lds > lds_cap)
      return fail(e, RK_ERR_STATE, "debug attn: %d keys need %zu bytes of LDS, the staged kernel of this engine has %zu", dec_keys, dp.lds, lds_cap);
    if (dp.mfma && Ld > ATTX_MAXQ) return fail(e, RK_ERR_STATE, "debug attn: the matrix-core kernel takes at most %d positions", ATTX_MAXQ);
  } else if (kind == 3) {
    const int M = q->M, d = q->d, Ld = q->Ld;
    if (M <= 0 || M > (1 << 16) || d <= 0 || d % 32 || d > 16384 || Ld <= 0 || q->row0 < 0) return fail(e, RK_ERR_INVALID, "debug attn: M, Ld, row0 and d (a multiple of 32)");
    if (q->ldq != H * d || q->ldkv != d || q->ldctx != H * d) return fail(e, RK_ERR_INVALID, "debug attn: the query-side form is dense: ldq = ldctx = H d, ldkv = d");
    if (maxL > 65536) return fail(e, RK_ERR_STATE, "debug attn: the chunk merge takes sequences of at most 65536 keys");
    for (int m = 0; m < M; ++m) {
      if (q->row_seq && q->row0 + m >= q->n_row_seq) return fail(e, RK_ERR_INVALID, "debug attn: row_seq has %d entries, row %d is read", q->n_row_seq, q->row0 + m);
      const int b = q->row_seq ? q->row_seq[q->row0 + m] : (q->row0 + m) / Ld;
      if (b < 0 || b >= B) return fail(e, RK_ERR_INVALID, "debug attn: row %d belongs to sequence %d of %d", q->row0 + m, b, B);
    }
    ldq_min = (long)H * d; ldkv_min = d; ldctx_min = (long)H * d; q_rows_need = out_rows_need = M; kv_rows_need = T;
    xp = plan_xattn(e, false, M, maxL, H, d);
    plan_out((int)xp.part, xp.part == XAttnPlan::VALU4 ? 4 : 16, xp.part_grid, dim3(H, M), 0);
    q->out_part = (int)xp.part; q->out_nch = xp.nch; q->out_mfma = xp.part == XAttnPlan::MFMA_FEW || xp.part == XAttnPlan::MFMA;
  } else if (kind == 4) {
    const int n_kv = q->n_kv;
    if (n_kv <= 0 || H % n_kv) return fail(e, RK_ERR_INVALID, "debug attn: n_kv must divide H");
    ldq_min = (long)(H + 2 * n_kv) * hd; ldctx_min = (long)H * hd; q_rows_need = out_rows_need = T;
    cp = plan_llama_attn(e, B, maxL, H, n_kv);
    plan_out((cp.hd == 64 ? 2 : (int)(cp.kind == CAUSAL_DMA)) + (cp.window > 0 ? 4 : 0), cp.nw, cp.grid, dim3(0, 0, 0), cp.lds);
    if (!causal_attn_exists(cp)) return refuse_window(e, "debug attn", maxL);
  } else if (kind == 6) {
    const int P = q->P;
    if (P <= 0 || P > 8192) return fail(e, RK_ERR_INVALID, "debug attn: the T5 cached step takes a cache of 1..8192 positions");
    ldq_min = 3L * H * 64; ldctx_min = (long)H * 64; q_rows_need = out_rows_need = B;
    if (!planning) {
      if (!q->pos || !q->bias_lut || !q->cache || !q->cache_all) return fail(e, RK_ERR_INVALID, "debug attn: the T5 cached step needs pos, bias_lut, cache and cache_all");
      if (q->pos[0] < 0 || q->pos[0] >= P) return fail(e, RK_ERR_INVALID, "debug attn: pos = %d outside the cache of %d positions", q->pos[0], P);
    }
    const bool one = e->opt.dec_cached_attn != 0;
    plan_out(one ? 1 : 0, 0, one ? dim3(H, B) : dim3(B), one ? dim3(0, 0, 0) : dim3(1, H, B), (int)attn_dec_lds(P));
  } else {
    const int n_kv = q->n_kv, P = q->P;
    if (n_kv <= 0 || H % n_kv || P <= 0 || P > (1 << 20)) return fail(e, RK_ERR_INVALID, "debug attn: n_kv must divide H, P > 0");
    if (q->ldctx != H * hd) return fail(e, RK_ERR_INVALID, "debug attn: the step's ctx is dense: ldctx = %d H", hd);
    ldq_min = (long)(H + 2 * n_kv) * hd; ldctx_min = (long)H * hd; q_rows_need = out_rows_need = B;
    if (!planning) {
      if (!q->pos || !q->cos_t || !q->sin_t || !q->cache || !q->cache_all) return fail(e, RK_ERR_INVALID, "debug attn: the step needs pos, cos_t, sin_t, cache and cache_all");
      for (int b = 0; b < B; ++b)
        if (q->pos[b] < 0 || q->pos[b] >= P || q->pos[b] >= q->max_pos) return fail(e, RK_ERR_INVALID, "debug attn: pos[%d] = %d outside the cache of %d / the tables of %d", b, q->pos[b], P, q->max_pos);
    }
    if (q->g1 < 0 || q->g1 > 8 || (q->g1 > 1 && B % q->g1)) return fail(e, RK_ERR_INVALID, "debug attn: the drafting step takes g1 in 2..8 rows per cache row and n_seq a multiple of it (g1 = %d, n_seq = %d)", q->g1, B);
    if (q->g1 > 1 && !planning && !q->live) return fail(e, RK_ERR_INVALID, "debug attn: the drafting step needs live[n_seq]");
    if (q->qk_norm && (hd != 128 || e->window > 0 || q->qkv_bias || !(q->qk_eps > 0.f)))
      return fail(e, RK_ERR_STATE, "debug attn: the step with the q / k head norm takes head_dim 128, no window, no qkv_bias and qk_eps > 0");
    lp = plan_llama_dec_attn(e, B, P, H, n_kv);
    lp.kv8 = 0;                                               // this entry's cache is fp16 on every engine (an FP8-cache engine's: rk_debug_kv8_step)
    plan_out(lp.window > 0 ? 1 : (q->qk_norm ? 2 : 0), lp.R, lp.grid, lp.cgrid, 0);
    q->out_R = lp.R; q->out_nch = lp.nch;
    if (H % lp.R) return fail(e, RK_ERR_STATE, "debug attn: R = %d does not divide %d heads", lp.R, H);
  }
  if (planning) return RK_OK;
  // ---- extents, from the addressing of the call, against what the caller gave ----
  if (q->ldq < ldq_min || q->ldq % 8 || q->ldctx < ldctx_min || q->ldctx % 8 || (ldkv_min && (q->ldkv < ldkv_min || q->ldkv % 8)) || q->k_col % 8 || q->v_col % 8)
    return fail(e, RK_ERR_INVALID, "debug attn: leading dimensions (ldq %d >= %ld, ldkv %d >= %ld, ldctx %d >= %ld; multiples of 8, as k_col and v_col)", q->ldq, ldq_min, q->ldkv, ldkv_min, q->ldctx, ldctx_min);
  if (q_rows_need > q->q_rows || out_rows_need > q->out_rows || (kv_rows_need && (!q->kv || kv_rows_need > q->kv_rows)))
    return fail(e, RK_ERR_INVALID, "debug attn: the call reaches beyond q (%ld of %ld rows), kv (%ld of %ld) or out (%ld of %ld)", q_rows_need, (long)q->q_rows, kv_rows_need, (long)q->kv_rows, out_rows_need, (long)q->out_rows);
  if (((long)q->q_rows + 2L * band) * q->ldq >= (1L << 31) || ((long)q->kv_rows + 2L * band) * std::max(q->ldkv, 1) >= (1L << 31))
    return fail(e, RK_ERR_INVALID, "debug attn: operands of 2^31 elements or more");   // (the DMA kernels address rows by 32-bit byte offsets)
  DebugScratch ds(e, "debug attn");
  const size_t q_all = ((size_t)q->q_rows + 2 * (size_t)band) * q->ldq, kv_all = q->kv ? ((size_t)q->kv_rows + 2 * (size_t)band) * q->ldkv : 0;
  half_t* dQ = ds.up<half_t>(q->q, q_all);               // (q and kv come with the caller's bands)
  half_t* dKV = q->kv ? ds.up<half_t>(q->kv, kv_all) : nullptr;
  const Banded O = ds.banded(band_rows_span((size_t)q->out_rows * q->ldctx, band, q->ldctx, 2), q->out);
  Banded Cache;
  half_t* const qi = dQ ? dQ + (size_t)band * q->ldq : nullptr;
  half_t* const kvi = dKV ? dKV + (size_t)band * q->ldkv : nullptr;
  half_t* const oi = O.interior<half_t>();
  int* dOff = has_off ? ds.up<int>(q->seq_off, (size_t)B + 1) : nullptr;
  const bool takes_lut = kind <= 2 || kind == 6;
  float* dLut = q->bias_lut && takes_lut ? ds.up<float>(q->bias_lut, (size_t)H * RK_LUT_N) : nullptr;
  hipStream_t st = e->slots[0].se;
  if (kind == 1) {
    if ((rc = ds.ready())) return rc;
    launch_enc_attn(e, st, EncAttnCall{qi, oi, dOff, dLut, q->ldq, q->ldctx, H * hd, H, B, maxL, T}, ep);
  } else if (kind == 2) {
    int* dRow = q->row_off ? ds.up<int>(q->row_off, (size_t)B + 1) : nullptr;
    int* dTk = q->tree_rows > 0 ? ds.up<int>(q->tree_keys, (size_t)q->tree_rows * q->Ld) : nullptr;
    int* dTp = q->tree_rows > 0 ? ds.up<int>(q->tree_pos, (size_t)q->tree_rows) : nullptr;
    if ((rc = ds.ready())) return rc;
    const half_t* kb = q->cross ? kvi : qi;
    launch_dec_attn(e, st, dp, AttnDecArgs{qi, q->ldq, kb + q->k_col, kb + q->v_col, q->cross ? q->ldkv : q->ldq, q->cross ? dOff : nullptr, oi, q->ldctx, dLut,
                                           q->Ld, q->cross ? 0 : 1, dec_keys, dTk, dTp, 0, dRow}, 0, 0);
  } else if (kind == 3) {
    int* dRs = q->row_seq ? ds.up<int>(q->row_seq, (size_t)q->n_row_seq) : nullptr;
    float* dPart = ds.alloc<float>((size_t)q->M * xp.nch * H * q->d, RK_DEBUG_SENTINEL);
    float* dStat = ds.alloc<float>((size_t)q->M * xp.nch * H * 2, RK_DEBUG_SENTINEL);
    if ((rc = ds.ready())) return rc;
    launch_xattn_part(e, st, xp, XAttnArgs{qi, kvi, dOff, dPart, dStat, oi, q->Ld, H, q->d, xp.nch, q->row0, dRs}, maxL, T);
  } else if (kind == 4) {
    if ((rc = ds.ready())) return rc;
    launch_llama_attn(e, st, CausalAttnCall{qi, oi, dOff, q->ldq, q->ldctx, H, q->n_kv, B, maxL, T}, cp);
  } else if (kind == 6) {
    const int I = H * 64, P = q->P;
    Cache = ds.banded(band_rows_span((size_t)B * P * 2 * I, band, 64, 2), q->cache);
    std::vector<int> keys((size_t)B * P);
    for (int b = 0; b < B; ++b) for (int j = 0; j < P; ++j) keys[(size_t)b * P + j] = b * P + j;   // (as rk_t5_generate lays them out)
    int* dPos = ds.up<int>(q->pos, 1);
    int* dTk = ds.up<int>(keys.data(), keys.size());
    int* dTp = ds.alloc<int>((size_t)B, 0);
    if ((rc = ds.ready())) return rc;
    launch_dec_cached_step(e, st, AttnCachedArgs{qi, q->ldq, Cache.interior<half_t>(), P, I, dPos, oi, q->ldctx, dLut}, B, H, dTk, dTp);
  } else {
    const int g1 = q->g1 > 1 ? q->g1 : 1;                     // the drafting step: g1 step rows per cache row
    const KvLayerLayout kl = kv_layer_layout(0, B / g1, q->n_kv, hd, q->P);   // the caller's cache: one layer of the fp16 layout
    Cache = ds.banded(band_rows_span(kl.bytes / 2, band, hd, 2), q->cache);
    int* dPos = ds.up<int>(q->pos, (size_t)B);
    float* dCos = ds.up<float>(q->cos_t, (size_t)q->max_pos * (hd / 2));
    float* dSin = ds.up<float>(q->sin_t, (size_t)q->max_pos * (hd / 2));
    float* dBias = q->qkv_bias ? ds.up<float>(q->qkv_bias, (size_t)(H + 2 * q->n_kv) * hd) : nullptr;
    float* dQkn = q->qk_norm ? ds.up<float>(q->qk_norm, (size_t)2 * hd) : nullptr;
    float* dPart = ds.alloc<float>((size_t)B * H * lp.nch * ldc_pstr(hd), RK_DEBUG_SENTINEL);
    int* dLive = g1 > 1 ? ds.up<int>(q->live, (size_t)B) : nullptr;
    if ((rc = ds.ready())) return rc;
    const float scale_log2e = (1.0f / std::sqrt((float)hd)) * 1.4426950408889634f;
    const LlamaDecAttnArgs aa{qi, nullptr, nullptr /* kc, vc: the cache's, in the launch */, dPos, dCos, dSin, dPart, oi, q->ldq, H, q->n_kv, q->P, lp.nch, scale_log2e, dBias, 0, dQkn, q->qk_eps};
    launch_llama_dec_attn(e, st, lp, aa, B, g1, dLive, kv_cache_layer(kl, Cache.interior<half_t>(), 0));   // (llama_step_rows' call)
  }
  DBG_HIP(ds, hipStreamSynchronize(st));
  DBG_HIP(ds, hipGetLastError());
  DBG_HIP(ds, O.read_back(q->out_all));
  if (Cache.all) DBG_HIP(ds, Cache.read_back(q->cache_all));
  return RK_OK;
}

// debug: the whole query-side cross-attention chain of one decoder layer on host operands (include/rk_engine.h).  No kernel and no
// dispatch of its own: it uploads the operands, regroups W_k as finalize does, fills an XAttnChain and calls run_xattn_chain - the
// function run_decoder calls.  The workspaces of a block are refilled with the sentinel in front of every block and copied out
// behind it.
int rk_debug_xattn_chain(rk_engine* e, rk_debug_xattn_chain_call* q) {
  if (!e || !q) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if (!e->finalized) return fail(e, RK_ERR_STATE, "debug xattn chain: engine not finalized");
  if (e->family != 0) return fail(e, RK_ERR_STATE, "debug xattn chain: needs a T5 engine");
  const int hd = head_width(e);
  const int M = q->M, H = q->H, d = q->d, Ld = q->Ld, B = q->n_seq, band = q->band_rows, I = H * hd;
  if (B <= 0 || B > (1 << 16) || H <= 0 || H > 1024) return fail(e, RK_ERR_INVALID, "debug xattn chain: n_seq and H");
  if (M <= 0 || M > (1 << 16) || d <= 0 || d % 32 || d > 16384 || Ld <= 0 || q->row0 < 0)
    return fail(e, RK_ERR_INVALID, "debug xattn chain: M, Ld, row0 and d (a multiple of 32)");
  if (!q->seq_off || q->seq_off[0] != 0) return fail(e, RK_ERR_INVALID, "debug xattn chain: seq_off[n_seq + 1] starting at 0");
  int maxL = 0;
  for (int b = 0; b < B; ++b) {
    const int L = q->seq_off[b + 1] - q->seq_off[b];
    if (L <= 0 || L > (1 << 20)) return fail(e, RK_ERR_INVALID, "debug xattn chain: sequence %d has %d keys", b, L);
    maxL = std::max(maxL, L);
  }
  const int T = q->seq_off[B];
  if (maxL > 65536) return fail(e, RK_ERR_STATE, "debug xattn chain: the chunk merge takes sequences of at most 65536 keys");
  for (int m = 0; m < M; ++m) {
    if (q->row_seq && q->row0 + m >= q->n_row_seq) return fail(e, RK_ERR_INVALID, "debug xattn chain: row_seq has %d entries, row %d is read", q->n_row_seq, q->row0 + m);
    const int b = q->row_seq ? q->row_seq[q->row0 + m] : (q->row0 + m) / Ld;
    if (b < 0 || b >= B) return fail(e, RK_ERR_INVALID, "debug xattn chain: row %d belongs to sequence %d of %d", q->row0 + m, b, B);
  }
  if (q->rowscale && q->ssq_in) return fail(e, RK_ERR_INVALID, "debug xattn chain: rowscale or ssq_in, not both");
  if (q->ssq_in && (q->nb_in <= 0 || q->nb_in > 4096)) return fail(e, RK_ERR_INVALID, "debug xattn chain: ssq_in needs nb_in in 1..4096");
  // ---- the plan: of the first and of the last block of the row loop ----
  XAttnChain c{};
  c.ldx = q->ldx; c.Ld = Ld; c.row0 = q->row0; c.ldo = q->ldo; c.M = M; c.H = H; c.dm = d; c.maxL = maxL; c.T = T; c.fuse_asked = q->fuse_asked != 0; c.hd = hd;
  c.family = dec_len_class(e, Ld).stream ? GEMM_STREAM : GEMM_TILED;
  const bool fuse = xattn_chain_fused(c);
  const int blk = xattn_block_rows(maxL), n_blocks = (M + blk - 1) / blk, wrows = std::min(blk, M), nch = (maxL + 63) / 64;
  q->out_fused = fuse; q->out_block_rows = blk; q->out_n_blocks = n_blocks; q->out_nch = nch; q->out_n_cu = e->n_cu;
  q->out_eps = e->d.eps; q->out_xs = RK_XRAW_SCALE;
  for (int i = 0; i < 2; ++i) {
    const int r0 = i ? (n_blocks - 1) * blk : 0;
    const XAttnPlan xp = plan_xattn(e, fuse, std::min(blk, M - r0), maxL, H, d);
    q->out_qk_R[i] = xp.fuse_qk ? xp.qk_R : 0; q->out_qk_CS[i] = xp.fuse_qk ? xp.qk_CS : 0; q->out_part_kind[i] = (int)xp.part;
    q->out_part_grid[i][0] = (int)xp.part_grid.x; q->out_part_grid[i][1] = (int)xp.part_grid.y; q->out_part_grid[i][2] = (int)xp.part_grid.z;
    q->out_fuse_cv[i] = xp.fuse_cv; q->out_cv_R[i] = xp.fuse_cv ? xp.cv_R : 0;
  }
  if (q->plan_only) return RK_OK;
  // ---- extents, from the addressing of the chain, against what the caller gave ----
  if (!q->x || !q->wq || !q->wk || !q->wv || !q->enc || !q->qk_all || !q->part_all || !q->stat_all || !q->xctx_all || !q->ctx_all || band < 1)
    return fail(e, RK_ERR_INVALID, "debug xattn chain: x, wq, wk, wv, enc, the five outputs and band_rows >= 1");
  if (q->ldx < d || q->ldx % 8 || q->ldx > (1 << 20) || q->ldo < I || q->ldo % 8 || q->ldo > (1 << 20))
    return fail(e, RK_ERR_INVALID, "debug xattn chain: leading dimensions (ldx %d >= %d, ldo %d >= %d; multiples of 8, at most 2^20)", q->ldx, d, q->ldo, I);
  if (q->enc_rows < T) return fail(e, RK_ERR_INVALID, "debug xattn chain: the call reaches beyond enc (%d of %ld rows)", T, (long)q->enc_rows);
  const size_t Hd = (size_t)H * d, part_in = (size_t)wrows * nch * Hd, stat_in = (size_t)wrows * nch * H * 2;
  const BandSpan part_s = band_rows_span(part_in, band, Hd, 4), stat_s = band_rows_span(stat_in, band, (size_t)H * 2, 4);
  const BandSpan xc_s = band_rows_span((size_t)wrows * Hd, band, Hd, 2), qk_s = band_rows_span((size_t)M * Hd, band, Hd, 2);
  const BandSpan ctx_s = band_rows_span((size_t)M * q->ldo, band, q->ldo, 2);
  const size_t enc_all = ((size_t)q->enc_rows + 2 * band) * d;
  if (enc_all >= (1ul << 31) || qk_s.all() / 2 >= (1ul << 31) || part_s.all() / 4 >= (1ul << 31) || stat_s.all() / 4 >= (1ul << 31) ||
      ctx_s.all() / 2 >= (1ul << 31) || (size_t)M * q->ldx >= (1ul << 31))
    return fail(e, RK_ERR_INVALID, "debug xattn chain: operands of 2^31 elements or more");
  DebugScratch ds(e, "debug xattn chain");
  const std::vector<half_t> ckT = regroup_ckT((const half_t*)q->wk, H, d, hd);
  c.x = ds.up<half_t>(q->x, (size_t)M * q->ldx);
  c.wq = ds.up<half_t>(q->wq, (size_t)I * d);
  c.wkT = ds.up<half_t>(ckT.data(), (size_t)I * d);
  c.wv = ds.up<half_t>(q->wv, (size_t)I * d);
  half_t* dEnc = ds.up<half_t>(q->enc, enc_all);          // (enc comes with the caller's bands)
  c.seq_off = ds.up<int>(q->seq_off, (size_t)B + 1);
  c.row_seq = q->row_seq ? ds.up<int>(q->row_seq, (size_t)q->n_row_seq) : nullptr;
  c.fold.rowscale = q->rowscale ? ds.up<float>(q->rowscale, (size_t)M) : nullptr;
  c.fold.ssq_in = q->ssq_in ? ds.up<float>(q->ssq_in, (size_t)M * q->nb_in) : nullptr;
  c.fold.nb_in = q->ssq_in ? q->nb_in : 0;
  c.q = ds.alloc<half_t>((size_t)M * I, RK_DEBUG_SENTINEL);
  const Banded Qk = ds.banded(qk_s), Part = ds.banded(part_s), Stat = ds.banded(stat_s), Xc = ds.banded(xc_s), Ctx = ds.banded(ctx_s, q->ctx);
  if ((rc = ds.failed())) return rc;
  c.enc = dEnc + (size_t)band * d;
  c.qk = Qk.interior<half_t>(); c.part = Part.interior<float>(); c.stat = Stat.interior<float>(); c.xctx = Xc.interior<half_t>();
  c.ctx = Ctx.interior<half_t>();
  hipStream_t st = e->slots[0].se;
  // the GEMMs of the unfused form against the contract of their kernel family, before anything is launched
  if (!fuse || nch > DECV_MAXCH) {
    std::vector<Gemm> gs;
    if (!fuse) { gs.push_back(xattn_q_gemm(c)); gs.push_back(xattn_qk_gemm(c, 0, wrows, c.qk)); }
    gs.push_back(xattn_cv_gemm(c, 0, wrows));
    for (const Gemm& g : gs) {
      const GemmPlan gp = plan_gemm(e, g, st);
      // (run_decoder hands a GEMM on the persistent ping-pong kernel ready-made row factors - NormStream::consumer; this call does not)
      if (q->ssq_in && &g == &gs[0] && !fuse && gp.pp2())
        return fail(e, RK_ERR_STATE, "debug xattn chain: the q GEMM of this shape takes ready-made row factors: pass rowscale, not ssq_in");
      if (gp.family == GEMM_NONE) return fail(e, RK_ERR_STATE, "debug xattn chain: no kernel takes the GEMM M=%d N=%d K=%d of the unfused form: %s", g.M, g.N, g.K, gp.why ? gp.why : "");
    }
  }
  // the qk workspace holds ONE block in the engine; here every block has rows of its own in qk_all (the front hook hands them out), the part / stat / xctx workspaces are refilled in front of a block and copied out behind it
  struct HookState { rk_engine* e; rk_debug_xattn_chain_call* q; hipStream_t st; half_t* qk0; const Banded *part, *stat, *xc; size_t Hd, part_in, stat_in; int blk; }
      hc{e, q, st, c.qk, &Part, &Stat, &Xc, Hd, part_in, stat_in, blk};
  XAttnChainHook hook{[](void* user, bool front, int r0, const XAttnPlan&, half_t** qk) -> int {
    HookState& h = *(HookState*)user;
    const size_t k = (size_t)(r0 / h.blk);
    bool ok = true;
    if (front) {
      *qk = h.qk0 + (size_t)r0 * h.Hd;
      ok = h.part->refill(h.st) == hipSuccess && h.stat->refill(h.st) == hipSuccess && h.xc->refill(h.st) == hipSuccess;
      if (ok && h.q->ws_fill)   // the caller's 32-bit pattern in the interiors (e.g. +inf: a chunk that must not be read poisons its row)
        ok = hipMemsetD32Async((hipDeviceptr_t)h.part->interior(), (int)h.q->ws_fill, h.part_in, h.st) == hipSuccess &&
             hipMemsetD32Async((hipDeviceptr_t)h.stat->interior(), (int)h.q->ws_fill, h.stat_in, h.st) == hipSuccess;
    } else {
      ok = hipStreamSynchronize(h.st) == hipSuccess && hipGetLastError() == hipSuccess &&
           h.part->read_back((char*)h.q->part_all + k * h.part->total()) == hipSuccess &&
           h.stat->read_back((char*)h.q->stat_all + k * h.stat->total()) == hipSuccess &&
           h.xc->read_back((char*)h.q->xctx_all + k * h.xc->total()) == hipSuccess;
    }
    if (!ok) { return fail(h.e, RK_ERR_HIP, "debug xattn chain: a HIP call failed at the block of row %d", r0); }
    return RK_OK;
  }, &hc};
  DBG_HIP(ds, hipDeviceSynchronize());
  if ((rc = run_xattn_chain(e, st, c, &hook))) return rc;
  DBG_HIP(ds, hipStreamSynchronize(st));
  DBG_HIP(ds, hipGetLastError());
  DBG_HIP(ds, Qk.read_back(q->qk_all));
  DBG_HIP(ds, Ctx.read_back(q->ctx_all));
  return RK_OK;
}

// debug: one launch of a row kernel or device state machine on host data, every output between sentinel bands
// (include/rk_engine.h).  No kernel, grid rule or dispatch of its own: it uploads the operands and calls the launcher of the op,
// the function the production path calls.
int rk_debug_rows(rk_engine* e, rk_debug_rows_call* q) {
  if (!e || !q) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  const int op = q->op, rows = q->rows, d = q->d;
  const long R = rows;
  if (op < 1 || op > 11) return fail(e, RK_ERR_INVALID, "debug rows: op 1..11");
  if (rows <= 0 || rows > (1 << 20)) return fail(e, RK_ERR_INVALID, "debug rows: rows = %d", rows);
  const int n_steps = op == 10 ? q->n_steps : 1;
  if (n_steps < 1 || n_steps > 4096) return fail(e, RK_ERR_INVALID, "debug rows: n_steps = %d", n_steps);
  // ---- what the launch addresses: bytes of every operand (0: unused; in_opt: may be null), from the op's arguments alone ----
  long in_need[4] = {0, 0, 0, 0}, out_need[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool in_opt[4] = {false, false, false, false};
  dim3 grid(1);
  int tparam = 0, variant = 0, maxL = 0;
  auto ints = [&](int i, long n) -> const int* { return (q->in[i].data && q->in[i].off >= 0 && q->in[i].off + n * 4 <= q->in[i].bytes) ? (const int*)((const char*)q->in[i].data + q->in[i].off) : nullptr; };
  auto state = [&](int i, long n) -> const int* { return (q->out[i].interior && n * 4 <= q->out[i].bytes) ? (const int*)q->out[i].interior : nullptr; };
  const bool planning = q->plan_only != 0;
  auto bad = [&](const char* what) { return fail(e, RK_ERR_INVALID, "debug rows: op %d: %s", op, what); };
  switch (op) {
    case 1: {
      if (d <= 0 || d % 8 || d > (1 << 16) || q->vocab <= 0 || q->vocab > (1 << 22)) return bad("d (a multiple of 8) and vocab");
      in_need[0] = R * 4; in_need[1] = (long)q->vocab * d * 2;
      out_need[0] = R * d * 4; out_need[1] = R * d * 2; out_need[2] = R * 4;
      grid = grid_waves(rows); variant = q->kind != 0;
    } break;
    case 2: {
      if (q->nb <= 0 || q->nb > (1 << 16) || d <= 0) return bad("nb and d");
      in_need[0] = R * q->nb * 4; out_need[0] = R * 4;
      grid = grid_rowscale(rows);
    } break;
    case 3: {
      if (d <= 0 || d % 4 || d > 4096) return bad("d must be a multiple of 4 and at most 4096 (rmsnorm_kernel<16> holds 4096 columns)");
      if (q->src_rows <= 0 || q->src_rows > (1 << 20)) return bad("src_rows");
      in_need[0] = (long)q->src_rows * d * 4; in_need[1] = (long)d * 4; in_need[2] = R * 4; in_opt[2] = true;
      out_need[0] = R * d * 2;
      grid = grid_waves(rows); tparam = rmsnorm_nv(d);
      if (!planning) {
        if (q->in[2].data) {
          const int* m = ints(2, R);
          if (!m) return bad("row_map of rows ints");
          for (long r = 0; r < R; ++r) if (m[r] < 0 || m[r] >= q->src_rows) return bad("row_map entry outside [0, src_rows)");
        } else if (rows > q->src_rows) return bad("rows beyond src_rows without a row_map");
      }
    } break;
    case 4: case 5: {
      const int n_out = op == 4 ? q->n_out : 2;
      if (d <= 0 || d % 8 || d > (1 << 16) || q->vocab <= 0 || q->vocab > (1 << 22) || n_out <= 0 || n_out > 4096) return bad("d (a multiple of 8), vocab and n_out");
      if (op == 5 && (rows < 2 || q->false_id < 0 || q->false_id >= q->vocab || q->true_id < 0 || q->true_id >= q->vocab)) return bad("at least 2 sequences, false_id and true_id inside the vocabulary");
      in_need[0] = R * d * 2; in_need[1] = (long)q->vocab * d * 2;
      if (op == 4) {
        in_need[2] = (long)n_out * 4; out_need[0] = R * n_out * 4;
        if (!planning) {
          const int* ids = ints(2, n_out);
          if (!ids) return bad("out_ids of n_out ints");
          for (int j = 0; j < n_out; ++j) if (ids[j] < 0 || ids[j] >= q->vocab) return bad("out_ids entry outside the vocabulary");
        }
        grid = grid_waves(rows * n_out);
      } else { out_need[0] = (3 * R + R / 2) * 4; grid = grid_pairs(rows); }
    } break;
    case 6: {
      if (q->nb <= 0 || q->nb > (1 << 20)) return bad("nb");
      in_need[0] = in_need[1] = R * q->nb * 4; out_need[0] = R * 4;
      grid = dim3(rows);
    } break;
    case 7: {
      if (q->nb <= 0 || q->nb > (1 << 20) || q->n_pos < 0 || q->n_pos > (1 << 16)) return bad("nb and n_pos");
      long n_rows = R * q->n_pos;
      in_need[2] = (R + 1) * 4; in_opt[2] = true; in_need[3] = R * 4; in_opt[3] = true;
      if (!planning && q->in[2].data) {
        const int* ro = ints(2, R + 1);
        if (!ro || ro[0] < 0) return bad("row_off of rows + 1 ints from >= 0");
        for (long b = 0; b < R; ++b) if (ro[b + 1] < ro[b]) return bad("row_off must not shrink");
        n_rows = ro[R];
      }
      if (!planning && q->in[3].data) {
        const int* oi = ints(3, R);
        if (!oi) return bad("out_idx of rows ints");
        for (long b = 0; b < R; ++b) if (oi[b] < 0 || oi[b] >= rows) return bad("out_idx entry outside [0, rows)");
      }
      in_need[0] = n_rows * q->nb * 8; in_need[1] = n_rows * 4; out_need[0] = R * 4;
      grid = dim3(rows);
    } break;
    case 8: {
      const int hd = q->hd, H = q->H, n_kv = q->n_kv;
      if ((hd != 64 && hd != 128) || H <= 0 || n_kv <= 0 || H > 1024 || n_kv > 1024 || q->max_pos <= 0) return bad("hd 64 or 128, H, n_kv, max_pos");
      if (q->ld % 8 || q->ld < (H + 2 * n_kv) * hd) return bad("ld: a multiple of 8, at least (H + 2 n_kv) hd");
      in_need[0] = R * 4; in_need[1] = in_need[2] = (long)q->max_pos * (hd / 2) * 4; in_need[3] = (long)(H + 2 * n_kv) * hd * 4; in_opt[3] = true;
      out_need[0] = R * q->ld * 2;
      if (!planning) {
        const int* pos = ints(0, R);
        if (!pos) return bad("pos of rows ints");
        for (long t = 0; t < R; ++t) if (pos[t] < 0 || pos[t] >= q->max_pos) return bad("pos entry outside the tables");
      }
      grid = dim3(rows); tparam = hd; variant = q->in[3].data != nullptr;
    } break;
    case 11: {   // op 8 with Qwen3's q / k head norm: 128 wide, in3 = the norm weights q | k (required), eps
      const int hd = q->hd, H = q->H, n_kv = q->n_kv;
      if (hd != 128 || H <= 0 || n_kv <= 0 || H > 1024 || n_kv > 1024 || q->max_pos <= 0 || !(q->eps > 0.f)) return bad("hd 128, H, n_kv, max_pos, eps > 0");
      if (q->ld % 8 || q->ld < (H + 2 * n_kv) * hd) return bad("ld: a multiple of 8, at least (H + 2 n_kv) hd");
      in_need[0] = R * 4; in_need[1] = in_need[2] = (long)q->max_pos * (hd / 2) * 4; in_need[3] = 2L * hd * 4;
      out_need[0] = R * q->ld * 2;
      if (!planning) {
        const int* pos = ints(0, R);
        if (!pos) return bad("pos of rows ints");
        for (long t = 0; t < R; ++t) if (pos[t] < 0 || pos[t] >= q->max_pos) return bad("pos entry outside the tables");
      }
      grid = dim3(rows); tparam = hd; variant = 2;
    } break;
    case 9: {
      const int hd = q->hd, H = q->H, n_kv = q->n_kv;
      if ((hd != 64 && hd != 128) || H <= 0 || n_kv <= 0 || H > 1024 || n_kv > 1024 || q->P <= 0 || q->P > (1 << 20)) return bad("hd 64 or 128, H, n_kv, P");
      if (q->ld % 8 || q->ld < (H + 2 * n_kv) * hd) return bad("ld: a multiple of 8, at least (H + 2 n_kv) hd");
      const bool slots = q->in[2].data != nullptr;
      if (slots && (q->n_slots <= 0 || q->n_slots > (1 << 16))) return bad("n_slots");
      const int* so = ints(1, R + 1);
      if (!so || so[0] != 0) return bad("seq_off of rows + 1 ints from 0");
      for (long b = 0; b < R; ++b) { if (so[b + 1] < so[b]) return bad("seq_off must not shrink"); maxL = std::max(maxL, so[b + 1] - so[b]); }
      if (maxL < 1 || maxL > (1 << 16)) return bad("the longest sequence has 1..65536 rows");
      in_need[0] = (long)so[R] * q->ld * 2; in_need[1] = (R + 1) * 4; in_need[2] = R * 4; in_opt[2] = true;
      out_need[0] = 2L * (slots ? q->n_slots : rows) * n_kv * q->P * hd * 2;
      grid = grid_kv_fill(maxL, rows); tparam = hd; variant = slots;
    } break;
    default: {
      const int kind = q->kind;
      if (kind < 0 || kind > 2) return bad("kind 0..2");
      const long A = kind == 2 ? std::max<long>(R, q->max_admit) : R;
      if (kind == 2 && (q->max_admit < 0 || q->max_admit > (1 << 20))) return bad("max_admit");
      in_need[0] = (long)n_steps * A * 4;
      variant = kind;
      if (planning) break;
      if (kind == 0) {
        if (q->dec_len <= 0 || q->max_new <= 0 || q->dec_len > (1 << 16) || q->max_new > (1 << 16)) return bad("dec_len and max_new");
        in_need[1] = (long)q->dec_len * 4;
        out_need[0] = 16; out_need[1] = R * 4; out_need[2] = R * q->max_new * 4; out_need[3] = R * 4;
        const int* st = state(0, 4);
        if (!st || st[0] < 0) return bad("st of 4 ints with st[0] >= 0");
      } else if (kind == 1) {
        const int* st = state(0, 16);
        if (!st || st[0] < 0 || st[3] < 0 || st[3] > 8 || st[4] <= 0 || st[4] > (1 << 16)) return bad("st of 16 ints: n >= 0, n_eos in 0..8, max_new > 0");
        in_need[1] = R * 4;
        out_need[0] = 64; out_need[1] = out_need[2] = out_need[4] = R * 4; out_need[3] = R * st[4] * 4;
      } else {
        const int* st = state(0, 16);
        if (!st || st[2] < 0 || st[2] > 8 || st[4] <= 0 || st[4] > (1 << 16)) return bad("st of 16 ints: n_eos in 0..8, cap > 0");
        out_need[0] = 64;
        for (int i = 1; i <= 7; ++i) out_need[i] = R * 4;
        out_need[6] = R * st[4] * 4;
        const int* col = state(2, R);
        if (!col) return bad("col of rows ints");
        for (long b = 0; b < R; ++b) if (col[b] < 0) return bad("col entry negative");
        in_need[1] = (long)n_steps * (1 + 3L * q->max_admit) * 4; in_opt[1] = true;
        if (q->in[1].data) {
          const int* ad = ints(1, (long)n_steps * (1 + 3L * q->max_admit));
          if (!ad) return bad("admit script of n_steps x (1 + 3 max_admit) ints");
          for (int s = 0; s < n_steps; ++s) {
            const int n = ad[(long)s * (1 + 3L * q->max_admit)];
            if (n < -1 || n > q->max_admit) return bad("admit count outside -1..max_admit");
          }
        }
      }
    } break;
  }
  q->out_grid[0] = (int)grid.x; q->out_grid[1] = (int)grid.y; q->out_grid[2] = (int)grid.z; q->out_tparam = tparam; q->out_variant = variant;
  if (planning) return RK_OK;
  // ---- extents against what the caller gave ----
  for (int i = 0; i < 4; ++i) {
    const rk_debug_rows_in& b = q->in[i];
    if (!in_need[i] || (in_opt[i] && !b.data)) continue;
    if (!b.data || b.off < 0 || b.off % 16 || b.off + in_need[i] > b.bytes)
      return fail(e, RK_ERR_INVALID, "debug rows: op %d: input %d needs %ld bytes at offset %ld (a multiple of 16) of %ld", op, i, in_need[i], (long)b.off, (long)b.bytes);
  }
  for (int i = 0; i < 8; ++i) {
    const rk_debug_rows_out& b = q->out[i];
    if (!out_need[i]) continue;
    if (!band_out_ok(b, out_need[i], BAND_AT_LEAST))
      return fail(e, RK_ERR_INVALID, "debug rows: op %d: output %d needs %ld of %ld bytes, interior, all and a band of 64 bytes or more (a multiple of 16)", op, i, out_need[i], (long)b.bytes);
  }
  DebugScratch ds(e, "debug rows");
  char* din[4] = {nullptr, nullptr, nullptr, nullptr};      // the kernels' pointers
  char* dout[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  Banded outs[8];
  for (int i = 0; i < 4; ++i) {
    const rk_debug_rows_in& b = q->in[i];
    if (!in_need[i] || !b.data) continue;
    char* p = ds.up<char>(b.data, (size_t)b.bytes);
    din[i] = p ? p + b.off : nullptr;
  }
  for (int i = 0; i < 8; ++i) {
    if (!out_need[i]) continue;
    outs[i] = ds.banded(q->out[i]);
    dout[i] = outs[i].interior();
  }
  if ((rc = ds.ready())) return rc;
  hipStream_t st = e->slots[0].se;
  const long A = (op == 10 && q->kind == 2) ? std::max<long>(R, q->max_admit) : R, rec = 1 + 3L * q->max_admit;
  for (int s = 0; s < n_steps; ++s) {
    switch (op) {
      case 1: launch_embed(st, (const int*)din[0], (const half_t*)din[1], (float*)dout[0], rows, d, q->vocab, q->kind ? (half_t*)dout[1] : nullptr,
                           q->kind ? (float*)dout[2] : nullptr, q->xs, q->eps); break;
      case 2: launch_rowscale(st, (const float*)din[0], (float*)dout[0], rows, q->nb, d, q->eps, q->xs); break;
      case 3: launch_rmsnorm(st, (const float*)din[0], (const float*)din[1], (half_t*)dout[0], (const int*)din[2], rows, d, q->eps, q->out_scale); break;
      case 4: launch_head_rows(st, (const half_t*)din[0], (const half_t*)din[1], (const int*)din[2], (float*)dout[0], rows, q->n_out, d); break;
      case 5: launch_pair_verdict(st, (const half_t*)din[0], (const half_t*)din[1], q->false_id, q->true_id, (float*)dout[0], rows, d); break;
      case 6: launch_argmax_blocks(st, (const float*)din[0], (const int*)din[1], q->nb, (int*)dout[0], rows); break;
      case 7: launch_qlm_lse(st, (const float2*)din[0], q->nb, (const float*)din[1], q->n_pos, (const int*)din[2], (const int*)din[3], (float*)dout[0], rows); break;
      case 8: launch_rope(st, q->hd, (half_t*)dout[0], (const int*)din[0], (const float*)din[1], (const float*)din[2], q->ld, q->H + q->n_kv,
                          (const float*)din[3], q->n_kv, rows); break;
      case 11: launch_rope(st, q->hd, (half_t*)dout[0], (const int*)din[0], (const float*)din[1], (const float*)din[2], q->ld, q->H + q->n_kv,
                           nullptr, q->n_kv, rows, (const float*)din[3], q->eps); break;
      case 9: launch_kv_fill(st, q->hd, (const half_t*)din[0], (const int*)din[1], (const int*)din[2], q->n_slots,
                             kv_cache_layer(kv_layer_layout(0, din[2] ? q->n_slots : rows, q->n_kv, q->hd, q->P), dout[0], 0), q->ld, q->H, q->n_kv,
                             q->P, maxL, rows); break;
      default: {
        const int* am = (const int*)din[0] + (size_t)s * A;
        if (q->kind == 0)
          launch_greedy_advance(st, am, (int*)dout[0], (const int*)din[1], (int*)dout[1], (int*)dout[2], (int*)dout[3], rows, q->dec_len, q->max_new);
        else if (q->kind == 1)
          // (out 3 is the output, out 4 the next ids: the kernel's order)
          launch_llama_advance(st, am, GenInts{(int*)dout[0], (int*)din[1], (int*)dout[1], (int*)dout[2], (int*)dout[4], (int*)dout[3]}, rows);
        else {
          const int* host_rec = din[1] ? (const int*)((const char*)q->in[1].data + q->in[1].off) + (size_t)s * rec : nullptr;
          const int n_admit = host_rec ? host_rec[0] : -1;
          const int* adm = n_admit >= 0 ? (const int*)din[1] + (size_t)s * rec + 1 : nullptr;
          auto o = [&](int i) { return (int*)dout[i]; };     // out 6 is the output, out 7 the next ids; no admit array, no drafting
          const SessionInts si{o(0), o(1), o(2), o(3), o(4), o(5), o(7), nullptr, o(6)};
          launch_session_advance(st, am, si, rows, SessionAdmit{adm, n_admit >= 0 ? n_admit : 0});
        }
      } break;
    }
    DBG_HIP(ds, hipStreamSynchronize(st));
    DBG_HIP(ds, hipGetLastError());
    DBG_HIP(ds, read_back_step(outs, q->out, 8, s));
  }
  return RK_OK;
}

// debug: a drafting session's accept machine and proposer on host state, one scripted launch group per step (include/rk_engine.h).
// No kernel, grid rule or dispatch of its own: launch_session_advance_draft and launch_draft_lookup, in the order session_admit,
// rk_llama_session_run's step and rk_debug_session_drafts call them.  Every extent the two kernels rely on is checked on the host
// before anything is allocated.
int rk_debug_draft_steps(rk_engine* e, rk_debug_draft_steps_call* q) {
  if (!e || !q) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  auto bad = [&](const char* what) { return fail(e, RK_ERR_INVALID, "debug draft steps: %s", what); };
  const int S = q->n_slots, g1 = q->g1, n_steps = q->n_steps, MA = q->max_admit, MT = q->max_tokens;
  if (S <= 0 || S > (1 << 16) || g1 < 1 || g1 > 8) return bad("n_slots in 1..65536 and g1 in 1..8");
  if (n_steps < 1 || n_steps > 4096 || MA < 0 || MA > (1 << 16) || MT < 0 || MT > (1 << 20)) return bad("n_steps in 1..4096, max_admit, max_tokens");
  const long A = std::max<long>((long)S * g1, MA), rec = 4 + A + 3L * MA + (MA + 1) + MT;
  if (!q->script || q->script_ints < (int64_t)n_steps * rec) return bad("script of n_steps x (4 + max(n_slots g1, max_admit) + 3 max_admit + max_admit + 1 + max_tokens) ints");
  auto state = [&](int i, long n) -> const int* { return (q->state[i].interior && n * 4 <= q->state[i].bytes) ? (const int*)q->state[i].interior : nullptr; };
  const int* st0 = state(0, INTS_HEAD);
  if (!st0) return bad("st of 16 ints");
  const int n_eos = st0[SES_N_EOS], max_len = st0[SES_MAX_LEN], cap = st0[SES_CAP], nmin = st0[SES_NGRAM_MIN], nmax = st0[SES_NGRAM_MAX];
  if (n_eos < 0 || n_eos > 8) return bad("n_eos = st[2] in 0..8");
  if (max_len < 1 || max_len > (1 << 20) || cap < 1 || cap > (1 << 16)) return bad("max_len = st[3] in 1..2^20, cap = st[4] in 1..65536");
  if (nmin < 1 || nmin > nmax || nmax > 8) return bad("1 <= ngram_min = st[5] <= ngram_max = st[6] <= 8");
  if ((long)S * max_len * 4 > (1L << 31)) return bad("hist beyond 2^31 bytes");
  // st, len, col, max_new, done, out, rnext, rpos, rlive, dlen, nstep, tabn, tab, hist
  const long need[RK_DEBUG_DRAFT_ARRAYS] = {INTS_HEAD, S, S, S, S, (long)S * cap, (long)S * g1, (long)S * g1, (long)S * g1, S, S, S, (long)S * cap, (long)S * max_len};
  for (int i = 0; i < RK_DEBUG_DRAFT_ARRAYS; ++i) {
    const rk_debug_rows_out& b = q->state[i];
    if (!band_out_ok(b, need[i] * 4, BAND_EXACT))
      return fail(e, RK_ERR_INVALID, "debug draft steps: state array %d has %ld bytes (%ld given) and needs interior, all and a band of 64 bytes or more (a multiple of 16)", i, need[i] * 4, (long)b.bytes);
  }
  {
    const int *len = state(1, S), *col = state(2, S), *mn = state(3, S), *dn = state(4, S), *dlen = state(9, S), *tabn = state(11, S);
    for (int s = 0; s < S; ++s) {
      if (tabn[s] < -1 || tabn[s] > cap) return bad("tabn entry outside -1..cap");
      if (dn[s]) continue;
      if (len[s] < 1 || mn[s] < 1 || mn[s] > cap || (long)len[s] + mn[s] > max_len) return bad("an active slot needs len >= 1, 1 <= max_new <= cap and len + max_new <= max_len");
      if (col[s] < 0 || col[s] >= mn[s]) return bad("an active slot's col must lie in [0, max_new)");
      if (dlen[s] < 0 || dlen[s] >= g1) return bad("an active slot's dlen must lie in [0, g1)");
    }
  }
  for (int s = 0; s < n_steps; ++s) {
    const int* r = q->script + (size_t)s * rec;
    const int kind = r[0], n = r[1];
    if (kind == 0) continue;
    if (kind == 1) {
      if (n < 0 || n > MA) return bad("admit count outside 0..max_admit");
      const int *adm = r + 4 + A, *so = adm + 3L * MA;
      std::vector<char> taken(S, 0);
      for (int b = 0; b < n; ++b) {
        const int slot = adm[b], L = adm[n + b], m = adm[2 * n + b];
        if (L < 1) return bad("an admitted prompt has at least one token");
        if (m < 1 || m > cap) return bad("an admit's max_new must lie in 1..cap");
        if ((long)L + m > max_len) return bad("an admit's len + max_new exceeds max_len");
        if (so[b] < 0 || (long)so[b] + L > MT) return bad("an admitted prompt lies outside the step's tokens");
        if (slot < 0 || slot >= S) continue;                 // (the kernels skip it)
        if (taken[slot]) return bad("a slot named twice in one admit");
        taken[slot] = 1;
      }
    } else if (kind == 2) {
      if (r[2] < 0 || r[2] >= S) return bad("a table change's slot is out of range");
      if (n < -1 || n > cap || n > MT) return bad("a table holds -1 (back to the lookup) or 0..min(cap, max_tokens) tokens");
    } else return bad("script kind 0 (step), 1 (admit) or 2 (table)");
  }
  DebugScratch ds(e, "debug draft steps");
  int* dscript = ds.up<int>(q->script, (size_t)n_steps * rec);
  Banded arrays[RK_DEBUG_DRAFT_ARRAYS]; int* da[RK_DEBUG_DRAFT_ARRAYS];
  for (int i = 0; i < RK_DEBUG_DRAFT_ARRAYS; ++i) {
    arrays[i] = ds.banded(q->state[i]);
    da[i] = arrays[i].interior<int>();
  }
  if ((rc = ds.ready())) return rc;
  hipStream_t stream = e->slots[0].se;
  // (no pos, next, admit: a drafting session's kernels take none of them)
  const SessionInts d{da[0], da[1], da[2], da[3], da[4], nullptr, nullptr, nullptr, da[5], da[6], da[7], da[8], da[9], da[10], da[11], da[12], da[13]};
  for (int s = 0; s < n_steps; ++s) {
    const int* r = q->script + (size_t)s * rec;
    const int* dr = dscript + (size_t)s * rec;
    const int kind = r[0], n = r[1];
    if (kind == 0) launch_session_advance_draft(stream, dr + 4, d, S, g1);
    else if (kind == 1) launch_session_advance_draft(stream, dr + 4, d, S, g1, SessionAdmit{dr + 4 + A, n, dr + 4 + A + 3L * MA + MA + 1, dr + 4 + A + 3L * MA});
    else {
      const int slot = r[2];
      if (n > 0) DBG_HIP(ds, hipMemcpy(d.tab + (size_t)slot * cap, r + 4 + A + 3L * MA + MA + 1, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
      DBG_HIP(ds, hipMemcpy(d.tabn + slot, &n, sizeof(int), hipMemcpyHostToDevice));
    }
    launch_draft_lookup(stream, d, S, g1);
    DBG_HIP(ds, hipStreamSynchronize(stream));
    DBG_HIP(ds, hipGetLastError());
    DBG_HIP(ds, read_back_step(arrays, q->state, RK_DEBUG_DRAFT_ARRAYS, s));
  }
  return RK_OK;
}

int rk_debug_gemm(rk_engine* e, const uint16_t* A, const uint16_t* W, float* C, int M, int N, int K, int use_glds) {
  if (!e || !A || !W || !C) return RK_ERR_INVALID;
  if (K % 64 || N % 4) return fail(e, RK_ERR_INVALID, "debug gemm needs K%%64==0 and N%%4==0");
  if (M <= 0) return RK_OK;
  // 2: the weight-streaming family, 3: the few-row GEMV family (M <= 16)
  rk_debug_gemm_call q{};
  q.epi = EPI_STORE_F32; q.family = use_glds == 3 ? 2 : (use_glds >= 2 ? 1 : 0);
  q.M = M; q.N = N; q.K = K; q.lda = q.ldw = K; q.ldc = N;
  q.A = A; q.a_elems = (int64_t)M * K; q.W = W; q.w_elems = (int64_t)N * K;
  q.C = C; q.c_elems = (int64_t)M * N; q.band_rows = 256; q.batch = 1;
  std::vector<float> all((size_t)(M + 512) * N);
  q.C_out = all.data();
  const int saved = e->opt.glds;
  e->opt.glds = use_glds != 0;
  const int rc = rk_debug_gemm_ex(e, &q);
  e->opt.glds = saved;
  if (rc) return rc;
  memcpy(C, all.data() + (size_t)256 * N, (size_t)M * N * 4);
  return RK_OK;
}

// debug/measurement: time `iters` back-to-back launches of the engine's GEMM at one shape (random fp16 operands on
// the device, epilogue `epi` as in GemmEpi).  *out_ms = average per launch from HIP events on the encoder stream.
int rk_debug_gemm_bench(rk_engine* e, int M, int N, int K, int epi, int iters, float* out_ms) {
  if (!e || !out_ms || M <= 0 || N <= 0 || K <= 0 || iters <= 0) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if (K % 64 || N % 4) return fail(e, RK_ERR_INVALID, "gemm bench needs K%%64==0 and N%%4==0");
  // (RK_BENCH_PAD: extra halfs per operand row - a leading dimension that is not a power of two; measurement of the L2 channel spread)
  const char* pad_env = getenv("RK_BENCH_PAD");
  const int pad = pad_env ? atoi(pad_env) : 0;
  const int ldk = K + pad;
  const size_t na = (size_t)M * ldk, nw = (size_t)N * ldk, nc = (size_t)M * N;
  DebugScratch ds(e, "gemm bench");                       // (every return below gives the operands back)
  const std::vector<half_t> h = lcg_halfs(std::max(na, nw), 12345u);
  half_t* dA = ds.up<half_t>(h.data(), na);
  half_t* dW = ds.up<half_t>(h.data(), nw);
  float* dC = ds.alloc<float>(nc, 0);
  const int ldc = EPI_IS_GATED(epi) ? N / 2 : N;
  // (RK_BENCH_FOLD: the residual epilogue as the encoder runs it - producer side of the folded RMSNorm: fp16 stream copy + sums of squares)
  GemmFold fold;
  if (getenv("RK_BENCH_FOLD") && atoi(getenv("RK_BENCH_FOLD")) && epi == EPI_RESID_F32) {
    fold.xraw = ds.alloc<half_t>(nc); fold.ssq = ds.alloc<float>((size_t)M * ((N + 31) / 32));
  }
  RC(ds.failed());
  const Gemm c = Gemm(PC_OTHER, epi, dA, ldk, dW, ldk, dC, ldc, M, N, K).with(fold);
  for (int i = 0; i < 2; ++i) RC(gemm(e, e->slots[0].se, c));
  HIPCHK(e, hipEventRecord(e->t0, e->slots[0].se));
  for (int i = 0; i < iters; ++i) RC(gemm(e, e->slots[0].se, c));
  HIPCHK(e, hipEventRecord(e->t1, e->slots[0].se));
  HIPCHK(e, hipEventSynchronize(e->t1));
  float ms = 0;
  HIPCHK(e, hipEventElapsedTime(&ms, e->t0, e->t1));
  HIPCHK(e, hipGetLastError());
  *out_ms = ms / iters;
  return RK_OK;
}

// debug: the decoder graph table and run_graphed's counters (host state only: nothing is launched or waited for)
int rk_debug_graph_stats(rk_engine* e, rk_debug_graph_stats_t* out) {
  if (!e || !out) return RK_ERR_INVALID;
  int ready = 0;
  for (const auto& kv : e->graphs) ready += kv.second.exec != nullptr;
  const auto& n = e->graph_count;
  out->n_keys = (int)e->graphs.size(); out->n_ready = ready; out->max_keys = RK_GRAPH_CACHE_KEYS;
  out->eager = n.eager; out->captures = n.captures; out->replays = n.replays; out->failed = n.failed; out->evictions = n.evictions;
  return RK_OK;
}

// debug: where the grown buffers are, how much they hold, and their move counters (host state only, like rk_debug_graph_stats)
int rk_debug_buffers(rk_engine* e, rk_debug_buffers_t* out) {
  if (!e || !out) return RK_ERR_INVALID;
  int i = 0;
  auto put = [&](const auto& b) { out->addr[i] = (uint64_t)(uintptr_t)b.p; out->cap[i] = (uint64_t)b.cap; ++i; };
  put(e->logits); put(e->amax_val); put(e->amax_idx); put(e->kv_cache); put(e->gen_buf); put(e->lkv); put(e->lpart); put(e->lints);   // RK_DEBUG_BUFFER_NAMES
  static_assert(RK_DEBUG_N_BUFFERS == 8, "one put per grown buffer");
  out->amax_gen = e->amax_gen; out->kv_gen = e->kv_gen; out->lkv_gen = e->lkv_gen;
  return RK_OK;
}

// debug: sample_rows_kernel alone on host logits, through the launcher the sampling head calls (include/rk_engine.h).  Memory of its
// own, freed on return; works on an engine of either family (every width comes from the call).
int rk_debug_sample(rk_engine* e, rk_debug_sample_call* q) {
  if (!e || !q) return RK_ERR_INVALID;
  if (q->rows <= 0 || q->rows > (1 << 20) || q->logit_rows <= 0 || q->logit_rows > q->rows || q->V <= 0 || q->V > sampling::MAX_VOCAB)
    return fail(e, RK_ERR_INVALID, "rk_debug_sample: rows %d (1 .. 2^20), logit_rows %d (1 .. rows), V %d (1 .. %d)", q->rows, q->logit_rows, q->V, sampling::MAX_VOCAB);
  if (!q->logits || !q->seeds || !q->index || !q->out_token) return fail(e, RK_ERR_INVALID, "rk_debug_sample: null logits, seeds, index or out_token");
  if (!(q->temperature > 0.f) || std::isinf(q->temperature) || q->top_k < 0 || !(q->top_p > 0.f && q->top_p <= 1.f))
    return fail(e, RK_ERR_INVALID, "rk_debug_sample: temperature %g (> 0), top_k %d (>= 0), top_p %g (in (0, 1])", (double)q->temperature, q->top_k, (double)q->top_p);
  for (int r = 0; r < q->rows; ++r)
    if (q->index[r] < 0) return fail(e, RK_ERR_INVALID, "rk_debug_sample: token index %d of row %d is negative", q->index[r], r);
  int rc = set_device(e);
  if (rc) return rc;
  const size_t rows = (size_t)q->rows, nl = (size_t)q->logit_rows * q->V;
  hipStream_t st = e->slots[0].se;
  std::vector<int> ints(4 * rows, -1);                     // index[rows] | token[rows] | kept[rows][2]
  memcpy(ints.data(), q->index, rows * sizeof(int));
  DebugScratch ds(e, "rk_debug_sample");
  float* d_logits = ds.up<float>(q->logits, nl);
  unsigned long long* d_seeds = ds.up<unsigned long long>(q->seeds, rows);
  int* d_ints = ds.up<int>(ints.data(), ints.size());
  if ((rc = ds.failed())) return rc;
  const rk_engine::Sampling sp{q->temperature, q->top_k, q->top_p};
  launch_sample_rows(st, d_logits, q->logit_rows, q->V, sp, d_seeds, nullptr, d_ints, nullptr, 0, d_ints + rows, d_ints + 2 * rows, q->rows);
  DBG_HIP(ds, hipStreamSynchronize(st));
  DBG_HIP(ds, hipGetLastError());
  DBG_HIP(ds, hipMemcpy(ints.data(), d_ints, ints.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < rows; ++r) {
    q->out_token[r] = ints[rows + r];
    if (q->out_kept_k) q->out_kept_k[r] = ints[2 * rows + 2 * r];
    if (q->out_kept_p) q->out_kept_p[r] = ints[2 * rows + 2 * r + 1];
  }
  return RK_OK;
}

// debug: the FP8 cache's quantiser on host vectors (include/rk_engine.h): kv8_quant16 through launch_kv8_quant
int rk_debug_kv8_quant(rk_engine* e, const uint16_t* x, int n, uint8_t* q_out, int8_t* exp_out, uint16_t* deq_out) {
  if (!e || !x) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if (e->family != 1 || !e->finalized) return fail(e, RK_ERR_STATE, "debug kv8 quant: a finalized Llama-family engine");
  if (n <= 0 || n > (1 << 22)) return fail(e, RK_ERR_INVALID, "debug kv8 quant: n in 1 .. 2^22 vectors (got %d)", n);
  hipStream_t st = e->slots[0].se;
  DebugScratch ds(e, "debug kv8 quant");
  const size_t N = (size_t)n * 128;
  half_t* dX = ds.up<half_t>(x, N);
  uint8_t* dQ = ds.alloc<uint8_t>(N, RK_DEBUG_SENTINEL);
  int8_t* dE = ds.alloc<int8_t>((size_t)n, RK_DEBUG_SENTINEL);
  half_t* dD = ds.alloc<half_t>(N, RK_DEBUG_SENTINEL);
  if ((rc = ds.ready())) return rc;
  launch_kv8_quant(st, dX, n, dQ, dE, dD);
  DBG_HIP(ds, hipStreamSynchronize(st));
  DBG_HIP(ds, hipGetLastError());
  if (q_out) DBG_HIP(ds, hipMemcpy(q_out, dQ, N, hipMemcpyDeviceToHost));
  if (exp_out) DBG_HIP(ds, hipMemcpy(exp_out, dE, (size_t)n, hipMemcpyDeviceToHost));
  if (deq_out) DBG_HIP(ds, hipMemcpy(deq_out, dD, N * 2, hipMemcpyDeviceToHost));
  return RK_OK;
}

// debug: one step's attention of an FP8-cache engine on host operands (include/rk_engine.h).  No launch code of its own: the
// caller's fp16 cache goes through launch_kv8_quant into the layout of the mode (kv_layer_layout), then plan_llama_dec_attn and
// launch_llama_dec_attn - llama_step_rows' call.
int rk_debug_kv8_step(rk_engine* e, rk_debug_kv8_step_call* q) {
  if (!e || !q) return RK_ERR_INVALID;
  int rc = set_device(e);
  if (rc) return rc;
  if (!e->finalized || e->family != 1 || !e->kv_fp8) return fail(e, RK_ERR_STATE, "debug kv8 step: a finalized Llama-family engine with an FP8 K / V cache (rk_llama_set_kv_fp8)");
  const int B = q->n_seq, H = q->H, n_kv = q->n_kv, P = q->P, hd = 128, g1 = q->g1 > 1 ? q->g1 : 1;
  if (B <= 0 || B > 4096 || H <= 0 || H > 1024 || n_kv <= 0 || H % n_kv || P <= 0 || P > (1 << 20) || q->mode < 0 || q->mode > 1)
    return fail(e, RK_ERR_INVALID, "debug kv8 step: n_seq, H, n_kv (divides H), P and mode 0 / 1");
  if (q->g1 < 0 || q->g1 > 8 || B % g1) return fail(e, RK_ERR_INVALID, "debug kv8 step: g1 in 0..8 and n_seq a multiple of it (g1 = %d, n_seq = %d)", q->g1, B);
  if (q->ld < (H + 2 * n_kv) * hd || q->ld % 8 || q->ld > (1 << 20)) return fail(e, RK_ERR_INVALID, "debug kv8 step: ld %d >= %d, a multiple of 8", q->ld, (H + 2 * n_kv) * hd);
  if (q->qk_norm && (e->window > 0 || q->qkv_bias || !(q->qk_eps > 0.f)))
    return fail(e, RK_ERR_STATE, "debug kv8 step: the step with the q / k head norm takes no window, no qkv_bias and qk_eps > 0");
  LlamaDecAttnPlan lp = plan_llama_dec_attn(e, B, P, H, n_kv);
  lp.kv8 = q->mode ? 2 : 1;                                  // (the engine's option chooses between the two; the call names one)
  const int rows = B / g1;
  const KvLayerLayout kl = kv_layer_layout(lp.kv8, rows, n_kv, hd, P), k16 = kv_layer_layout(0, rows, n_kv, hd, P);   // the step's cache; the caller's
  q->out_R = lp.R; q->out_nch = lp.nch; q->out_pe = kv_layer_layout(1, rows, n_kv, hd, P).pe;
  if (H % lp.R) return fail(e, RK_ERR_STATE, "debug kv8 step: R = %d does not divide %d heads", lp.R, H);
  if (q->plan_only) return RK_OK;
  if (!q->qkv || !q->pos || !q->cos_t || !q->sin_t || !q->cache || (g1 > 1 && !q->live)) return fail(e, RK_ERR_INVALID, "debug kv8 step: qkv, pos, cos_t, sin_t, cache (and live with g1 > 1)");
  for (int b = 0; b < B; ++b)
    if (q->pos[b] < 0 || q->pos[b] >= P || q->pos[b] >= q->max_pos) return fail(e, RK_ERR_INVALID, "debug kv8 step: pos[%d] = %d outside the cache of %d / the tables of %d", b, q->pos[b], P, q->max_pos);
  const size_t heads = (size_t)rows * n_kv, nvec = heads * P, cache_bytes = kl.bytes;   // nvec key vectors and as many value vectors
  const size_t ctx_bytes = (size_t)B * H * hd * 2, part_bytes = (size_t)B * H * lp.nch * ldc_pstr(hd) * 4;
  if (nvec > (1u << 22) || !band_out_ok(q->ctx, (int64_t)ctx_bytes, BAND_EXACT) || !band_out_ok(q->part, (int64_t)part_bytes, BAND_EXACT) ||
      !band_out_ok(q->cache_out, (int64_t)cache_bytes, BAND_EXACT))
    return fail(e, RK_ERR_INVALID, "debug kv8 step: ctx (%zu bytes), part (%zu) and cache_out (%zu) as rk_debug_rows_out with bands of 64 bytes or more, multiples of 16; at most 2^22 cached vectors", ctx_bytes, part_bytes, cache_bytes);
  hipStream_t st = e->slots[0].se;
  DebugScratch ds(e, "debug kv8 step");
  half_t* dQkv = ds.up<half_t>(q->qkv, (size_t)B * q->ld);
  half_t* dC16 = ds.up<half_t>(q->cache, k16.bytes / 2);
  int* dPos = ds.up<int>(q->pos, (size_t)B);
  float* dCos = ds.up<float>(q->cos_t, (size_t)q->max_pos * 64);
  float* dSin = ds.up<float>(q->sin_t, (size_t)q->max_pos * 64);
  float* dBias = q->qkv_bias ? ds.up<float>(q->qkv_bias, (size_t)(H + 2 * n_kv) * hd) : nullptr;
  float* dQkn = q->qk_norm ? ds.up<float>(q->qk_norm, (size_t)2 * hd) : nullptr;
  int* dLive = g1 > 1 ? ds.up<int>(q->live, (size_t)B) : nullptr;
  uint8_t* dQ = ds.alloc<uint8_t>(2 * nvec * hd);            // the quantiser's dense outputs [2][nvec]: bytes, exponents, dequantised
  int8_t* dE = ds.alloc<int8_t>(2 * nvec);
  half_t* dD = ds.alloc<half_t>(2 * nvec * hd);
  const Banded Ctx = ds.banded(q->ctx), Part = ds.banded(q->part);
  const Banded Cache = ds.banded(BandSpan{cache_bytes, (size_t)q->cache_out.band});   // (its interior comes from the quantiser)
  if ((rc = ds.ready())) return rc;
  launch_kv8_quant(st, dC16, (int)(2 * nvec), dQ, dE, dD);
  const Kv8Cache cc = kv_cache_layer(kl, Cache.interior<char>(), 0);
  if (q->mode) DBG_HIP(ds, hipMemcpyAsync(cc.kc, dD, k16.bytes, hipMemcpyDeviceToDevice, st));   // (dense K | V: the fp16 layout itself)
  else {
    uint8_t* const by[2] = {(uint8_t*)cc.kc, (uint8_t*)cc.vc};
    int8_t* const ex[2] = {cc.ke, cc.ve};
    for (int s = 0; s < 2; ++s) {
      DBG_HIP(ds, hipMemcpyAsync(by[s], dQ + s * nvec * hd, nvec * hd, hipMemcpyDeviceToDevice, st));
      DBG_HIP(ds, hipMemsetAsync(ex[s], 0, heads * cc.pe, st));   // (the pad behind P: no kernel reads it as a visible key's)
      DBG_HIP(ds, hipMemcpy2DAsync(ex[s], (size_t)cc.pe, dE + s * nvec, (size_t)P, (size_t)P, heads, hipMemcpyDeviceToDevice, st));
    }
  }
  const float scale_log2e = (1.0f / std::sqrt((float)hd)) * 1.4426950408889634f;
  const LlamaDecAttnArgs aa{dQkv, nullptr, nullptr /* kc, vc: cc's, in the launch */, dPos, dCos, dSin, Part.interior<float>(), Ctx.interior<half_t>(), q->ld, H, n_kv, P, lp.nch, scale_log2e, dBias, 0, dQkn, q->qk_eps};
  launch_llama_dec_attn(e, st, lp, aa, B, g1, dLive, cc);
  DBG_HIP(ds, hipStreamSynchronize(st));
  DBG_HIP(ds, hipGetLastError());
  DBG_HIP(ds, Ctx.read_back(q->ctx.all));
  DBG_HIP(ds, Part.read_back(q->part.all));
  DBG_HIP(ds, Cache.read_back(q->cache_out.all));
  return RK_OK;
}

int64_t rk_debug_read(rk_engine* e, const char* name, float* out, int64_t max_floats) {
  if (!e || !name || !out) return RK_ERR_INVALID;
  if (set_device(e)) return RK_ERR_HIP;
  if (sync_all(e)) return RK_ERR_HIP;
  if (!strcmp(name, "occupancy")) {   // resident workgroups per CU the runtime computes for the main kernels
    if (max_floats < 6) return RK_ERR_INVALID;
    int n = 0;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, attn_enc_kernel, 256, 0); out[0] = (float)n;
    out[1] = 0.f;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gemm_f16_kernel<EPI_STORE_F16, true>, 256, GEMM_LDS_BYTES); out[2] = (float)n;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gemm_pp2_kernel<EPI_STORE_F16, 0>, 512, 163840); out[3] = (float)n;
    out[4] = 0.f;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, rmsnorm_kernel<4>, 256, 0); out[5] = (float)n;
    if (max_floats >= 10) {
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, attn_enc_dma_kernel<1>, 384, ATTD_LDS_BYTES); out[6] = (float)n;
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, attn_enc_dma_kernel<2>, 768, 2 * ATTD_LDS_BYTES); out[7] = (float)n;
      out[8] = out[9] = 0.f;
      return 10;
    }
    return 6;
  }
  const Slot& sl = e->slots[0];
  const std::string n(name);
  const int I = e->inner, dm = e->d.d_model;
  const void* src = nullptr; int64_t cnt = 0; bool is_half = true;
  if (n == "enc_hidden") { src = sl.enc.hidden; cnt = (int64_t)sl.T * dm; is_half = false; }
#ifdef RK_MEASURE
  else if (n == "attn_trace" && e->attn_trace) { src = e->attn_trace; cnt = 12 * 16 * 16; is_half = false; }
#endif
  else if (n == "enc_out") { src = sl.enc_out; cnt = (int64_t)sl.T * dm; }
  else if (n == "qkv") { src = sl.qkv; cnt = (int64_t)sl.T * 3 * I; }
  else if (n == "ctx") { src = sl.ctx; cnt = (int64_t)sl.T * I; }
  else if (n == "xn") { src = sl.enc.xn; cnt = (int64_t)sl.T * dm; }
  else if (n == "llama_last") { src = sl.dlast; cnt = (int64_t)sl.n_seq * dm; }   // final-normed last rows of the most recent Llama call (a session's step: n_slots rows)
  else if (n == "dec_hidden") { src = sl.dec.hidden; cnt = (int64_t)sl.n_seq * e->d.max_dec_len * dm; is_half = false; }
  else if (n == "lkv") { src = e->lkv.p; cnt = (int64_t)(e->lkv.cap / 2); is_half = false; }   // RAW: the Llama K / V cache's bytes, four per float slot, in its layout
  else return fail(e, RK_ERR_INVALID, "unknown buffer %s", name);
  cnt = std::min(cnt, max_floats);
  if (is_half) {
    std::vector<half_t> tmp(cnt);
    if (hipMemcpy(tmp.data(), src, cnt * 2, hipMemcpyDeviceToHost) != hipSuccess) return fail(e, RK_ERR_HIP, "copy failed");
    for (int64_t i = 0; i < cnt; ++i) out[i] = (float)tmp[i];
  } else if (hipMemcpy(out, src, cnt * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(e, RK_ERR_HIP, "copy failed");
  return cnt;
}

}  // extern "C"
#undef DBG_HIP
