"""FP8 step weights of the Llama engine (rk_llama_set_weight_fp8; DESIGN.md section 3 "FP8 step weights").

The design needs no tolerance of its own: with power-of-two group scales every dequantised weight is an fp16 number, so an engine in
FP8 mode is, bit for bit, the fp16 engine running on the dequantised matrices.  Held here:
  1. the engine's quantiser (quant_fp8_rows_kernel) equals tests/_fp8_ref.py byte for byte on an adversarial matrix;
  2. gemm_skinny_fp8_kernel's outputs equal, byte for byte, gemm_skinny_kernel's on the dequantised matrix - interior, guard bands,
     xraw / ssq - and lie within tests/_gemm_ref.py's rules of fp64;
  3. the model three ways (FP8 bytes, the same engine on the fp16 kernel, a plain fp16 engine loaded with the reference's dequantised
     state dict): identical tokens and logits; against the fp32 oracle on the dequantised weights within the Llama tests' bound;
  4. random norm weights (folding no longer the identity), the Qwen2 / Qwen3 / 64-wide forms, graph replay against eager launches;
  5. a four-slot session; 6. the contract."""
import numpy as np
import pytest

import _fp8_ref as F
import _gemm_ref as R
from llmrankers import _synth

pytestmark = pytest.mark.gpu
BOUND = 4e-3              # x logit scale: what the Llama prefill and step are held to (tests/test_gpu_rankr1.py, test_gpu_llama_listwise.py)
BAND_ROWS = 256
PAD = 0
STEP_MATRICES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 4096)
    kw.setdefault("max_seqs", 16)
    return RkLlamaEngine(dims, device=0, **kw).load_state(state.items())


def _state(dims, seed, unit_norms):
    state = dict(_synth.synth_state_dict(dims, seed=seed))
    if unit_norms:                      # every RMSNorm weight 1: finalize's fold W[n][k] * ln[k] is the identity
        for k in state:
            if k.endswith("layernorm.weight") or k == "model.norm.weight":
                state[k] = np.ones_like(state[k])
    return state


def _dequantised(state):
    """the state dict a plain fp16 engine needs to be the FP8 engine's model (unit norm weights: the groups run along K inside a row,
    so quantising q / k / v and gate / up one by one is quantising the fused, interleaved matrices finalize builds)"""
    out = dict(state)
    for k, v in state.items():
        if k.startswith("model.layers.") and k.endswith(".weight") and k.split(".")[-2] in STEP_MATRICES:
            out[k] = F.quantize(np.asarray(v, dtype=np.float16))[2]
    return out


@pytest.fixture(scope="module")
def eng():
    """a toy Llama engine in FP8 mode: the two debug entries take every shape from the call"""
    dims = _synth.TOY_LLAMA
    e = _engine(dims, _state(dims, 5, True), max_tokens=1024, max_seqs=8, weight_fp8=True)
    e.gemm_info = e.debug_gemm_ex(R.EPI_STORE_F32, R.STREAM, np.zeros(64, np.float16), np.zeros(64 * 64, np.float16), 1, 64, 64, plan_only=True)
    yield e
    e.close()


# ---- 1. the quantiser ------------------------------------------------------------------------------------------------------------
def test_quantiser_equals_the_reference_byte_for_byte(eng):
    """W [70][400]: a tail group of 16, N no multiple of 32; an all-zero group, absmax 60 000 (clamp at 7, saturation), absmax 1e-7
    (clamp at -15), exact ties, +-448 * 2^e boundaries (tests/_fp8_ref.py: adversarial_matrix).  Also with a row stride > K."""
    w = F.adversarial_matrix(70, 400)
    q_ref, e_ref, d_ref = F.quantize(w)
    assert e_ref.min() == F.E_MIN and e_ref.max() == F.E_MAX and (q_ref[1, :128] == 0).all()
    q, e, d = eng.debug_quant_fp8(w)
    np.testing.assert_array_equal(e, e_ref, err_msg="group exponents")
    bad = np.argwhere(q != q_ref)
    assert bad.size == 0, f"{len(bad)} bytes differ, first at {bad[0]}: engine {q[tuple(bad[0])]:#x} reference {q_ref[tuple(bad[0])]:#x} for w = {float(w[tuple(bad[0])])!r}"
    np.testing.assert_array_equal(d.view(np.uint16), d_ref.view(np.uint16), err_msg="dequantised fp16")
    wide = np.full((70, 416), np.nan, dtype=np.float16)
    wide[:, :400] = w
    q2, e2, d2 = eng.debug_quant_fp8(wide, K=400)
    assert q2.tobytes() == q.tobytes() and e2.tobytes() == e.tobytes() and d2.tobytes() == d.tobytes()
    # the dequantised matrix is a fixed point of the quantiser (tests/test_fp8_weights_host.py: its bytes and exponents may move
    # where a group's largest weight rounds down onto 448 * 2^(e - 1); its values never do)
    q3, e3, d3 = eng.debug_quant_fp8(d)
    q3_ref, e3_ref, _ = F.quantize(d)
    assert d3.tobytes() == d.tobytes() and q3.tobytes() == q3_ref.tobytes() and e3.tobytes() == e3_ref.tobytes()


# ---- 2. the kernel ---------------------------------------------------------------------------------------------------------------
# (N, K): (96, 144) the tail-only loop (9 K steps); (70 -> 72, 400) 25 steps, N no multiple of 32 (70 itself: refused, below); (64, 528) 33 steps: one trip of the
# 32-step main loop + tail; (160, 2064) 129 steps: four trips + tail, a tail exponent group of 16
SHAPES = [(96, 144), (70, 400), (64, 528), (160, 2064)]
M_ALL = [1, 5, 16, 33]    # 33: a second row slab (blockIdx.z)
# (epilogue, producer): store f16; residual f32 without / with the xraw / ssq producer; SwiGLU f16
FORMS = [(R.EPI_STORE_F16, False), (R.EPI_RESID_F32, False), (R.EPI_RESID_F32, True), (R.EPI_SWIGLU_F16, False)]
CONSUMERS = [None, "rowscale", "ssq8", "ssq66"]      # ssq_in with nb_in = 8 (the DMA path) and 66 (the plain path)


def _weights(rs, n, k):
    """normal weights at the scale of a trained projection, with groups that reach the format's edges: a tiny row (exponent clamp at
    -15, fp16-subnormal products), a large one, an all-zero group"""
    w = (rs.standard_normal((n, k)) * 0.04).astype(np.float16)
    w[n // 3] = (rs.standard_normal(k) * 2e-7).astype(np.float16)
    w[n // 2] = rs.standard_normal(k).astype(np.float16)
    w[n - 1, :min(128, k)] = 0
    return w


@pytest.mark.parametrize("consumer", CONSUMERS, ids=lambda c: c or "plain")
@pytest.mark.parametrize("epi,producer", FORMS, ids=["store_f16", "resid_f32", "resid_f32_producer", "swiglu_f16"])
def test_fp8_kernel_equals_the_fp16_kernel_on_the_dequantised_matrix(eng, epi, producer, consumer):
    eps = eng.gemm_info["eps"]
    for si, (N0, K) in enumerate(SHAPES):
        N = N0 if epi != R.EPI_SWIGLU_F16 else {96: 128, 70: 64, 64: 64, 160: 192}[N0]      # gated: N % 64
        N = N if N % 4 == 0 else N + 2                                                       # 70 -> 72: 4-column pieces
        for M in M_ALL:
            rs = np.random.RandomState(1000 * si + 10 * M + epi)
            what = f"epi {epi} producer {producer} consumer {consumer} M={M} N={N} K={K}"
            a = rs.standard_normal((M, K)).astype(np.float16)
            w = _weights(rs, N, K)
            _, _, deq = eng.debug_quant_fp8(w)
            np.testing.assert_array_equal(deq.view(np.uint16), F.quantize(w)[2].view(np.uint16), err_msg=what)
            gated = epi == R.EPI_SWIGLU_F16
            width = N // 2 if gated else N
            dt = np.float32 if epi == R.EPI_RESID_F32 else np.float16
            c_old = rs.standard_normal((M, N)).astype(np.float32) if epi == R.EPI_RESID_F32 else None
            c_in = c_old.reshape(-1) if c_old is not None else None
            kw, factor, frel = {}, None, 0.0
            if consumer == "rowscale":
                kw["rowscale"] = rs.uniform(0.5, 2.0, size=M).astype(np.float32)
                factor = R.consumer_factor(K, eps, rowscale=kw["rowscale"])
            elif consumer:
                nb_in = int(consumer[3:])
                kw["ssq_in"] = (rs.uniform(0.5, 2.0, size=(M, nb_in)) * K * 256.0 / nb_in).astype(np.float32)
                factor, frel = R.consumer_factor(K, eps, ssq_in=kw["ssq_in"]), R.factor_rel_error(nb_in)
            call = dict(c_in=c_in, producer=producer, **kw)
            got = eng.debug_gemm_fp8(epi, a, w, M, N, K, **call)
            ref = eng.debug_gemm_ex(epi, R.STREAM, a, deq, M, N, K, **call)
            assert got["family"] == ref["family"] == R.STREAM and got["nb"] == ref["nb"], what
            # a. every byte: interior, both guard bands, xraw_out, ssq_out
            for key in ("C", "xraw", "ssq"):
                if ref.get(key) is not None:
                    assert got[key].tobytes() == ref[key].tobytes(), f"{what}: {key} of the FP8 kernel differs from the fp16 kernel on the dequantised matrix"
            band = got["band"]
            assert (got["C"][:band].view(np.uint8) == R.SENTINEL).all() and (got["C"][band + M * width:].view(np.uint8) == R.SENTINEL).all(), f"{what}: a guard band was written"
            # b. within the rules of _gemm_ref against fp64 on the dequantised weights
            out = got["C"][band:band + M * width].reshape(M, width)
            t = R.tau(a, deq)
            e = R.expected(epi, a, deq, c_in=c_old, factor=factor)
            mag = None if factor is None else np.abs(R.acc64(a, deq) * factor[:, None])
            if epi == R.EPI_RESID_F32:
                R.check_f32(out, e["out"], t, what, factor=factor, frel=frel, mag=mag)
            else:
                gmag = None if mag is None or not gated else 2.0 * e["lip"] * np.maximum(*[np.abs(x) for x in R.deinterleave_gate_up(mag, axis=1)])
                R.check_f16(out, e["out"], t, what, lip=e["lip"], factor=factor, frel=frel, mag=gmag if gated else mag)


def test_fp8_debug_entry_refuses_what_the_kernel_does_not_take(eng):
    """another family, an epilogue the FP8 kernel has no instantiation of, K % 16: an error, nothing launched.  N = 70 (the
    quantiser test's row count) is outside the stream family's contract - its epilogues store 4-column pieces, N % 4 - on FP8
    bytes as on fp16: RK_ERR_STATE from both entries, which is why the kernel test above runs (72, 400)."""
    from llmrankers._engine import RkError
    a70, w70 = np.zeros((5, 400), np.float16), np.zeros((70, 400), np.float16)
    for entry in ("rk_debug_gemm_fp8", "rk_debug_gemm_ex"):
        with pytest.raises(RkError) as ei:
            eng.debug_gemm_ex(R.EPI_STORE_F16, R.STREAM, a70, w70, 5, 70, 400, entry=entry)
        assert ei.value.code == -4 and "4-column" in str(ei.value), (entry, ei.value)
    a, w = np.zeros((2, 64), np.float16), np.zeros((64, 64), np.float16)
    for epi, fam, K in ((R.EPI_STORE_F16, R.TILED, 64), (R.EPI_STORE_F32, R.STREAM, 64), (R.EPI_RELU_F16, R.STREAM, 64), (R.EPI_STORE_F16, R.STREAM, 40)):
        with pytest.raises(RkError):
            eng.debug_gemm_ex(epi, fam, a[:, :K], w[:, :K], 2, 64, K, entry="rk_debug_gemm_fp8")


# ---- 3. the model, three ways ------------------------------------------------------------------------------------------------------
PROMPT_LENS = (3, 17, 64, 65, 129, 140)
NEW = 24


def _prompts(dims, seed=71):
    return [[int(t) for t in _synth.synth_token_batch(1, n, n, dims.vocab, seed=seed + n)[0]] for n in PROMPT_LENS]


def _all_logits(eng, seqs, vocab):
    return np.concatenate([eng.last_logits(seqs, list(range(v0, v0 + 64))) for v0 in range(0, vocab, 64)], axis=1)


def _run(eng, seqs, dims):
    toks, steps = eng.generate(seqs, NEW, [], PAD)
    assert steps == NEW
    last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), dims.hidden).copy()
    return toks.copy(), last, _all_logits(eng, seqs, dims.vocab)


def test_model_three_ways_bit_for_bit_and_within_the_oracle_bound():
    """TOY_LLAMA with every norm weight 1 (the fold W[n][k] * ln[k] is then the identity, exactly: x * 1.0f).  FP8 engine on the
    bytes, the same engine on the fp16 kernel, a plain fp16 engine loaded with the reference's dequantised state dict: the same
    tokens, the same final rows of the last step, the same prefill logits, bit for bit.  The prefill and the step's logits against the
    fp32 oracle on the dequantised weights: the Llama tests' bound.  (hidden 256 / intermediate 512: the model's projections run the
    kernel's tail loop; its main loop is test 2's.)"""
    from oracle.llama_numpy import LlamaOracle
    dims = _synth.TOY_LLAMA
    state = _state(dims, 23, True)
    deq_state = _dequantised(state)
    changed = sum(int((np.asarray(state[k]) != np.asarray(deq_state[k])).sum()) for k in state)
    assert changed > 1000, "the quantisation must change the model for this test to mean anything"
    seqs = _prompts(dims)
    e8 = _engine(dims, state, weight_fp8=True)
    t1, l1, p1 = _run(e8, seqs, dims)
    e8.set_option("llama_step_fp8", 0)
    t0, l0, p0 = _run(e8, seqs, dims)
    e8.close()
    e16 = _engine(dims, deq_state)
    t2, l2, p2 = _run(e16, seqs, dims)
    e16.close()
    for name, (t, l, p) in {"the fp16 kernel on the same engine": (t0, l0, p0), "the fp16 engine on the dequantised state": (t2, l2, p2)}.items():
        np.testing.assert_array_equal(t1, t, err_msg=f"tokens: FP8 bytes vs {name}")
        assert l1.tobytes() == l.tobytes(), f"the last step's rows: FP8 bytes vs {name}"
        assert p1.tobytes() == p.tobytes(), f"prefill logits: FP8 bytes vs {name}"
    orc = LlamaOracle(dims, deq_state)
    head = np.asarray(deq_state["lm_head.weight" if not dims.tied_head else "model.embed_tokens.weight"], dtype=np.float32)
    want = orc.last_logits(seqs)
    scale, err = float(np.abs(want).max()), float(np.abs(p1 - want).max())
    print(f"prefill: max |logit - oracle| = {err:.3e} at scale {scale:.2f} (bound {BOUND * scale:.3e})")
    assert err < BOUND * scale, (err, scale)
    want = orc.last_logits([s + [int(t) for t in t1[b, :NEW - 1]] for b, s in enumerate(seqs)])
    scale, err = float(np.abs(want).max()), float(np.abs(l1 @ head.T - want).max())
    print(f"step {NEW}: max |logit - oracle| = {err:.3e} at scale {scale:.2f} (bound {BOUND * scale:.3e})")
    assert err < BOUND * scale, (err, scale)
    # and the FP8 model is another model than the fp16 one: the same check against the unquantised oracle must miss
    off = float(np.abs(LlamaOracle(dims, state).last_logits(seqs) - p1).max())
    print(f"against the unquantised oracle: {off:.3e}")
    assert off > BOUND * scale, off


# ---- 4. random norm weights and the other forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy-llama", "toy-qwen2", "toy-qwen3", "toy-llama-hd64"])
def test_fp8_bytes_against_the_fp16_kernel_with_random_norm_weights(name):
    """Folding is no longer the identity: the engine quantises the FOLDED matrices.  Option 1 against option 0 on one engine: the
    same tokens and the same last rows; graph replay (dec_graph 1) against eager launches (0) the same too."""
    dims = _synth.NAMED_DIMS[name]
    state = _state(dims, 31, False)
    seqs = _prompts(dims, seed=5)
    e8 = _engine(dims, state, weight_fp8=True)
    out = {}
    for fp8 in (1, 0):
        for graph in (1, 0):
            e8.set_option("llama_step_fp8", fp8)
            e8.set_option("dec_graph", graph)
            out[fp8, graph] = _run(e8, seqs, dims)
    e8.close()
    for key, (t, l, p) in out.items():
        np.testing.assert_array_equal(out[1, 1][0], t, err_msg=f"{name}: tokens (llama_step_fp8, dec_graph) = (1, 1) vs {key}")
        assert out[1, 1][1].tobytes() == l.tobytes() and out[1, 1][2].tobytes() == p.tobytes(), f"{name}: rows or logits, (1, 1) vs {key}"


# ---- 5. the session ----------------------------------------------------------------------------------------------------------------
def _session(eng, prompts, max_new, n_slots):
    """the requests in order through a session of n_slots (free slots refilled whenever there are any) -> {request: tokens}, refills"""
    got, nxt, refills = {}, 0, 0
    with eng.session(n_slots, 256, 32, [], PAD) as s:
        owner = {}
        while nxt < len(prompts) or s.busy:
            free = s.free_slots()
            take = list(range(nxt, min(nxt + len(free), len(prompts))))
            if take:
                refills += bool(s.busy)
                slots = free[:len(take)]
                s.admit([prompts[r] for r in take], slots, [max_new[r] for r in take])
                owner.update(zip(slots, take))
                nxt += len(take)
            finished, _ = s.run()
            assert finished
            for slot in finished:
                got[owner.pop(slot)] = [int(t) for t in s.read(slot)]
    return got, refills


def test_session_on_fp8_bytes_equals_the_fp16_kernel_and_generate():
    """four slots, seven requests of different lengths and budgets: staggered admits into re-used slots while the others decode"""
    dims = _synth.TOY_LLAMA
    state = _state(dims, 47, False)
    prompts = [[int(t) for t in _synth.synth_token_batch(1, n, n, dims.vocab, seed=200 + n)[0]] for n in (4, 33, 70, 129, 9, 64, 17)]
    max_new = [5, 12, 18, 8, 9, 4, 6]              # the first four finish one by one: three refills beside decoding slots
    e8 = _engine(dims, state, weight_fp8=True)
    got1, refills = _session(e8, prompts, max_new, 4)
    assert refills >= 2, "no slot was re-used while others were decoding"
    alone = {r: [int(t) for t in e8.generate([p], max_new[r], [], PAD)[0][0]] for r, p in enumerate(prompts)}
    e8.set_option("llama_step_fp8", 0)
    got0, _ = _session(e8, prompts, max_new, 4)
    e8.close()
    assert got1 == got0, "session: FP8 bytes vs the fp16 kernel"
    assert got1 == alone, "session vs generate per prompt"


# ---- 6. the contract ---------------------------------------------------------------------------------------------------------------
def test_set_weight_fp8_is_refused_on_t5_and_after_finalize(eng):
    from llmrankers._engine import RkEngine, RkError
    dims = _synth.TOY_GATED_UNTIED
    t5 = RkEngine(dims, device=0, max_tokens=512, max_seqs=4, max_dec_len=2)
    try:
        assert t5.lib.rk_llama_set_weight_fp8(t5.h, 1) == -4             # RK_ERR_STATE
        assert b"Llama" in t5.lib.rk_last_error(t5.h)
    finally:
        t5.close()
    assert eng.lib.rk_llama_set_weight_fp8(eng.h, 0) == -4               # finalized
    assert b"finalize" in eng.lib.rk_last_error(eng.h)
    with pytest.raises(RkError):
        eng.set_option("llama_step_fp8", 2)


def test_step_option_changes_nothing_on_a_plain_engine():
    dims = _synth.TOY_LLAMA
    state = _state(dims, 23, False)
    seqs = _prompts(dims)
    e = _engine(dims, state)
    a = _run(e, seqs, dims)
    e.set_option("llama_step_fp8", 0)
    b = _run(e, seqs, dims)
    e.close()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
