"""CPU-only: the fp64 GEMM reference (tests/_gemm_ref.py) agrees with the oracles, and its two tiers REJECT numpy emulations of
subtly wrong kernels while accepting an honest fp32 blocked sum - the proof that tests/test_gpu_gemm_epilogues.py would notice."""
import numpy as np
import pytest

import _gemm_ref as R
from llmrankers import _synth


def _fp16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def test_reference_ffn_pieces_agree_with_the_t5_oracle():
    from oracle.t5_numpy import T5Oracle, gelu_new
    for dims in (_synth.TOY_GATED_UNTIED, _synth.TOY_RELU_TIED):
        state = _synth.synth_state_dict(dims, seed=5)
        o = T5Oracle(dims, state)
        p = "encoder.block.0.layer.1.DenseReluDense"
        x = _fp16(np.random.RandomState(3).standard_normal((37, dims.d_model)))
        if dims.gated:
            w = R.interleave_gate_up(_fp16(state[p + ".wi_0.weight"]), _fp16(state[p + ".wi_1.weight"]))
            h = R.expected(R.EPI_GEGLU_F16, x, w)["out"]
            np.testing.assert_allclose(R.gelu_new(np.linspace(-6, 6, 101)), gelu_new(np.linspace(-6, 6, 101).astype(np.float32)), rtol=2e-6, atol=1e-6)   # (the fp32 oracle cancels in 1 + tanh)
        else:
            h = R.expected(R.EPI_RELU_F16, x, _fp16(state[p + ".wi.weight"]))["out"]
        got = h @ _fp16(state[p + ".wo.weight"]).astype(np.float64).T
        want = o._ffn(x.astype(np.float32), p)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * float(np.abs(want).max()))


def test_reference_swiglu_agrees_with_the_llama_oracle():
    from oracle.llama_numpy import LlamaOracle
    dims = _synth.TOY_LLAMA
    state = _synth.synth_state_dict(dims, seed=7)
    o = LlamaOracle(dims, state)
    p = "model.layers.0.mlp"
    x = _fp16(np.random.RandomState(4).standard_normal((29, dims.hidden)))
    w = R.interleave_gate_up(_fp16(state[p + ".gate_proj.weight"]), _fp16(state[p + ".up_proj.weight"]))
    got = R.expected(R.EPI_SWIGLU_F16, x, w)["out"]
    g = o._lin(x.astype(np.float32), p + ".gate_proj.weight")              # oracle/llama_numpy.py: hidden_states, the mlp lines
    want = (g / (1.0 + np.exp(-g))) * o._lin(x.astype(np.float32), p + ".up_proj.weight")
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * float(np.abs(want).max()))


def test_interleave_round_trips_and_groups_by_32():
    rs = np.random.RandomState(0)
    gate, up = rs.standard_normal((96, 8)), rs.standard_normal((96, 8))
    w = R.interleave_gate_up(gate, up)
    assert w.shape == (192, 8)
    np.testing.assert_array_equal(w[0:32], gate[0:32])
    np.testing.assert_array_equal(w[32:64], up[0:32])
    np.testing.assert_array_equal(w[64:96], gate[32:64])
    g2, u2 = R.deinterleave_gate_up(w)
    np.testing.assert_array_equal(g2, gate)
    np.testing.assert_array_equal(u2, up)
    g3, u3 = R.deinterleave_gate_up(w.T, axis=1)
    np.testing.assert_array_equal(g3, gate.T)
    np.testing.assert_array_equal(u3, up.T)


def test_gradients_of_the_gate_functions():
    x = np.linspace(-8, 8, 401)
    h = 1e-6
    np.testing.assert_allclose(R.gelu_new_grad(x), (R.gelu_new(x + h) - R.gelu_new(x - h)) / (2 * h), atol=1e-6)
    np.testing.assert_allclose(R.silu_grad(x), (R.silu(x + h) - R.silu(x - h)) / (2 * h), atol=1e-6)


def test_f16_sat_rounds_to_nearest_even_and_saturates():
    got = R.f16_sat(np.array([2049.0, 2051.0, 4098.0, 70000.0, -1e9, 65519.0, 65520.0]))
    np.testing.assert_array_equal(got.astype(np.float64), [2048.0, 2052.0, 4096.0, 65504.0, -65504.0, 65504.0, 65504.0])


# ---- tier A: exact ------------------------------------------------------------------------------------------------------------
def _tier_a_problem():
    rs = np.random.RandomState(11)
    return R.int_operands_big(rs, 70, 132, 1024)          # sums up to 16 384: above 2048, fp16 roundings bite


def test_tier_a_is_order_independent_and_catches_the_mutants():
    a, w = _tier_a_problem()
    want = R.acc64(a, w)
    assert np.abs(want).max() > 2048 and np.abs(want).max() < 2 ** 24
    honest = R.blocked_sum_f32(a, w)
    np.testing.assert_array_equal(honest.astype(np.float64), want)                 # any fp32 order is exact
    np.testing.assert_array_equal(np.cumsum((a[:1].astype(np.float32) * w.astype(np.float32)), axis=1, dtype=np.float32)[:, -1], want[0])
    # fp16 outputs: the honest kernel rounds once
    np.testing.assert_array_equal(honest.astype(np.float16), R.f16_sat(want))
    # mutant: accumulator rounded to fp16 every 64 k
    assert (R.blocked_sum_f32(a, w, round_acc_f16=True).astype(np.float64) != want).any()
    # mutant: fp16 rounding before an fp32 store
    assert (honest.astype(np.float16).astype(np.float64) != want).any()
    # mutant: inf instead of saturation (rows scaled by a power of two)
    scaled = want * 8.0
    assert np.abs(scaled).max() > R.F16_MAX
    with np.errstate(over="ignore"):
        inf_mutant = scaled.astype(np.float32).astype(np.float16)
    assert np.isinf(inf_mutant).any() and not np.isinf(R.f16_sat(scaled)).any()
    assert (inf_mutant != R.f16_sat(scaled)).any()


def test_tier_a_argmax_ties_first_index_and_partial_block():
    rs = np.random.RandomState(12)
    a, w = R.int_operands(rs, 9, 100, 64)                # 100 columns: the last block holds 4
    w[40] = w[35]                                        # an exact tie inside block 1
    w[70] = w[35]                                        # ... and across blocks
    w[99] = w[97]                                        # ... and in the partial last block
    e = R.expected(R.EPI_ARGMAX_F32, a, w)
    acc = R.acc64(a, w)
    assert e["idx"].shape == (9, 4) and (e["idx"][:, 3] >= 96).all()
    assert (acc[:, 40] == acc[:, 35]).all()
    # last-index mutant differs wherever a block's maximum is tied
    pad = np.full((9, 128), -np.inf)
    pad[:, :100] = acc
    blk = pad.reshape(9, 4, 32)
    last = 31 - blk[:, :, ::-1].argmax(axis=2) + 32 * np.arange(4)[None, :]
    assert (last != e["idx"]).any(), "the planted ties never reach a block maximum: the case proves nothing"
    np.testing.assert_array_equal(np.take_along_axis(pad, e["idx"], axis=1), e["max"])


def test_ssq_partial_last_block_mutant_is_rejected():
    rs = np.random.RandomState(13)
    c = rs.randint(-50, 51, size=(5, 100)).astype(np.float64)          # 100 = 64 + 36: the last 64-block is partial
    _, ssq = R.producer_expected(c, 64)
    R.check_ssq(ssq.astype(np.float32), c, 64, "honest")
    clamped = np.concatenate([c, np.repeat(c[:, -1:], 28, axis=1)], axis=1)    # mutant: clamped columns summed too
    mutant = (clamped ** 2).reshape(5, 2, 64).sum(axis=2)
    with pytest.raises(AssertionError):
        R.check_ssq(mutant.astype(np.float32), c, 64, "mutant")
    assert (mutant != ssq).any()


# ---- tier B: random -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [64, 1024, 2816])
@pytest.mark.parametrize("outliers", [False, True])
def test_tier_b_accepts_the_honest_sum_and_rejects_the_mutants(k, outliers):
    rs = np.random.RandomState(k + outliers)
    a, w = R.normal_operands(rs, 24, 160, k, outliers)
    want = R.acc64(a, w)
    t = R.tau(a, w)
    honest = R.blocked_sum_f32(a, w)
    err = R.check_f32(honest, want, t, "honest fp32")
    assert err <= t
    R.check_f16(honest.astype(np.float16), want, t, "honest fp16")
    # tau is far below the tolerance these tests replace, and below an fp16 half-ulp at the typical magnitude
    if not outliers:
        assert t < 2e-3 * np.sqrt(k) / 20
        assert t < R.U16 * np.sqrt(k)
    if k >= 1024:
        with pytest.raises(AssertionError):
            R.check_f32(R.blocked_sum_f32(a, w, round_acc_f16=True), want, t, "fp16 accumulator")
        with pytest.raises(AssertionError):
            R.check_f16(R.blocked_sum_f32(a, w, round_acc_f16=True).astype(np.float16), want, t, "fp16 accumulator, fp16 out")
    with pytest.raises(AssertionError):
        R.check_f32(honest.astype(np.float16).astype(np.float32), want, t, "fp16 rounding before an fp32 store")


def test_tier_b_saturation_and_inf_mutant():
    rs = np.random.RandomState(21)
    a, w = R.normal_operands(rs, 8, 64, 1024, outliers=True)
    factor = np.full(8, 512.0)
    want = R.acc64(a, w) * 512.0
    assert (np.abs(want) > R.F16_MAX * 1.01).any()
    t = R.tau(a, w)
    honest = (R.blocked_sum_f32(a, w) * np.float32(512.0))
    R.check_f16(np.clip(honest, -R.F16_MAX, R.F16_MAX).astype(np.float16), want, t, "saturating", factor=factor)
    with np.errstate(over="ignore"):
        inf_mutant = honest.astype(np.float16)
    with pytest.raises(AssertionError):
        R.check_f16(inf_mutant, want, t, "inf mutant", factor=factor)


def test_gated_tolerance_follows_the_lipschitz_factor():
    rs = np.random.RandomState(22)
    a, w = R.normal_operands(rs, 16, 128, 1024)
    for epi in R.GATED:
        e = R.expected(epi, a, w)
        t = R.tau(a, w)
        acc32 = R.blocked_sum_f32(a, w).astype(np.float64)
        g, u = R.deinterleave_gate_up(acc32, axis=1)
        act = R.gelu_new if epi == R.EPI_GEGLU_F16 else R.silu
        R.check_f16(R.f16_sat(act(g) * u), e["out"], t, R.EPI_NAMES[epi], lip=e["lip"])
        gm, um = R.deinterleave_gate_up(R.blocked_sum_f32(a, w, round_acc_f16=True).astype(np.float64), axis=1)
        with pytest.raises(AssertionError):
            R.check_f16(R.f16_sat(act(gm) * um), e["out"], t, "mutant", lip=e["lip"])


def test_lse_reference_blocks_merge_to_logsumexp():
    rs = np.random.RandomState(23)
    a, w = R.normal_operands(rs, 6, 100, 128)
    lab = rs.randint(0, 100, size=6)
    e = R.expected(R.EPI_LSE_F32, a, w, labels=lab)
    acc = R.acc64(a, w)
    m = e["max"].max(axis=1)
    lse = m + np.log((e["sumexp"] * np.exp(e["max"] - m[:, None])).sum(axis=1))
    np.testing.assert_allclose(lse, np.log(np.exp(acc).sum(axis=1)), rtol=1e-12)
    np.testing.assert_array_equal(e["xlab"], acc[np.arange(6), lab])


# ---- the contract ---------------------------------------------------------------------------------------------------------------
def test_contract_mirror_refuses_the_listed_calls_and_admits_the_engine_sites():
    """tests/_gemm_ref.py mirrors gemm_contract (csrc/rk_engine.hip); the GPU suite asserts that the two agree call by call.  Here:
    every listed call is refused, and the call shapes of the engine's own sites (flan-t5-large dims) pass."""
    for fam, epi, m, n, k, kw, why in R.REFUSED:
        assert R.contract_violation(fam, epi, m, n, k, **kw), (fam, epi, m, n, k, kw, why)
    dm, inner, ff, heads, t = 1024, 1024, 2816, 16, 5888
    sites = [
        (R.TILED, R.EPI_STORE_F16, t, 3 * inner, dm, dict(consumer="rowscale")),
        (R.TILED, R.EPI_RESID_F32, t, dm, inner, dict(producer=True)),
        (R.TILED, R.EPI_GEGLU_F16, t, 2 * ff, dm, dict(consumer="ssq_in")),
        (R.TILED, R.EPI_RESID_F32, t, dm, ff, dict(producer=True)),
        (R.TILED, R.EPI_STORE_F16, t, 24 * 2 * inner, dm, dict(n_split=2 * inner, split_stride=8192 * 2 * inner, ldc=2 * inner)),
        (R.STREAM, R.EPI_STORE_F16, 40, dm, 64, dict(lda=inner, ldw=64, ldc=heads * dm, batch=heads, bsA=64, bsW=dm * 64, bsC=dm)),
        (R.STREAM, R.EPI_STORE_F16, 40, 64, dm, dict(lda=heads * dm, ldw=dm, ldc=inner, batch=heads, bsA=dm, bsW=64 * dm, bsC=64)),
        (R.STREAM, R.EPI_RESID_F32, 100, dm, dm, dict(consumer="ssq_in", producer=True)),
        (R.STREAM, R.EPI_ARGMAX_F32, 13, 32128, dm, dict()),
        (R.TILED, R.EPI_LSE_F32, 640, 32128, dm, dict()),
        (R.GEMV, R.EPI_GEGLU_F16, 3, 2 * ff, dm, dict(consumer="ssq_in")),
        (R.GEMV, R.EPI_RESID_F32, 2, dm, ff, dict(producer=True)),
    ]
    for fam, epi, m, n, k, kw in sites:
        assert R.contract_violation(fam, epi, m, n, k, **kw) is None, (fam, epi, m, n, k, kw)
    # N = 8 j + 4: fp32 outputs are 4-column pieces (admitted), tiled fp16 outputs 8-column pieces (refused), the other families' fp16 4
    assert R.contract_violation(R.TILED, R.EPI_STORE_F32, 33, 260, 64) is None
    assert R.contract_violation(R.TILED, R.EPI_RESID_F32, 33, 260, 64, producer=True) is None
    assert R.contract_violation(R.TILED, R.EPI_STORE_F16, 33, 260, 64)
    assert R.contract_violation(R.STREAM, R.EPI_STORE_F16, 33, 260, 64) is None
    assert R.contract_violation(R.GEMV, R.EPI_STORE_F16, 3, 261, 64) is None
