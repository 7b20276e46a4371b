"""GPU parity tests (run with -m gpu on an MI355X): HIP kernels + C ABI vs the oracle and the HF goldens.

Tolerances: the engine computes with fp16 MFMA inputs / fp32 accumulation / fp32 residual stream, the oracle in
fp32.  north_star: logit scores within 1e-3 (fp16 tolerance) for pointwise -> asserted on the yes/no
probability; raw logits of magnitude ~10 are allowed LOGIT_TOL."""
import json
import os

import numpy as np
import pytest

import _gemm_ref
from conftest import GOLD, load_state

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-3
LOGIT_TOL = 2e-2
DEC_GEMV_ROWS_DEFAULT = 4      # engine default of option dec_gemv_rows (csrc/rk_engine.hip, Options): restored by the tests that widen it


def _engine(dims, state, **kw):
    from llmrankers._engine import RkEngine
    kw.setdefault("max_tokens", 4096)
    kw.setdefault("max_seqs", 64)
    kw.setdefault("max_dec_len", 40)
    return RkEngine(dims, device=0, **kw).load_state(state.items())


def _gemm_close(got, a, w, what=""):
    """fp32 GEMM output against fp64 A W^T within tau = 4 E32 + one fp32 rounding (tests/_gemm_ref.py: E32 = the error of a
    k-ordered fp32 chain of the exact products on a sample of this very problem) - about 1 / 100 of the 2e-3 sqrt(K) these tests
    allowed before, which a kernel rounding its accumulator to fp16 would have passed.  Returns |got - fp64|."""
    want = _gemm_ref.acc64(a, w)
    _gemm_ref.check_f32(got, want, _gemm_ref.tau(a, w), what)
    return np.abs(got - want)


def _sigm(d):
    return 1.0 / (1.0 + np.exp(-d))


@pytest.fixture(scope="module")
def toy(ckpt_dirs):
    out = {}
    for name in ("ckpt_gated_untied", "ckpt_relu_tied"):
        dims, state = load_state(ckpt_dirs[name])
        out[name] = (dims, state, _engine(dims, state))
    yield out
    for _, _, e in out.values():
        e.close()


# variant: 1 = 128x128 tile kernel (glds / register staging), 2..4 = 256x{256,192,128} kernels, 5 = 256x256 ping-pong
# (falls back to variant 2 for a single K tile), 6 = 64x64 small-M kernel
@pytest.mark.parametrize("variant,glds", [(1, True), (1, False), (2, True), (3, True), (4, True), (5, True), (6, True)])
@pytest.mark.parametrize("shape", [(128, 128, 64), (200, 192, 128), (70, 576, 192), (1, 4, 64), (333, 260, 1024),
                                    (5888, 1024, 2816), (777, 516, 384), (256, 256, 128)])
def test_gemm_vs_numpy(toy, shape, variant, glds):
    """C = A W^T with fp16 inputs, fp32 accumulate: exact products, only summation order differs."""
    m, n, k = shape
    if variant == 1 and k % 64:
        pytest.skip("128x128 kernel steps K by 64")
    rs = np.random.RandomState(m + n + k)
    a = rs.standard_normal((m, k)).astype(np.float16)
    w = rs.standard_normal((n, k)).astype(np.float16)
    eng = toy["ckpt_gated_untied"][2]
    eng.set_option("gemm_variant", variant)
    try:
        got = eng.debug_gemm(a, w, use_glds=glds)
    finally:
        eng.set_option("gemm_variant", 0)
    if variant in (5, 6):                                # every tile shape / schedule sums K in the same order
        eng.set_option("gemm_variant", 2)
        try:
            np.testing.assert_array_equal(got, eng.debug_gemm(a, w, use_glds=True))
        finally:
            eng.set_option("gemm_variant", 0)
    _gemm_close(got, a, w, f"shape {shape} variant {variant} glds {glds}")


def test_pingpong_gemm_random_shapes_bit_equal_to_lockstep_kernel(toy):
    """The persistent ping-pong kernel keeps DMA loads in flight across barriers and tiles (counted vmcnt, staging
    beside DMA targets): a schedule bug would show up as a mismatch that comes and goes, so many shapes, each run
    three times, against the lock-step 256x256 kernel (bit-equal) and numpy."""
    eng = toy["ckpt_gated_untied"][2]
    rs = np.random.RandomState(20260926)
    shapes = [(int(rs.randint(1, 1400)), int(rs.randint(1, 300)) * 4, int(rs.randint(2, 24)) * 64) for _ in range(20)]
    shapes += [(2048, 1024, 1024), (513, 768, 128), (3000, 256, 2816)]
    for m, n, k in shapes:
        a = rs.standard_normal((m, k)).astype(np.float16)
        w = rs.standard_normal((n, k)).astype(np.float16)
        try:
            eng.set_option("gemm_variant", 2)
            ref = eng.debug_gemm(a, w, use_glds=True)
            eng.set_option("gemm_variant", 5)
            for _ in range(3):
                np.testing.assert_array_equal(eng.debug_gemm(a, w, use_glds=True), ref, err_msg=f"shape {(m, n, k)}")
        finally:
            eng.set_option("gemm_variant", 0)
        _gemm_close(ref, a, w, f"shape {(m, n, k)}")


def test_k_split_pingpong_gemm_vs_numpy_unsplit_kernel_and_deterministic(toy):
    """gemm_pp2_kernel<.., SPLIT> (round 6): two workgroups share an output tile, each sums a contiguous K range, the first
    arriver's fp32 partial tile travels as a write-through slab and the LAST arriver adds it to its registers.  Option gemm_sk = 2
    forces the split wherever every half keeps two K tiles (the default, gemm_sk = 1, never splits: a split chosen from a launch's
    tile count would make a row's bits depend on its batch).  (1) vs numpy at the fp16-input tolerance; (2) vs the unsplit kernel: equal to
    fp32 re-association noise; (3) each shape three times: bit-identical runs (fixed combine order, tickets reset by the last
    arriver), also right after another shape used the same slabs; (4) K too short for the split: the unsplit bits."""
    eng = toy["ckpt_gated_untied"][2]
    rs = np.random.RandomState(20261001)
    shapes = [(int(rs.randint(1, 1600)), int(rs.randint(1, 300)) * 4, int(rs.randint(4, 60)) * 64) for _ in range(10)]
    shapes += [(1536, 1024, 4096), (1450, 1024, 2816), (700, 516, 14336), (256, 256, 256), (257, 260, 512), (3000, 1024, 1024), (100, 64, 128)]
    for m, n, k in shapes:
        a = rs.standard_normal((m, k)).astype(np.float16)
        w = rs.standard_normal((n, k)).astype(np.float16)
        try:
            eng.set_option("gemm_variant", 5)
            eng.set_option("gemm_sk", 0)
            ref = eng.debug_gemm(a, w, use_glds=True)
            for splits in (2,):
                eng.set_option("gemm_sk", splits)
                first = eng.debug_gemm(a, w, use_glds=True)
                for _ in range(2):
                    np.testing.assert_array_equal(eng.debug_gemm(a, w, use_glds=True), first, err_msg=f"shape {(m, n, k)} x{splits}: not deterministic")
                tiles = -(-m // 256) * -(-n // 256)
                if (k // 64) // splits < 2 or tiles * splits > 256:
                    np.testing.assert_array_equal(first, ref, err_msg=f"shape {(m, n, k)} x{splits}: must not be split")
                _gemm_close(first, a, w, f"shape {(m, n, k)} x{splits}")
                assert np.abs(first - ref).max() < 1e-5 * np.sqrt(k) * max(1.0, float(np.abs(ref).max())), (m, n, k, splits, np.abs(first - ref).max())
        finally:
            eng.set_option("gemm_variant", 0)
            eng.set_option("gemm_sk", 1)


def test_small_tile_gemm_stage_counts_bit_equal_to_lockstep_kernel(toy):
    """The 64x64 kernel keeps 1 - 3 K tiles of DMA in flight with counted vmcnt (2 / 3 / 4 LDS stages): every stage count,
    K from one tile (shorter than the pipeline) to 44 tiles, each run three times, bit-equal to the lock-step kernel."""
    eng = toy["ckpt_gated_untied"][2]
    rs = np.random.RandomState(20260927)
    shapes = [(int(rs.randint(1, 1500)), int(rs.randint(1, 300)) * 4, int(rs.randint(1, 24)) * 64) for _ in range(12)]
    shapes += [(1450, 1024, 1024), (1450, 1024, 2816), (64, 64, 64), (65, 68, 128), (130, 64, 192), (2900, 1024, 256)]
    for m, n, k in shapes:
        a = rs.standard_normal((m, k)).astype(np.float16)
        w = rs.standard_normal((n, k)).astype(np.float16)
        try:
            eng.set_option("gemm_variant", 2)
            ref = eng.debug_gemm(a, w, use_glds=True)
            eng.set_option("gemm_variant", 6)
            for nst in (0, 2, 3, 4):
                eng.set_option("gemm_s64_stages", nst)
                for _ in range(3):
                    np.testing.assert_array_equal(eng.debug_gemm(a, w, use_glds=True), ref, err_msg=f"shape {(m, n, k)} stages {nst}")
        finally:
            eng.set_option("gemm_variant", 0)
            eng.set_option("gemm_s64_stages", 0)
        _gemm_close(ref, a, w, f"shape {(m, n, k)}")


@pytest.mark.parametrize("shape", [(1, 64, 64), (32, 128, 1024), (33, 96, 192), (100, 1024, 2816), (256, 1024, 1024), (200, 96, 2816)])
def test_weight_streaming_gemm_vs_numpy(toy, shape):
    """The decoder's split-K kernel: fixed reduction tree -> every row is independent of how many rows share the launch."""
    m, n, k = shape
    rs = np.random.RandomState(m * n + k)
    a = rs.standard_normal((m, k)).astype(np.float16)
    w = rs.standard_normal((n, k)).astype(np.float16)
    eng = toy["ckpt_gated_untied"][2]
    got = eng.debug_gemm(a, w, use_glds=2)
    _gemm_close(got, a, w, f"shape {shape}")
    np.testing.assert_array_equal(eng.debug_gemm(a[m - 1:], w, use_glds=2)[0], got[m - 1])
    for lo, hi in ((0, 32), (m // 3, m // 3 + 40), (m // 2, m)):          # any sub-batch (other slab grouping): same bits
        if hi <= m and hi - lo >= 1:
            np.testing.assert_array_equal(eng.debug_gemm(a[lo:hi], w, use_glds=2), got[lo:hi])


@pytest.mark.parametrize("shape", [(1, 64, 64), (2, 1024, 1024), (2, 3072, 1024), (2, 1024, 2816), (13, 1024, 1024), (13, 1024, 2816), (16, 516, 1024),
                                    (7, 36, 3072), (5, 2052, 576), (9, 8, 64)])
def test_few_row_gemv_vs_numpy(toy, shape):
    """gemv_rows_kernel (round 6: the decoder projections of ONE setwise compare, M <= 16 rows): one wave per output column, lanes
    split K, v_dot2 with fp32 accumulation, fixed xor tree - exact products, another summation order than the MFMA kernels: against
    numpy at the fp16-input tolerance and against the weight-streaming kernel to fp32 re-association noise; three runs bit-identical."""
    m, n, k = shape
    rs = np.random.RandomState(m * 7 + n + k)
    a = rs.standard_normal((m, k)).astype(np.float16)
    w = rs.standard_normal((n, k)).astype(np.float16)
    eng = toy["ckpt_gated_untied"][2]
    got = eng.debug_gemm(a, w, use_glds=3)
    for _ in range(2):
        np.testing.assert_array_equal(eng.debug_gemm(a, w, use_glds=3), got)
    _gemm_close(got, a, w, f"shape {shape}")
    ws = eng.debug_gemm(a, w, use_glds=2)
    assert np.abs(got - ws).max() < 1e-5 * np.sqrt(k) * max(1.0, float(np.abs(ws).max()))


def test_few_row_decoder_family_vs_weight_streaming_family_and_oracle(toy):
    """The decoder pass of one setwise prompt (a handful of rows at >= 2 positions; option dec_gemv_rows, default 4, here 16 = all the
    kernel takes) on the few-row GEMV family (option dec_gemv = 1, the default) against the weight-streaming family (0) and the fp32 oracle: label logits after a two-token prefix (2 rows), greedy
    continuations (rows grow 2, 3, 4), a three-prompt call (6 rows) and rk_t5_greedy2's tree pass - same tokens, logits within the
    suite's tolerance of the oracle and within fp32-order noise of each other; rows do not depend on what shares the call WITHIN the
    family (one prompt alone == inside the three-prompt call, bit for bit); more than 16 rows take the other family either way."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    for ck in ("ckpt_gated_untied", "ckpt_relu_tied"):
        dims, state, eng = toy[ck]
        orc = T5Oracle(dims, state)
        seqs = _synth.synth_token_batch(3, 20, 120, dims.vocab, seed=61)
        prefix, ids = [0, 17], [11, 12, 13, 14, 15]
        try:
            eng.set_option("dec_gemv_rows", 16)                                      # the whole family (default: up to 4 rows)
            got = eng.score(seqs, prefix, ids)
            np.testing.assert_array_equal(eng.score(seqs[1:2], prefix, ids)[0], got[1])          # batch independence inside the family
            tok = eng.greedy(seqs[:1], [0, 17], 3)[0]
            tok2 = eng.greedy(seqs[:1], [0, 17], 2, candidates=ids)[0]               # the tree pass of rk_t5_greedy2
            eng.set_option("dec_gemv", 0)
            ref = eng.score(seqs, prefix, ids)
            tok_ref = eng.greedy(seqs[:1], [0, 17], 3)[0]
            big = _synth.synth_token_batch(9, 20, 60, dims.vocab, seed=62)                     # 18 rows: the other family either way
            big_ref = eng.score(big, prefix, ids)
            eng.set_option("dec_gemv", 1)
            np.testing.assert_array_equal(eng.score(big, prefix, ids), big_ref)
            eng.set_option("dec_gemv_rows", DEC_GEMV_ROWS_DEFAULT)
            np.testing.assert_array_equal(eng.score(seqs, prefix, ids), ref)         # 6 rows at the default limit: the other family
            np.testing.assert_array_equal(eng.score(seqs[1:2], prefix, ids), eng.score(seqs[1:3], prefix, ids)[:1])   # 2 and 4 rows: this one
        finally:
            eng.set_option("dec_gemv", 1)
            eng.set_option("dec_gemv_rows", DEC_GEMV_ROWS_DEFAULT)
        want = orc.score_last(seqs, prefix, ids)
        assert np.abs(got - want).max() < LOGIT_TOL and np.abs(ref - want).max() < LOGIT_TOL
        assert np.abs(got - ref).max() < 2e-3, np.abs(got - ref).max()
        np.testing.assert_array_equal(tok, tok_ref)
        np.testing.assert_array_equal(tok2, tok[:, :2])                                   # tree pass == two steps (same family)


def test_few_row_decoder_family_wide_attention_inner_dim():
    """A 2-row, 2-position decoder pass of a model whose attention width I = n_heads * d_kv = 3328 exceeds what the GEMV kernel
    takes as K (512 * GEMV_MAX_PIECES = 3072): the O / cross-O projections cannot run on it, so the whole pass must stay on the
    weight-streaming family (one statistics layout for the folded norms) - default options, dec_gemv = 0 and the oracle agree."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims = _synth.T5Dims(vocab=256, d_model=256, n_heads=52, d_kv=64, d_ff=512, n_enc=1, n_dec=2)
    state = _synth.synth_state_dict(dims, seed=71, gain=2.0)
    eng = _engine(dims, state)
    try:
        seqs = _synth.synth_token_batch(1, 20, 120, dims.vocab, seed=72)
        prefix, ids = [0, 17], [11, 12, 13, 14, 15]
        got = eng.score(seqs, prefix, ids)
        eng.set_option("dec_gemv", 0)
        ref = eng.score(seqs, prefix, ids)
    finally:
        eng.close()
    want = T5Oracle(dims, state).score_last(seqs, prefix, ids)
    assert np.abs(got - want).max() < LOGIT_TOL and np.abs(ref - want).max() < LOGIT_TOL, (np.abs(got - want).max(), np.abs(ref - want).max())
    assert np.abs(got - ref).max() < 2e-3, np.abs(got - ref).max()


def test_encoder_stages_one_layer():
    """1-layer model: every intermediate buffer vs the oracle (localises a wrong kernel)."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle, rmsnorm
    dims = _synth.T5Dims(vocab=256, d_model=128, n_heads=3, d_kv=64, d_ff=256, n_enc=1, n_dec=1)
    state = _synth.synth_state_dict(dims, seed=21, gain=2.0)
    eng = _engine(dims, state)
    orc = T5Oracle(dims, state)
    seqs = _synth.synth_token_batch(5, 3, 200, dims.vocab, seed=3) + [np.array([7], dtype=np.int32)]
    eng.score(seqs, [0], [5, 6])
    T = sum(len(s) for s in seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    I, dm = dims.inner, dims.d_model
    qkv = eng.debug_read("qkv", T * 3 * I).reshape(T, 3 * I)
    ctx = eng.debug_read("ctx", T * I).reshape(T, I)
    hid = eng.debug_read("enc_hidden", T * dm).reshape(T, dm)
    enc_out = eng.debug_read("enc_out", T * dm).reshape(T, dm)
    for b, ids in enumerate(seqs):
        orc.capture = {}
        orc.encode(ids)
        h0 = orc.capture["enc.embed"]
        x = rmsnorm(h0, state["encoder.block.0.layer.0.layer_norm.weight"], dims.eps)
        p = "encoder.block.0.layer.0.SelfAttention."
        want_qkv = np.concatenate([x @ state[p + m + ".weight"].T for m in "qkv"], axis=1)
        sl = slice(off[b], off[b + 1])
        np.testing.assert_allclose(qkv[sl], want_qkv, atol=3e-2, rtol=2e-3, err_msg=f"qkv seq {b}")
        L = len(ids)
        q, k, v = (want_qkv[:, i * I:(i + 1) * I].reshape(L, dims.n_heads, 64).transpose(1, 0, 2) for i in range(3))
        s = q @ k.transpose(0, 2, 1) + orc.capture["enc.bias"]
        pr = np.exp(s - s.max(-1, keepdims=True))
        pr /= pr.sum(-1, keepdims=True)
        want_ctx = (pr @ v).transpose(1, 0, 2).reshape(L, I)
        np.testing.assert_allclose(ctx[sl], want_ctx, atol=3e-2, rtol=5e-3, err_msg=f"ctx seq {b} (len {L})")
        np.testing.assert_allclose(hid[sl], orc.capture["enc.0.ffn"], atol=6e-2, rtol=5e-3, err_msg=f"hidden seq {b}")
        np.testing.assert_allclose(enc_out[sl], orc.capture["enc.final"], atol=3e-2, rtol=5e-3, err_msg=f"enc_out seq {b}")
    eng.close()


@pytest.mark.parametrize("name", ["gated_untied", "relu_tied"])
def test_toy_logits_vs_hf_goldens(toy, name):
    dims, state, eng = toy["ckpt_" + name]
    g = np.load(os.path.join(GOLD, f"model_{name}.npz"))
    seqs = [g["input_ids"][b, :n].astype(np.int32) for b, n in enumerate(g["lens"])]
    for tag in ("d1", "d2", "d5"):
        dec = g[f"{tag}.dec_ids"].tolist()
        want = g[f"{tag}.logits"][:, -1, :]
        got = np.concatenate([eng.score(seqs, dec, list(range(c, c + 64))) for c in range(0, dims.vocab, 64)], axis=1)
        err = np.abs(got - want)
        assert err.max() < LOGIT_TOL, f"{tag}: max logit err {err.max():.4f} (mean {err.mean():.5f})"
        # pointwise-style probability between two arbitrary vocabulary rows
        assert np.abs(_sigm(got[:, 10] - got[:, 20]) - _sigm(want[:, 10] - want[:, 20])).max() < SCORE_TOL


@pytest.mark.parametrize("name", ["gated_untied", "relu_tied"])
def test_toy_qlm_and_greedy_vs_hf_goldens(toy, name):
    dims, state, eng = toy["ckpt_" + name]
    g = np.load(os.path.join(GOLD, f"model_{name}.npz"))
    seqs = [g["input_ids"][b, :n].astype(np.int32) for b, n in enumerate(g["lens"])]
    labels = g["qlm.labels"]
    lg = g["qlm.logits"].astype(np.float64)
    m = lg.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(lg - m).sum(-1, keepdims=True)))[..., 0]
    want = -(lse - np.take_along_axis(lg, labels[None, :, None].repeat(len(seqs), 0), -1)[..., 0]).sum(-1)
    got = eng.qlm(seqs, labels.tolist())
    assert np.abs(got - want).max() < 5e-2, (got, want)          # sum of 6 log-probs of magnitude ~5 each
    prefix = g["gen.prefix"].tolist()
    toks, steps = eng.greedy(seqs, prefix, 2)
    gen = g["gen.output_ids"]
    assert steps == gen.shape[1] - len(prefix)
    np.testing.assert_array_equal(toks[:, :steps], gen[:, len(prefix):])
    for b, s in enumerate(json.loads(bytes(g["gen.single_json"]).decode())):   # the reference's B=1 call shape
        t1, st1 = eng.greedy([seqs[b]], prefix, 2)
        assert t1[0, :st1].tolist() == s[len(prefix):]


def test_config1_flan_t5_small_vs_hf_golden():
    """BASELINE.json configs[0]: flan-t5-small shape, pointwise yes_no, hits=20, batch_size=4 — HF CPU logits."""
    from llmrankers import _synth
    g = np.load(os.path.join(GOLD, "config1_flan_t5_small.npz"))
    dims = _synth.FLAN_T5_SMALL
    eng = _engine(dims, _synth.synth_state_dict(dims, seed=int(g["seed"]), threads=8), max_tokens=4096, max_seqs=32, max_dec_len=4)
    off = np.concatenate([[0], np.cumsum(g["lens"])])
    seqs = [g["tokens"][off[i]:off[i + 1]].astype(np.int32) for i in range(len(g["lens"]))]
    ids = g["yes_no_ids"].tolist()
    got = np.concatenate([eng.score(seqs[s:s + 4], [0], ids) for s in range(0, 20, 4)], axis=0)
    want = g["logits"]
    assert np.abs(got - want).max() < LOGIT_TOL, np.abs(got - want).max()
    p_got, p_want = _sigm(got[:, 0] - got[:, 1]), _sigm(want[:, 0] - want[:, 1])
    assert np.abs(p_got - p_want).max() < SCORE_TOL, np.abs(p_got - p_want).max()
    assert np.array_equal(np.argsort(-p_got, kind="stable"), np.argsort(-p_want, kind="stable")) or \
        np.abs(np.sort(p_want)[1:] - np.sort(p_want)[:-1]).min() < 2 * SCORE_TOL
    # one whole call of 20 ragged passages == five calls of 4 (batch composition cannot matter)
    np.testing.assert_array_equal(eng.score(seqs, [0], ids), got)
    eng.close()


def test_pipelined_slots_with_decoder_graphs_match_blocking_calls_at_bench_shape():
    """Stress of the counted-wait kernels under the conditions of the bench pipeline: flan-t5-large dims, one query's hits=100
    x 184 tokens per slot, both slots in flight (the decoder chain of one - replayed as a HIP graph - beside the encoder of
    the other), six launch sequences; every slot's scores must be the bits of a blocking call.  Round 4 found a wait that
    only failed here: the ping-pong GEMM counted its four row-factor loads (plain loads) against the next tile's twelve LDS-DMA
    instructions issued behind them, and the two kinds do not retire in one order - a few rows per launch were scaled by stale
    registers (scores off by up to 0.5) once the compiler's own vmcnt(0) in front of the barrier was gone (asm form of the
    DMA).  The serial tests never saw it; bench.py --mode shard's recomputation check did."""
    from llmrankers import _synth
    dims = _synth.FLAN_T5_LARGE
    state = _synth.synth_state_dict(dims, seed=929, threads=16)
    eng = _engine(dims, state, max_tokens=100 * 256, max_seqs=128, max_dec_len=4)
    qs = [_synth.synth_token_batch(100, 184, 184, dims.vocab, seed=4000 + q) for q in range(2)]
    ids = [2163, 465]
    for opts in ({}, {"dec_fuse": 0}, {"gemm_split": 0}, {"overlap": 0}):
        for k, v in opts.items():
            eng.set_option(k, v)
        for rep in range(2):
            for s_ in range(2):
                eng.stage(qs[s_], slot=s_)
            for it in range(6):
                eng.score_staged([0], ids, slot=it % 2)
            eng.sync()
            staged = [eng.read_scores(s_) for s_ in range(2)]
            for s_ in range(2):
                np.testing.assert_array_equal(eng.score(qs[s_], [0], ids), staged[s_], err_msg=f"{opts} rep {rep} slot {s_}")
        for k in opts:
            eng.set_option(k, 1)
    eng.close()


def test_fused_decoder_projections_match_the_separate_gemms():
    """decoder_kernels.h (round 4): the q projection + W_k^T q, and the chunk merge + W_v projection, each fused per (head,
    row slab) on the matrix cores (engine option dec_fuse, default on) against the five-launch form they replace: same
    rounding points, another fp32 summation order over K (which flips fp16 roundings of q and qk here and there) -> logits
    within 4e-3 of their scale, yes/no probabilities within half the score tolerance, greedy tokens identical; and the fused path against the oracle.
    Shapes: toy (d = 128: partial 256-column pieces, two k16 steps per wave), flan-t5-small dims (6 heads, d = 512) and
    flan-t5-large dims; one and three decoder positions, the tree form of rk_t5_greedy2, ragged rows (1 .. 4 key chunks)."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    for dims, n, lo, hi in ((_synth.TOY_GATED_UNTIED, 37, 3, 250), (_synth.FLAN_T5_SMALL, 40, 20, 184), (_synth.FLAN_T5_LARGE, 70, 60, 184)):
        state = _synth.synth_state_dict(dims, seed=5, gain=1.0, threads=16)
        eng = _engine(dims, state, max_tokens=16384, max_seqs=80, max_dec_len=8)
        seqs = _synth.synth_token_batch(n, lo, hi, dims.vocab, seed=77)
        ids = [21 % dims.vocab, 22 % dims.vocab, 50 % dims.vocab]
        outs = {}
        for fuse in (1, 0):
            eng.set_option("dec_fuse", 2 * fuse)             # 2: the fused form for every decoder length (default 1: one position only)
            outs[fuse] = (eng.score(seqs, [0], ids), eng.score(seqs[:9], [0, 7, 9], ids),
                          eng.greedy(seqs[:5], [0, 7], 2, 1, 0, candidates=ids)[0], eng.greedy(seqs[:5], [0, 7], 2, 1, 0)[0])
        eng.set_option("dec_fuse", 2)
        for a, b in zip(outs[1][:2], outs[0][:2]):
            scale = float(np.abs(b).max())
            assert np.abs(a - b).max() < 4e-3 * max(scale, 1.0), (dims.d_model, np.abs(a - b).max(), scale)
            # two fp16 pipelines with the same rounding POINTS but another fp32 summation order flip ~1 % of the fp16 roundings of q and
            # qk; over 24 layers that is 5e-4 on a probability (measured) - as far as either is from the fp32 oracle.  Parity itself
            # is pinned by the oracle / HF goldens (below and test_flan_t5_large_full_batch_vs_hf_golden)
            assert np.abs(_sigm(a[:, 0] - a[:, 1]) - _sigm(b[:, 0] - b[:, 1])).max() < SCORE_TOL
        np.testing.assert_array_equal(outs[1][2], outs[1][3])            # speculative two-token pass == two steps (fused path)
        # batch independence of the fused path across the rows-per-workgroup choices (70 / 9 / 1 rows pick different slabs)
        np.testing.assert_array_equal(eng.score(seqs[3:4], [0], ids)[0], outs[1][0][3])
        for k in (2, 9, 17, 33):                                         # (slab heights 2 .. 16, column splits 1 .. 8, both merge item shapes)
            np.testing.assert_array_equal(eng.score(seqs[:k], [0], ids), outs[1][0][:k])
        np.testing.assert_array_equal(eng.score(seqs[:4], [0, 7, 9], ids), outs[1][1][:4])
        if dims.d_model <= 512:
            want = T5Oracle(dims, state).score_last(seqs[:6], [0, 7, 9], ids)
            assert np.abs(outs[1][1][:6] - want).max() < LOGIT_TOL, np.abs(outs[1][1][:6] - want).max()
        eng.close()


def test_flan_t5_large_dims_vs_oracle_and_properties():
    """BASELINE.json configs[1] model shape: a few sequences vs the fp32 oracle, then size-independent
    properties on the full B=32 x L=184 batch (batch independence, permutation equivariance)."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims = _synth.FLAN_T5_LARGE
    state = _synth.synth_state_dict(dims, seed=929, threads=16)
    eng = _engine(dims, state, max_tokens=8192, max_seqs=32, max_dec_len=4)
    batch = _synth.synth_token_batch(32, 184, 184, dims.vocab, seed=929)
    ragged = _synth.synth_token_batch(3, 20, 184, dims.vocab, seed=930)
    ids = [2163, 465]
    got_r = eng.score(ragged, [0], ids)
    want_r = T5Oracle(dims, state).score_last(ragged, [0], ids)
    p_got, p_want = _sigm(got_r[:, 0] - got_r[:, 1]), _sigm(want_r[:, 0] - want_r[:, 1])
    assert np.abs(p_got - p_want).max() < SCORE_TOL, (got_r, want_r)
    full = eng.score(batch, [0], ids)
    assert np.isfinite(full).all()
    perm = np.random.RandomState(1).permutation(32)
    np.testing.assert_array_equal(eng.score([batch[i] for i in perm], [0], ids), full[perm])
    np.testing.assert_array_equal(eng.score(batch[5:9], [0], ids), full[5:9])
    eng.set_option("gemm_variant", 1)
    eng.set_option("gemm_glds", 0)
    v1_regs = eng.score(batch, [0], ids)
    eng.set_option("gemm_glds", 1)
    v1_glds = eng.score(batch, [0], ids)
    eng.set_option("gemm_variant", 5)
    v5 = eng.score(batch, [0], ids)
    eng.set_option("gemm_variant", 6)
    v6 = eng.score(batch[:8], [0], ids)
    eng.set_option("gemm_variant", 0)
    np.testing.assert_array_equal(v5, full)              # ping-pong schedule: same arithmetic again
    np.testing.assert_array_equal(v6, full[:8])          # 64x64 small-M tiles: and again
    np.testing.assert_array_equal(v1_regs, v1_glds)      # DMA and register staging run the same arithmetic
    np.testing.assert_array_equal(v1_glds, full)         # ... and so do all tile shapes (same K order per output)
    eng.set_option("attn_short", 0)                      # the tiled kernel instead of the DMA one
    np.testing.assert_array_equal(eng.score(batch, [0], ids), full)
    for mode in (6, 5):                                  # DMA kernel with one / two head groups per workgroup,
        eng.set_option("attn_short", mode)
        for hpw in (1, 2, 16):                           # ... heads per group: same bits
            eng.set_option("attn_heads_per_wg", hpw)
            np.testing.assert_array_equal(eng.score(batch, [0], ids), full)
    eng.set_option("attn_heads_per_wg", 0)
    # cross-attention: query-side form (default for <= 32 decoder rows) vs materialised K/V projections — same math,
    # different rounding points
    eng.set_option("xattn_direct", 0)
    kv_path = eng.score(batch, [0], ids)
    kv_ragged = eng.score(ragged, [0], ids)
    eng.set_option("xattn_direct", 1)
    assert np.abs(_sigm(kv_path[:, 0] - kv_path[:, 1]) - _sigm(full[:, 0] - full[:, 1])).max() < SCORE_TOL
    assert np.abs(_sigm(kv_ragged[:, 0] - kv_ragged[:, 1]) - p_want).max() < SCORE_TOL
    eng.close()


def test_encoder_attention_kernels_bit_identical_on_ragged_batches():
    """The two encoder attention kernels (DMA-staged whole-row default; tiled, which walks the key tiles of a short sequence
    twice) write the same context rows for ragged lengths around the tile edges (1, 64, 65, 128, 129, 191, 192 ...), whatever
    the number of heads a workgroup of the DMA kernel walks, and a short sequence gets the same rows when a longer one in its
    batch sends the whole batch to the tiled kernel (with and without the key split for sequences beyond 512 tokens) - a
    sequence's bits must not depend on the kernel its batch selects."""
    from llmrankers import _synth
    for dims, lens in ((_synth.TOY_GATED_UNTIED, [109, 5, 64, 192, 130, 1, 65, 128, 184, 191, 2, 33, 129]),
                       (_synth.FLAN_T5_SMALL, [184, 20, 77, 192, 65, 129, 96, 1, 184, 127])):
        state = _synth.synth_state_dict(dims, 3, gain=2.0)
        eng = _engine(dims, state, max_tokens=4096, max_seqs=32, max_dec_len=4)
        rs = np.random.RandomState(1)
        seqs = [rs.randint(2, dims.vocab, size=n).tolist() for n in lens]
        T, I = sum(lens), dims.n_heads * dims.d_kv

        def ctx(batch=None, rows=T):
            eng.score(batch or seqs, [0], [3, 4])
            return eng.debug_read("ctx", rows * I).copy()
        eng.set_option("attn_short", 0)
        ref = ctx()
        assert np.isfinite(ref).all()
        for mode in (5, 6):                              # two / one six-wave group(s) per workgroup
            eng.set_option("attn_short", mode)
            for hpw in (0, 1, 2, 3, 16):                 # (3 heads: a group short of heads repeats one without storing)
                eng.set_option("attn_heads_per_wg", hpw)
                np.testing.assert_array_equal(ctx(), ref, err_msg=f"DMA kernel {mode}, heads_per_wg={hpw}")
        eng.set_option("attn_heads_per_wg", 0)
        eng.set_option("attn_short", 5)
        for extra in (300, 700):                         # a longer sequence behind them: tiled kernel / tiled kernel with key split
            longer = seqs + [rs.randint(2, dims.vocab, size=extra).tolist()]
            np.testing.assert_array_equal(ctx(longer, T), ref, err_msg=f"short sequences beside one of {extra} tokens")
        eng.close()


def test_encoder_attention_persistent_walk_on_random_batches():
    """The persistent DMA attention kernel deals (sequence, head) items out in contiguous runs per wave group and prefetches
    across sequence boundaries: random batch shapes (1 .. 40 sequences of 1 .. 192 tokens, 3 and 6 heads, forced and automatic
    run lengths - runs that end inside a sequence, groups without items, a last workgroup short of items) against the tiled
    kernel, bit for bit."""
    from llmrankers import _synth
    rs = np.random.RandomState(7)
    for dims in (_synth.TOY_GATED_UNTIED, _synth.FLAN_T5_SMALL):
        state = _synth.synth_state_dict(dims, 5, gain=2.0)
        eng = _engine(dims, state, max_tokens=8192, max_seqs=48, max_dec_len=4)
        I = dims.n_heads * dims.d_kv
        for trial in range(10):
            n = int(rs.randint(1, 41))
            lens = [int(x) for x in rs.choice([1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 150, 184, 191, 192], size=n)]
            while sum(lens) > 8000:
                lens.pop()
            seqs = [rs.randint(2, dims.vocab, size=m).tolist() for m in lens]
            T = sum(lens)

            def ctx():
                eng.score(seqs, [0], [3, 4])
                return eng.debug_read("ctx", T * I).copy()
            eng.set_option("attn_short", 0)
            ref = ctx()
            for mode, per in ((5, 0), (5, int(rs.randint(1, 8))), (6, 0), (6, int(rs.randint(1, 30)))):
                eng.set_option("attn_short", mode)
                eng.set_option("attn_heads_per_wg", per)
                np.testing.assert_array_equal(ctx(), ref, err_msg=f"trial {trial}: lens={lens} mode={mode} items per group={per}")
            eng.set_option("attn_heads_per_wg", 0)
            eng.set_option("attn_short", 5)
        eng.close()


def test_capacity_and_argument_errors(toy):
    from llmrankers._engine import RkError
    dims, state, eng = toy["ckpt_gated_untied"]
    with pytest.raises(RkError):
        eng.score([[5, 1]] * 100, [0], [3])                 # > max_seqs
    with pytest.raises(RkError):
        eng.score([[5, 999, 1]], [0], [3])                  # token id out of range
    with pytest.raises(RkError):
        eng.score([[5, 1], []], [0], [3])                   # empty sequence
    with pytest.raises(RkError):
        eng.score([[5, 1]], [0] * 100, [3])                 # decoder prefix beyond max_dec_len
    assert np.isfinite(eng.score([[5, 1]], [0], [3])).all()   # engine still usable after errors


def test_setwise_shape_flan_t5_large_vs_oracle():
    """BASELINE.json configs[2] call shape: ONE long prompt (11 passages x ~134 tokens + query + template ~ 1.5k tokens),
    decoder prefix [0, Passage] -> 11 label logits (likelihood) and 2 greedy tokens (generation), flan-t5-large dims."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims = _synth.FLAN_T5_LARGE
    state = _synth.synth_state_dict(dims, seed=929, threads=16)
    eng = _engine(dims, state, max_tokens=4096, max_seqs=8, max_dec_len=8)
    orc = T5Oracle(dims, state)
    seq = _synth.synth_token_batch(1, 1536, 1536, dims.vocab, seed=77)
    prefix = [0, 5454]
    labels = list(range(71, 71 + 11))
    enc = orc.encode(seq[0])
    want = orc.decode(enc, prefix)[-1]
    got = eng.score(seq, prefix, labels)[0]
    err = np.abs(got - want[labels]).max()
    assert err < 3e-2, err                              # logits of magnitude ~3; fp16 activations over 1.5k keys
    top2 = np.sort(want[labels])[-2:]
    if top2[1] - top2[0] > 0.1:                          # decision margin above the noise floor -> same label
        assert int(np.argmax(got)) == int(np.argmax(want[labels]))
    toks, steps = eng.greedy(seq, prefix, 2)
    full_sorted = np.sort(want)
    if full_sorted[-1] - full_sorted[-2] > 0.1:
        assert toks[0, 0] == int(np.argmax(want))
    assert steps in (1, 2)
    # a second, shorter prompt in the same call must not change the first (ragged batch of long prompts)
    two = seq + _synth.synth_token_batch(1, 700, 700, dims.vocab, seed=78)
    np.testing.assert_array_equal(eng.score(two, prefix, labels)[0], got)
    eng.close()


def test_qlm_flan_t5_small_vs_oracle():
    """BASELINE.json configs[3] method (pointwise qlm) at flan-t5-small dims: 33 label positions, full-vocabulary CE;
    more than 32 decoder rows -> exercises the materialised cross-K/V path and the tiled GEMM in the decoder."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims = _synth.FLAN_T5_SMALL
    state = _synth.synth_state_dict(dims, seed=929, threads=8)
    eng = _engine(dims, state, max_tokens=4096, max_seqs=16, max_dec_len=40)
    seqs = _synth.synth_token_batch(6, 40, 150, dims.vocab, seed=31)
    labels = [0] + np.random.RandomState(5).randint(3, dims.vocab, size=32).tolist()
    got = eng.qlm(seqs, labels)
    want = T5Oracle(dims, state).qlm(seqs, labels)
    assert np.abs(got - want).max() < 0.15, (got, want)            # sum of 33 log-probs of magnitude ~10 each
    assert np.abs(got - want).max() / np.abs(want).max() < 5e-4
    np.testing.assert_array_equal(np.argsort(-got), np.argsort(-want))
    eng.close()


def test_folded_rmsnorm_matches_separate_norm_kernels(toy):
    """Default encoder path: the two RMSNorms of a layer are folded into the GEMMs (un-normalised fp16 stream as A,
    norm weight in the GEMM weight, row factor in the epilogue).  It must agree with the separate-kernel path to well
    inside the score tolerance, be as close to the fp32 oracle, and not depend on the GEMM tile shape."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims, state, eng = toy["ckpt_gated_untied"]
    seqs = _synth.synth_token_batch(9, 3, 190, dims.vocab, seed=77)
    ids = [11, 12, 13, 14]
    want = T5Oracle(dims, state).score_last(seqs, [0], ids)
    try:
        eng.set_option("fold_norm", 0)
        plain = eng.score(seqs, [0], ids)
        eng.set_option("fold_norm", 1)
        fold = eng.score(seqs, [0], ids)
        for v in (1, 2, 3, 4, 5, 6):
            eng.set_option("gemm_variant", v)
            np.testing.assert_array_equal(eng.score(seqs, [0], ids), fold, err_msg=f"tile variant {v}")
        # row factors formed by the consumer GEMM's epilogue (fill-in variants) or by rowscale_kernel (ping-pong kernel): same bits
        for v in (0, 1, 6):
            eng.set_option("gemm_variant", v)
            eng.set_option("consumer_stats", 0)
            np.testing.assert_array_equal(eng.score(seqs, [0], ids), fold, err_msg=f"rowscale_kernel in front of variant {v}")
            eng.set_option("consumer_stats", 1)
    finally:
        eng.set_option("gemm_variant", 0)
        eng.set_option("fold_norm", 1)
        eng.set_option("consumer_stats", 1)
    assert np.abs(fold - plain).max() < 5e-3, np.abs(fold - plain).max()
    assert np.abs(fold - want).max() < LOGIT_TOL and np.abs(plain - want).max() < LOGIT_TOL
    assert np.abs(_sigm(fold[:, 0] - fold[:, 1]) - _sigm(want[:, 0] - want[:, 1])).max() < SCORE_TOL
    np.testing.assert_array_equal(eng.score(seqs[2:5], [0], ids), fold[2:5])       # batch independence holds for the folded path


@pytest.mark.parametrize("ckpt", ["ckpt_gated_untied", "ckpt_relu_tied"])
def test_decoder_folded_rmsnorm_matches_separate_norm_kernels(toy, ckpt):
    """Default decoder path for up to 4 decoder positions: the three RMSNorms of a layer are folded into the weight-streaming
    GEMMs (the residual GEMMs leave fp16 rows + block sums of squares, the next GEMM forms the row factor itself).  Scores
    at L_d = 1 (product matrix: consumer and producer in one launch), 2 and 3 agree with the separate-kernel path and
    the fp32 oracle; rows stay independent of the batch they are scored in (bit-exact within a GEMM family: calls of <= 16 rows at
    L_d >= 2 take the few-row GEMV family, round 6)."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims, state, eng = toy[ckpt]
    seqs = _synth.synth_token_batch(37, 3, 150, dims.vocab, seed=78)      # 37 rows: two 32-row slabs of the GEMMs
    ids = [11, 12, 13, 14]
    orc = T5Oracle(dims, state)
    for prefix in ([0], [0, 17], [0, 17, 5]):
        want = orc.score_last(seqs[:9], prefix, ids)
        try:
            eng.set_option("dec_fold_norm", 0)
            plain = eng.score(seqs, prefix, ids)
        finally:
            eng.set_option("dec_fold_norm", 1)
        fold = eng.score(seqs, prefix, ids)
        assert np.abs(fold - plain).max() < 5e-3, (prefix, np.abs(fold - plain).max())
        assert np.abs(fold[:9] - want).max() < LOGIT_TOL and np.abs(plain[:9] - want).max() < LOGIT_TOL, prefix
        sub, one = eng.score(seqs[30:35], prefix, ids), eng.score(seqs[3:4], prefix, ids)
        if len(prefix) == 1:
            np.testing.assert_array_equal(sub, fold[30:35])
            np.testing.assert_array_equal(one, fold[3:4])
        else:
            # a handful of rows (option dec_gemv_rows: default 4, the kernel's limit 16) at >= 2 positions run on the few-row GEMV family (another K summation order): fp16
            # noise against the 74-row call, rows independent of the batch WITHIN the family, and the weight-streaming family
            # (dec_gemv = 0) bit-equal to the large call
            assert np.abs(sub - fold[30:35]).max() < 2e-3 and np.abs(one - fold[3:4]).max() < 2e-3, prefix   # (fp16 roundings of the stream flip)
            try:
                eng.set_option("dec_gemv_rows", 16)
                sub16 = eng.score(seqs[30:35], prefix, ids)
                np.testing.assert_array_equal(eng.score(seqs[32:33], prefix, ids), sub16[2:3])
                np.testing.assert_array_equal(eng.score(seqs[2:5], prefix, ids)[1:2], one)
                eng.set_option("dec_gemv", 0)
                np.testing.assert_array_equal(eng.score(seqs[30:35], prefix, ids), fold[30:35])
                np.testing.assert_array_equal(eng.score(seqs[3:4], prefix, ids), fold[3:4])
            finally:
                eng.set_option("dec_gemv", 1)
                eng.set_option("dec_gemv_rows", DEC_GEMV_ROWS_DEFAULT)
    tok, _ = eng.greedy(seqs[:6], [0], 3)                                   # L_d grows 1 -> 3 across the steps
    for i in (0, 5):
        np.testing.assert_array_equal(eng.greedy(seqs[i:i + 1], [0], 3)[0][0], tok[i])


@pytest.mark.parametrize("ckpt", ["ckpt_gated_untied", "ckpt_relu_tied"])
def test_decoder_one_position_with_ffn_in_streamed_and_few_row_gemms_tiled(toy, ckpt):
    """Options dec_ffn_tiled = 0 (the one-position decoder's FFN-in on the weight-streaming kernel) and gemm_skinny = 0 (every
    few-row GEMM on the tiled kernels - which also takes the decoder off the folded norm: it needs the weight-streaming family),
    each alone and both together, at one decoder position: within the oracle bound of this file, within the 5e-3 this file allows
    between the folded and the separate-norm path, and the passages in the same order as under the defaults.
    The order is compared on the passages the ORACLE tells apart: walking down its margins (logit 11 - logit 12), a passage is kept
    when it lies at least 2e-2 below the last one kept - four times the 5e-3 above: two paths, two logits per margin.  Closer
    passages have no order that fp16 arithmetic owes anybody: of the 37 passages here, 20 and 30 of the ReLU checkpoint are
    3.7e-4 apart in the oracle (-0.798362 / -0.798728), the default path has them the other way round (-0.799041 / -0.798520) and
    gemm_skinny = 0 the oracle's way (-0.797198 / -0.797602) - bit for bit what dec_fold_norm = 0 gives, an order the test above
    has accepted since the fold exists."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims, state, eng = toy[ckpt]
    seqs = _synth.synth_token_batch(37, 3, 150, dims.vocab, seed=79)
    ids = [11, 12, 13, 14]
    want = T5Oracle(dims, state).score_last(seqs, [0], ids)
    dw = want[:, 0] - want[:, 1]
    apart = []
    for i in np.argsort(-dw, kind="stable"):
        if not apart or dw[apart[-1]] - dw[i] >= 2e-2:
            apart.append(int(i))
    assert len(apart) >= 6, (len(apart), np.sort(dw))
    base = eng.score(seqs, [0], ids)
    assert np.abs(base - want).max() < LOGIT_TOL
    for opts in ({"dec_ffn_tiled": 0}, {"gemm_skinny": 0}, {"dec_ffn_tiled": 0, "gemm_skinny": 0}):
        try:
            for key, v in opts.items():
                eng.set_option(key, v)
            got = eng.score(seqs, [0], ids)
        finally:
            eng.set_option("dec_ffn_tiled", 1)
            eng.set_option("gemm_skinny", 1)                              # (1 = every epilogue kind: the default)
        assert np.abs(got - want).max() < LOGIT_TOL, (opts, np.abs(got - want).max())
        assert np.abs(_sigm(got[:, 0] - got[:, 1]) - _sigm(dw)).max() < SCORE_TOL, opts
        assert np.abs(got - base).max() < 5e-3, (opts, np.abs(got - base).max())
        db, dg = (base[:, 0] - base[:, 1])[apart], (got[:, 0] - got[:, 1])[apart]
        np.testing.assert_array_equal(np.argsort(-dg, kind="stable"), np.argsort(-db, kind="stable"), err_msg=str(opts))


@pytest.mark.parametrize("ckpt", ["ckpt_gated_untied", "ckpt_relu_tied"])
def test_two_token_greedy_with_candidates_equals_two_steps(toy, ckpt):
    """rk_t5_greedy2: the second step computed speculatively for every candidate first token, in the same decoder pass as
    the first - tokens and step count identical to rk_t5_greedy(max_new=2), whether the first token is a candidate
    (speculation hit), is not (fallback), or is EOS; one prompt and a batch; candidates beyond the workspace fall back."""
    from llmrankers import _synth
    dims, state, eng = toy[ckpt]
    seqs = _synth.synth_token_batch(5, 3, 120, dims.vocab, seed=91)
    for prefix in ([0], [0, 17]):
        want, wsteps = eng.greedy(seqs, prefix, 2)
        firsts = sorted(set(int(t) for t in want[:, 0]))
        cases = [firsts, firsts + [3, 4], [5, 6, 7] if not set(firsts) & {5, 6, 7} else [8, 9], list(range(20, 20 + 200))]
        for cand in cases:
            got, gsteps = eng.greedy(seqs, prefix, 2, candidates=cand)
            np.testing.assert_array_equal(got, want, err_msg=f"prefix {prefix} candidates {cand[:6]}")
            assert gsteps == wsteps
        for i in range(len(seqs)):
            one, _ = eng.greedy(seqs[i:i + 1], prefix, 2, candidates=firsts)
            np.testing.assert_array_equal(one[0], want[i])
        # EOS as the first token: pad follows and a single-row call stops after one step
        eos = int(want[0, 0])
        w1, s1 = eng.greedy(seqs[:1], prefix, 2, eos_id=eos)
        g1, t1 = eng.greedy(seqs[:1], prefix, 2, eos_id=eos, candidates=firsts)
        np.testing.assert_array_equal(g1, w1)
        assert (s1, t1) == (1, 1) and int(w1[0, 1]) == 0
    try:
        eng.set_option("greedy_spec", 0)                                     # switch: never speculate
        np.testing.assert_array_equal(eng.greedy(seqs, [0], 2, candidates=[3, 4])[0], eng.greedy(seqs, [0], 2)[0])
    finally:
        eng.set_option("greedy_spec", 160)


def test_fused_greedy_head_first_index_on_exact_ties(ckpt_dirs):
    """The greedy head never writes the logits: the head GEMM keeps per 32-column block the maximum and its first column,
    a second kernel picks per row.  Exact ties - identical lm_head rows in one block (both lane halves) and in later
    blocks - resolve to the FIRST index (torch.argmax).  Two tie groups, +8x and -8x one direction: whatever the sign of
    a row's projection, one group holds the row maximum, and the token must be that group's smallest index."""
    from llmrankers import _synth
    dims, state = load_state(ckpt_dirs["ckpt_gated_untied"])
    head = state["lm_head.weight"].copy()
    plus, minus = [37, 45, 59, 70, 131, 200], [38, 46, 60, 71, 132, 201]
    for r in plus:
        head[r] = head[40] * np.float32(8.0)
    for r in minus:
        head[r] = head[40] * np.float32(-8.0)
    state = dict(state)
    state["lm_head.weight"] = head
    eng = _engine(dims, state)
    try:
        seqs = _synth.synth_token_batch(8, 3, 90, dims.vocab, seed=3)
        tok, _ = eng.greedy(seqs, [0], 1)
        full = np.concatenate([eng.score(seqs, [0], list(range(c, min(c + 64, dims.vocab)))) for c in range(0, dims.vocab, 64)], axis=1)
        hits = 0
        for b in range(len(seqs)):
            assert len(set(full[b, plus].tolist())) == 1 and len(set(full[b, minus].tolist())) == 1   # the ties are exact
            want = int(np.argmax(full[b]))                                   # numpy: first index of the maximum
            others = np.delete(full[b], plus if want in plus else (minus if want in minus else [want]))
            if full[b, want] - others.max() > 0.05:                          # (the scored logits sum K in another order)
                assert int(tok[b, 0]) == want, (b, int(tok[b, 0]), want)
                hits += want in (37, 38)
        assert hits >= 3, hits                                              # a tie group won, and its FIRST index was returned
        # two new tokens and the candidate form go through the same head
        np.testing.assert_array_equal(eng.greedy(seqs, [0], 2, candidates=[37, 38])[0], eng.greedy(seqs, [0], 2)[0])
    finally:
        eng.close()


def test_comm_single_rank_gather_equals_local_scores(toy):
    """rk_comm_*: RCCL communicator of ONE rank on this GPU; the all_gather of the slot's device score buffer returns
    exactly what rk_t5_read_scores returns (the N > 1 path differs only in the number of ranks)."""
    from llmrankers import _synth
    dims, state, eng = toy["ckpt_gated_untied"]
    seqs = _synth.synth_token_batch(7, 4, 60, dims.vocab, seed=5)
    want = eng.score(seqs, [0], [21, 22])
    eng.comm_init(eng.comm_unique_id(), 0, 1, 64)
    try:
        eng.stage(seqs, slot=1)
        eng.score_staged([0], [21, 22], slot=1)
        eng.comm_all_gather(7 * 2, slot=1)
        got = eng.comm_read_gathered(1)
        assert got.shape == (1, 14)
        np.testing.assert_array_equal(got.reshape(7, 2), want)
        np.testing.assert_array_equal(eng.read_scores(1), want)
    finally:
        eng.comm_destroy()


TWO_RANK_WORKER = r'''
import os, sys, json, time
import numpy as np
repo, rank, idfile = sys.argv[1], int(sys.argv[2]), sys.argv[3]
sys.path[:0] = [os.path.join(repo, "llm-rankers_amd"), repo]
import torch
from llmrankers import _synth
from llmrankers._engine import RkEngine
dims = _synth.TOY_GATED_UNTIED
eng = RkEngine(dims, device=rank, max_tokens=2048, max_seqs=16, max_dec_len=8).load_state(_synth.synth_state_dict(dims, seed=11).items())
if rank == 0:
    with open(idfile + ".tmp", "wb") as f:
        f.write(eng.comm_unique_id())
    os.replace(idfile + ".tmp", idfile)
else:
    for _ in range(600):
        if os.path.exists(idfile):
            break
        time.sleep(0.1)
uid = open(idfile, "rb").read()
eng.comm_init(uid, rank, 2, 64)
seqs = _synth.synth_token_batch(13, 4, 60, dims.vocab, seed=5)
lo, hi = (0, 7) if rank == 0 else (7, 13)
local = eng.score(seqs[lo:hi], [0], [21, 22])
eng.comm_all_gather(7 * 2, slot=0)
allv = eng.comm_read_gathered(0)
print("RESULT " + json.dumps({"local": local.tolist(), "all": allv.tolist()}))
eng.comm_destroy(); eng.close()
'''


def test_comm_two_ranks_gather(tmp_path):
    """Two processes, one GPU each: 13 candidates sharded 7 + 6, ONE engine-issued RCCL all_gather; both ranks end up
    with both score blocks, equal to a single-GPU run.  Skipped on a 1-GPU box."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from conftest import REPO
    w = tmp_path / "worker.py"
    w.write_text(TWO_RANK_WORKER)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(w), REPO, str(r), str(tmp_path / "uid.bin")], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, env=env) for r in range(2)]
    outs = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-2000:]
        outs.append(json.loads(next(l for l in out.splitlines() if l.startswith("RESULT "))[7:]))
    a0, a1 = np.array(outs[0]["all"]), np.array(outs[1]["all"])
    np.testing.assert_array_equal(a0, a1)
    np.testing.assert_array_equal(a0[0].reshape(7, 2), np.array(outs[0]["local"]))
    np.testing.assert_array_equal(a0[1][:12].reshape(6, 2), np.array(outs[1]["local"]))


def test_comm_single_rank_appended_gather_of_a_multi_chunk_share(toy):
    """A rank's share that needs SEVERAL engine calls (here max_seqs = 4 against 11 passages: 3 calls): each call's scores
    are appended to the engine's send buffer on the device (rk_comm_append_scores_slot) and ONE all_gather ships the whole
    share - through the real T5Runtime.sharded_scores, for yes_no logits and for qlm, with a one-rank RCCL communicator.
    (Round 2 gathered slot 0's buffer after the last call: everything but the last chunk was lost.)"""
    from llmrankers import _synth
    from llmrankers._runtime import T5Runtime
    dims, state, _ = toy["ckpt_gated_untied"]
    eng = _engine(dims, state, max_tokens=2048, max_seqs=4, max_dec_len=8)
    rt = T5Runtime.from_engine(eng, dims)
    eng.comm_init(eng.comm_unique_id(), 0, 1, 256)
    assert rt.comm_capacity == 256                       # the ENGINE's figure, whoever built the communicator
    info = eng.comm_library_info()
    assert "librccl" in info and int(info.rsplit("|", 1)[1]) > 0, info
    try:
        seqs = _synth.synth_token_batch(11, 4, 60, dims.vocab, seed=5)
        want = np.concatenate([eng.score(seqs[i:i + 4], [0], [21, 22]) for i in range(0, 11, 4)])
        # scores [13 x 2] then host side data [13] (the prompts' token counts of a sharded query) in ONE gather
        lens = np.asarray([len(q) for q in seqs], dtype=np.float32)
        local, allv = rt.sharded_scores("score", seqs, [0], [21, 22], 13 * 3, tail=lens, tail_offset=13 * 2)
        np.testing.assert_array_equal(local.reshape(11, 2), want)
        np.testing.assert_array_equal(np.asarray(allv).reshape(-1)[:22].reshape(11, 2), want)
        np.testing.assert_array_equal(np.asarray(allv).reshape(-1)[26:37], lens)
        with pytest.raises(ValueError):                   # beyond the send buffer: refused on the host, before any collective
            rt.sharded_scores("score", seqs, [0], [21, 22], 257)
        labels = [0, 5, 9, 17]
        want_q = np.concatenate([eng.qlm(seqs[i:i + 4], labels) for i in range(0, 11, 4)])
        local_q, allv_q = rt.sharded_scores("qlm", seqs, labels, None, 13)
        np.testing.assert_array_equal(local_q, want_q)
        np.testing.assert_array_equal(np.asarray(allv_q).reshape(-1)[:11], want_q)
    finally:
        eng.comm_destroy()
        eng.close()


def test_comm_single_rank_grouped_sharded_rerank_many(toy, ckpt_dirs):
    """Round 6: PointwiseLlmRanker.rerank_many under candidate sharding (run.py's default with --shard_candidates 1): the shares
    of SEVERAL queries in one launch sequence - here through a one-rank RCCL communicator (the one-GPU box's way into the
    sharded code path), engine calls of at most five sequences so that the group takes several appends - and ONE gather for all
    of them; rankings, scores (bit for bit: a passage's score does not depend on what shares its call) and counters equal the
    same queries one at a time, sharded and unsharded."""
    import contextlib, io
    from transformers import T5Tokenizer
    from llmrankers._runtime import T5Runtime
    from llmrankers.pointwise import PointwiseLlmRanker
    from llmrankers.rankers import SearchResult
    dims, state, _ = toy["ckpt_gated_untied"]
    with open(os.path.join(GOLD, "rerank_cases.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["kind"] == "pointwise" and c["ckpt"] == "ckpt_gated_untied" and c["method"] == "yes_no"]
    bs = cases[0]["batch_size"]
    cases = [c for c in cases if c["batch_size"] == bs]
    eng = _engine(dims, state, max_tokens=2048, max_seqs=5, max_dec_len=8)
    rt = T5Runtime.from_engine(eng, dims)
    tok = T5Tokenizer.from_pretrained(ckpt_dirs["ckpt_gated_untied"])
    fresh = lambda c: [SearchResult(docid=d, score=s, text=t) for d, s, t in c["input"]]
    plain = PointwiseLlmRanker.from_runtime(rt, tok, method="yes_no", batch_size=bs)
    want = []
    for c in cases:
        r = plain.rerank(c["query"], fresh(c))
        want.append(([(x.docid, x.score) for x in r], (plain.total_compare, plain.total_prompt_tokens, plain.total_completion_tokens)))
    eng.comm_init(eng.comm_unique_id(), 0, 1, 4096)
    try:
        rk = PointwiseLlmRanker.from_runtime(rt, tok, method="yes_no", batch_size=bs, shard_candidates=True)
        ranked, counters = rk.rerank_many([(c["query"], fresh(c)) for c in cases] + [(cases[0]["query"], [])])
        assert ranked[-1] == [] and tuple(counters[-1]) == (0, 0, 0)
        for c, r, cnt, (w, wc) in zip(cases, ranked, counters, want):
            assert [(x.docid, x.score) for x in r] == w and tuple(cnt) == wc
            assert [x.docid for x in r] == [d for d, _ in c["result"]]
        one = rk.rerank(cases[0]["query"], fresh(cases[0]))           # and the single-query sharded path still agrees
        assert [(x.docid, x.score) for x in one] == want[0][0]
    finally:
        eng.comm_destroy()
        eng.close()


TWO_RANK_API_WORKER = r'''
import json, os, sys
repo, ck = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(repo, "llm-rankers_amd"), repo]
import torch
import torch.distributed as dist
dist.init_process_group("gloo")                       # host control plane; the scores travel over the engine's RCCL
from llmrankers.pointwise import PointwiseLlmRanker
from llmrankers.rankers import SearchResult
case = json.load(open(sys.argv[3]))
rk = PointwiseLlmRanker(ck, ck, "cuda", method=case["method"], batch_size=case["batch_size"], shard_candidates=True)
rk.llm.max_seqs = 3                                   # a share of 7 / 6 passages then takes three / two engine calls
out = []
for rep in range(2):
    ranking = [SearchResult(docid=d, score=s, text=t) for d, s, t in case["input"]]
    res = rk.rerank(case["query"], ranking)
    out.append([[r.docid, r.score] for r in res])
print("RESULT " + json.dumps({"rankings": out, "comm_world": rk.llm.engine.comm_world}))
dist.destroy_process_group()
'''


def _two_gpu_env(port):
    return dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")


def test_two_ranks_pointwise_ranker_and_run_py_shard_candidates(tmp_path, ckpt_dirs):
    """The product path of BASELINE configs[3] on two GPUs: PointwiseLlmRanker(shard_candidates=True) builds the engine's
    RCCL communicator itself on the first sharded query, multi-call shares are gathered whole, both ranks return the
    reference's ranking; then run.py --num_gpus 2 (self-spawned) writes the run file of a single-GPU run.  Skipped on a
    1-GPU box (ready for the driver's 8-GPU tier)."""
    import socket
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from conftest import GOLD, REPO
    with open(os.path.join(GOLD, "rerank_cases.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["kind"] == "pointwise" and c["ckpt"] == "ckpt_gated_untied"]
    ck = ckpt_dirs["ckpt_gated_untied"]
    (tmp_path / "worker.py").write_text(TWO_RANK_API_WORKER)
    for method, n_docs in (("yes_no", 13), ("qlm", 10)):
        case = next(c for c in cases if c["method"] == method and len(c["input"]) == n_docs)
        (tmp_path / "case.json").write_text(json.dumps(case))
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        procs = [subprocess.Popen([sys.executable, str(tmp_path / "worker.py"), REPO, ck, str(tmp_path / "case.json")],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                  env=dict(_two_gpu_env(port), RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
        outs = []
        for p in procs:
            out, err = p.communicate(timeout=900)
            assert p.returncode == 0, err[-2000:]
            outs.append(json.loads(next(l for l in out.splitlines() if l.startswith("RESULT "))[7:]))
        assert outs[0]["rankings"] == outs[1]["rankings"] and all(o["comm_world"] == 2 for o in outs)
        for ranking in outs[0]["rankings"]:
            assert [d for d, _ in ranking] == [d for d, _ in case["result"]]
            np.testing.assert_allclose([s for _, s in ranking], [s for _, s in case["result"]], atol=SCORE_TOL if method == "yes_no" else 5e-2)
    # run.py: --num_gpus 2 against a single-GPU run of the same command
    (tmp_path / "q.tsv").write_text("q1\tneural ranking model\nq2\twater river mountain\n")
    (tmp_path / "d.tsv").write_text("\n".join(f"d{i}\t{w}" for i, w in enumerate(
        ["search engine index", "river water city", "music art film", "vaccine covid virus", "bank money trade",
         "neural model answer", "mountain river water"])) + "\n")
    (tmp_path / "in.trec").write_text("\n".join(f"{q} Q0 d{i} {r + 1} {10 - r} bm25" for q in ("q1", "q2") for r, i in enumerate(range(7))) + "\n")

    def run(save, extra):
        cmd = [sys.executable, os.path.join(REPO, "run.py"), "run", "--model_name_or_path", ck, "--run_path", str(tmp_path / "in.trec"),
               "--save_path", str(save), "--query_file", str(tmp_path / "q.tsv"), "--doc_file", str(tmp_path / "d.tsv"), "--hits", "7",
               *extra, "pointwise", "--method", "yes_no", "--batch_size", "3"]
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(env, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        assert r.returncode == 0, r.stderr[-2000:]
        return [l.split("\t") for l in open(save).read().splitlines()]
    a = run(tmp_path / "one.trec", [])
    b = run(tmp_path / "two.trec", ["--num_gpus", "2"])
    assert [x[:4] + x[5:] for x in a] == [x[:4] + x[5:] for x in b] and len(a) == 14
    assert [x[4] for x in a] == [x[4] for x in b]             # bit-identical scores: a passage's bits do not depend on its batch


def test_qlm_flan_t5_xl_dims_vs_oracle_and_batch_independence():
    """BASELINE.json configs[3] model shape (flan-t5-xl: d_model 2048, 32 heads, d_ff 5120, 24+24 layers), pointwise qlm:
    3 ragged passages x 33 label positions vs the fp32 oracle (relative 5e-4 on sums of ~33 log-probs), then the call
    shape of an 8-way shard of hits=100 (13 passages x 33 labels) for batch independence and permutation equivariance."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims = _synth.FLAN_T5_XL
    state = _synth.synth_state_dict(dims, seed=929, threads=32)
    eng = _engine(dims, state, max_tokens=4096, max_seqs=16, max_dec_len=40)
    labels = [0] + np.random.RandomState(6).randint(3, dims.vocab - 28, size=32).tolist()
    ragged = _synth.synth_token_batch(3, 30, 150, dims.vocab, seed=41)
    got = eng.qlm(ragged, labels)
    want = T5Oracle(dims, state).qlm(ragged, labels)
    assert np.abs(got - want).max() / np.abs(want).max() < 5e-4, (got, want)
    shard = _synth.synth_token_batch(13, 100, 150, dims.vocab, seed=42)
    full = eng.qlm(shard, labels)
    assert np.isfinite(full).all()
    perm = np.random.RandomState(2).permutation(13)
    np.testing.assert_array_equal(eng.qlm([shard[i] for i in perm], labels), full[perm])
    np.testing.assert_array_equal(eng.qlm(shard[4:6], labels), full[4:6])
    # yes_no at the same width: 8 heads per workgroup pairs, rmsnorm_kernel<8>, 2048-wide rows in every kernel
    sc = eng.score(ragged, [0], [2163, 465])
    ref = T5Oracle(dims, state).score_last(ragged, [0], [2163, 465])
    assert np.abs(_sigm(sc[:, 0] - sc[:, 1]) - _sigm(ref[:, 0] - ref[:, 1])).max() < SCORE_TOL
    eng.close()


def _llama_state(spec):
    from llmrankers import _synth
    dims = _synth.NAMED_DIMS[spec["dims"]]
    state = _synth.synth_state_dict(dims, seed=spec["seed"], gain=spec.get("gain", 1.0))
    if spec.get("boost_ids"):
        w = state["lm_head.weight"].copy()
        ids = np.asarray(spec["boost_ids"], dtype=np.int64)
        w[ids] = (w[ids] * np.float32(spec["boost"])).astype(np.float16).astype(np.float32)
        state["lm_head.weight"] = w
    return dims, state


def test_llama_toy_vs_hf_golden_and_reference_cases(ckpt_dirs):
    """Llama family (rk_llama_*: RoPE, grouped-query causal attention with head_dim 128, SwiGLU, folded RMSNorm) through
    the product path (checkpoint directory -> LlamaRuntime -> C ABI): last-position logits vs HF's LlamaForCausalLM,
    batch independence, and every compare of the reference's SetwiseLlmRanker cases (greedy token = the oracle's
    wherever its margin is above the fp16 noise floor; trajectory follows the recorded one)."""
    import contextlib, io, random
    from transformers import AutoTokenizer
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import SetwiseLlmRanker
    from oracle.llama_numpy import LlamaOracle
    g = np.load(os.path.join(GOLD, "model_llama.npz"))
    rt = LlamaRuntime(ckpt_dirs["ckpt_llama"], "cuda", max_tokens=8192, max_seqs=16)
    off = np.concatenate([[0], np.cumsum(g["lens"])])
    seqs = [g["tokens"][off[i]:off[i + 1]].astype(np.int32) for i in range(len(g["lens"]))]
    scale = float(np.abs(g["last_logits"]).max())
    cols = list(range(0, 256, 4))
    got = rt.last_logits(seqs, cols)
    err = np.abs(got - g["last_logits"][:, cols]).max()
    assert err < 6e-3 * scale, (err, scale)                       # hot (gain 2) toy weights, logits up to ~35
    for b, s in enumerate(seqs):                                  # one prompt at a time == all together (ragged batch)
        np.testing.assert_array_equal(rt.last_logits([s], cols)[0], got[b])
    tok_want = np.argmax(g["last_logits"], axis=-1)
    top2 = np.sort(g["last_logits"], axis=-1)[:, -2:]
    tok_got = rt.greedy1(seqs)
    for b in range(len(seqs)):
        if top2[b, 1] - top2[b, 0] > 0.02 * scale:
            assert tok_got[b] == tok_want[b]
    # ---- the reference's setwise cases: engine checked against the oracle on every compare ----
    with open(os.path.join(GOLD, "llama_cases.json")) as f:
        gold = json.load(f)
    with open(os.path.join(GOLD, "ckpts.json")) as f:
        dims, state = _llama_state(json.load(f)["ckpt_llama"])
    orc = LlamaOracle(dims, state)
    tok = AutoTokenizer.from_pretrained(ckpt_dirs["ckpt_llama"])
    stats = {"calls": 0, "decided": 0}

    class Checked:
        model_type, config = "llama", rt.config

        def greedy1(self, prompts):
            want = orc.last_logits(prompts)
            got_tok = rt.greedy1(prompts)
            for b in range(len(prompts)):
                two = np.sort(want[b])[-2:]
                stats["calls"] += 1
                if two[1] - two[0] > 0.02 * scale:
                    stats["decided"] += 1
                    assert got_tok[b] == int(np.argmax(want[b]))
            return np.argmax(want, axis=-1).astype(np.int32)

    for case in gold["cases"]:
        rk = SetwiseLlmRanker.from_runtime(Checked(), tok, num_child=case["num_child"], k=case["k"], scoring=case["scoring"],
                                           method=case["method"], num_permutation=case["num_permutation"])
        ranking = [SearchResult(docid=d, score=s, text=t) for d, s, t in case["input"]]
        random.seed(929)
        if case["raises"]:
            with pytest.raises({"IndexError": IndexError, "NotImplementedError": NotImplementedError}[case["raises"]]), contextlib.redirect_stdout(io.StringIO()):
                rk.rerank(case["query"], ranking)
            continue
        with contextlib.redirect_stdout(io.StringIO()):
            res = rk.rerank(case["query"], ranking)
        assert [[r.docid, r.score] for r in res] == case["result"]
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"]
    assert stats["calls"] >= 40 and stats["decided"] >= 0.7 * stats["calls"], stats
    rt.engine.close()


def test_llama_3_8b_widths_one_compare_vs_oracle():
    """BASELINE.json configs[4] shapes: Llama-3-8B widths (hidden 4096, 32 query / 8 kv heads x 128, SwiGLU 14336, vocabulary
    128256, rope_theta 5e5) with two layers (the oracle runs on the host): one ~700-token setwise-sized prompt and a short
    one in the same call; label logits vs the fp32 oracle, same greedy token, batch independence."""
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    from oracle.llama_numpy import LlamaOracle
    dims = _synth.LlamaDims(vocab=128256, hidden=4096, n_heads=32, n_kv_heads=8, head_dim=128, intermediate=14336, n_layers=2,
                            bos_token_id=128000, eos_token_id=128001)
    state = _synth.synth_state_dict(dims, seed=929, threads=32)
    eng = RkLlamaEngine(dims, device=0, max_tokens=4096, max_seqs=8).load_state(state.items())
    seqs = [s for n in (700, 45) for s in _synth.synth_token_batch(1, n, n, dims.vocab, seed=100 + n)]
    labels = list(range(32, 32 + 23))
    orc = LlamaOracle(dims, state)
    want_full = orc.last_logits(seqs)
    got = eng.last_logits(seqs, labels)
    scale = float(np.abs(want_full).max())
    assert np.abs(got - want_full[:, labels]).max() < 4e-3 * scale, (np.abs(got - want_full[:, labels]).max(), scale)
    toks = eng.greedy1(seqs)
    for b in range(2):
        two = np.sort(want_full[b])[-2:]
        if two[1] - two[0] > 0.02 * scale:
            assert toks[b] == int(np.argmax(want_full[b]))
    np.testing.assert_array_equal(eng.last_logits(seqs[:1], labels)[0], got[0])
    np.testing.assert_array_equal(eng.last_logits(seqs[1:], labels)[0], got[1])
    eng.close()


def test_llama_attention_by_lds_dma_vs_oracle_first_kernel_and_batch_independence():
    """attn_causal_dma_kernel (round 5: K / V chunks of 64 keys by LDS-DMA, V^T by transposing reads; engine option
    llama_attn_dma): the last-position logits of MANY PREFIXES of one 700-token sequence - the logits of many positions: every
    chunk count, the diagonal chunk at both halves, query-block boundaries, a one-token sequence - against the fp32 oracle (as
    close as the register-staged kernel), the two kernels within fp16 noise of each other, and batch independence: a prefix
    alone, in the batch and in the reversed batch (other workgroup -> XCD assignment) gives the same bits."""
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    from oracle.llama_numpy import LlamaOracle
    dims = _synth.TOY_LLAMA
    state = _synth.synth_state_dict(dims, seed=929)
    base = _synth.synth_token_batch(1, 700, 700, dims.vocab, seed=17)[0]
    lens = sorted(set([1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 255, 256, 257, 383, 384,
                       385, 511, 512, 513, 639, 640, 641, 700] + list(range(7, 700, 37))))
    seqs = [base[:n] for n in lens]
    ids = list(range(64))
    want = LlamaOracle(dims, state).last_logits(seqs)[:, ids]
    scale = float(np.abs(want).max())
    eng = RkLlamaEngine(dims, device=0, max_tokens=32768, max_seqs=128).load_state(state.items())
    eng.set_option("llama_attn_dma", 0)
    first = eng.last_logits(seqs, ids)
    eng.set_option("llama_attn_dma", 1)
    got = eng.last_logits(seqs, ids)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() < 2e-3 * max(1.0, scale), (np.abs(got - want).max(), scale)
    assert np.abs(got - want).max() < 1.5 * np.abs(first - want).max() + 1e-4
    assert np.abs(got - first).max() < 2e-3 * max(1.0, scale)
    np.testing.assert_array_equal(eng.last_logits(seqs[::-1], ids)[::-1], got)
    eng.set_option("llama_attn_nw", 8)                              # eight waves per workgroup: the same bits
    np.testing.assert_array_equal(eng.last_logits(seqs, ids), got)
    eng.set_option("llama_attn_nw", 0)
    for i in (0, 3, 8, 17, len(seqs) - 1):
        np.testing.assert_array_equal(eng.last_logits([seqs[i]], ids)[0], got[i], err_msg=f"prefix of {lens[i]} tokens alone")
    eng.close()


def test_llama3_rope_scaling_on_the_engine_vs_hf_golden():
    """rope type "llama3" (Llama-3.1 / 3.2 checkpoints; rk_llama_set_rope_scaling before finalize): last-position logits of
    ragged prompts vs HF LlamaForCausalLM (tests/golden/model_llama3rope.npz) and vs the oracle; the default rope type on
    the same weights must NOT match (a scaling that is silently ignored would)."""
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    g = np.load(os.path.join(GOLD, "model_llama3rope.npz"))
    dims = _synth.NAMED_DIMS["toy-llama3rope"]
    state = _synth.synth_state_dict(dims, seed=int(g["seed"]), gain=float(g["gain"]))
    off = np.concatenate([[0], np.cumsum(g["lens"])])
    seqs = [g["tokens"][off[i]:off[i + 1]].astype(np.int32) for i in range(len(g["lens"]))]
    want = g["last_logits"]
    ids = list(range(dims.vocab))
    eng = RkLlamaEngine(dims, device=0, max_tokens=2048, max_seqs=8).load_state(state.items())
    def all_logits(e):                                   # rk_llama_last_logits takes up to 64 vocabulary rows per call
        return np.concatenate([e.last_logits(seqs, ids[c:c + 64]) for c in range(0, len(ids), 64)], axis=1)
    got = all_logits(eng)
    scale = float(np.abs(want).max())
    assert np.abs(got - want).max() < 8e-3 * scale, (np.abs(got - want).max(), scale)
    np.testing.assert_array_equal(eng.greedy1(seqs)[np.sort(want, axis=1)[:, -1] - np.sort(want, axis=1)[:, -2] > 0.05 * scale],
                                  np.argmax(want, axis=1)[np.sort(want, axis=1)[:, -1] - np.sort(want, axis=1)[:, -2] > 0.05 * scale])
    eng.close()
    plain = _synth.LlamaDims(**{**dims.__dict__, "rope_scaling": None})
    eng2 = RkLlamaEngine(plain, device=0, max_tokens=2048, max_seqs=8).load_state(state.items())
    assert np.abs(all_logits(eng2) - want).max() > 5 * 8e-3 * scale
    eng2.close()


def test_llama_3_8b_full_depth_vs_oracle_golden():
    """BASELINE.json configs[4] at FULL depth: Llama-3-8B dimensions, all 32 layers.  (1) one 700-token setwise-sized prompt:
    the label logits and the greedy token against the fp32 oracle's (tests/golden/llama8b_full_depth.json, generated once by
    tools/make_llama8b_golden.py - 32 GB of fp32 weights do not fit a test run on the host).  (2) the whole setwise heapsort
    query of tests/golden/llama_setwise_query.json (hits=100, num_child=10, k=10, generation; its oracle run exists at two
    layers only, test_gpu_rerank.py) through SetwiseLlmRanker at the full depth, for its properties: the run is
    deterministic, the level-batched driver and four queries in lockstep (rerank_many) give the one-by-one rankings and
    counters (batch independence), the counters add up, and generations are labels.  The 8 G synthetic weights are
    regenerated here from their counters and streamed into the engine; the lm_head rows of the 23 label tokens are boosted
    (x6, like the fixture checkpoints) so that greedy tokens are labels - part (1) therefore reads the golden's un-boosted
    rows, and checks the fused arg-max head against the logits of the boosted rows and the golden's top token."""
    import contextlib, io
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    path = os.path.join(GOLD, "llama8b_full_depth.json")
    if not os.path.exists(path):
        pytest.skip("golden not generated")
    with open(path) as f:
        gold = json.load(f)
    qpath = os.path.join(GOLD, "llama_setwise_query.json")
    qgold = json.load(open(qpath)) if os.path.exists(qpath) else None
    boost_ids = list(qgold["boost_ids"]) if qgold else []
    boost = float(qgold["boost"]) if qgold else 1.0
    dims = _synth.NAMED_DIMS[gold["dims"]]

    def tensors():
        for name, arr in _synth.synth_tensors(dims, seed=gold["seed"], threads=min(48, os.cpu_count() or 8)):
            if name == "lm_head.weight" and boost_ids:
                arr = np.array(arr, dtype=np.float32, copy=True)
                rows = np.asarray(boost_ids, dtype=np.int64)
                arr[rows] = (arr[rows] * np.float32(boost)).astype(np.float16).astype(np.float32)
            yield name, arr
    eng = RkLlamaEngine(dims, device=0, max_tokens=16384, max_seqs=16)
    eng.load_state(tensors())
    ids = _synth.synth_token_batch(1, gold["prompt_len"], gold["prompt_len"], dims.vocab, seed=gold["prompt_seed"])
    keep = [k for k, t in enumerate(gold["label_ids"]) if t not in boost_ids]
    got = eng.last_logits(ids, [gold["label_ids"][k] for k in keep])[0]
    want = np.asarray(gold["label_logits"], dtype=np.float32)[keep]
    scale = gold["logit_abs_max"]
    err = float(np.abs(got - want).max())
    print(f"[llama8b full depth] max |label logit - oracle| = {err:.4f} at logit scale {scale:.3f}")
    assert err < 4e-3 * scale, (err, scale)            # measured 6e-4 of the scale: 32 layers of fp16 operands, fp32 stream
    top = eng.last_logits(ids, gold["top_ids"])[0]
    assert np.abs(top - np.asarray(gold["top_logits"], dtype=np.float32)).max() < 4e-3 * scale
    # fused arg-max head: the greedy token is the best of (the golden's top token, the boosted label rows)
    cand = [gold["top_ids"][0]] + boost_ids
    cl = eng.last_logits(ids, cand)[0]
    best2 = np.sort(cl)[-2:]
    if (not boost_ids and gold["top_logits"][0] - gold["top_logits"][1] > 4e-2 * scale) or (boost_ids and best2[1] - best2[0] > 4e-2 * scale):
        assert int(eng.greedy1(ids)[0]) == cand[int(np.argmax(cl))]
    # (1b) round 6: compares OF THE HEAPSORT QUERY at the full depth against the fp32 oracle (tools/make_llama8b_compares_golden.py:
    # the first prompts of the one-by-one sort, ~500 tokens each, label rows boosted as here): label logits, greedy token wherever
    # the oracle's margin is above the fp16 noise floor - and at least three of them are (asserted: no dead branch)
    qc = gold.get("query_compares")
    if qc:
        assert qgold and list(qc["boost_ids"]) == boost_ids and float(qc["boost"]) == boost
        decided = 0
        for k, rec in enumerate(qc["compares"]):
            prompt = [np.asarray(rec["prompt"], dtype=np.int32)]
            cscale = rec["logit_abs_max"]
            lg = eng.last_logits(prompt, boost_ids)[0]
            lerr = float(np.abs(lg - np.asarray(rec["label_logits"], dtype=np.float32)).max())
            print(f"[llama8b full depth] query compare {k}: {len(rec['prompt'])} tokens, max |label logit - oracle| = {lerr:.4f} at scale {cscale:.2f}, "
                  f"oracle margin {rec['margin']:.3f}")
            assert lerr < 4e-3 * cscale, (k, lerr, cscale)
            if rec["margin"] > 4e-2 * cscale:
                decided += 1
                assert int(eng.greedy1(prompt)[0]) == rec["token"], (k, rec["margin"])
        assert decided >= 3, decided
    if qgold:
        from transformers import AutoTokenizer
        from llmrankers._runtime import LlamaRuntime
        from llmrankers.rankers import SearchResult
        from llmrankers.setwise import SetwiseLlmRanker
        rt = LlamaRuntime.from_engine(eng, dims)
        tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, "tok_llama"))

        def fresh():
            return [SearchResult(docid=f"d{i}", score=float(100 - i), text=t) for i, t in enumerate(qgold["docs"])]

        def run(batched):
            rk = SetwiseLlmRanker.from_runtime(rt, tok, num_child=10, k=10, scoring="generation", method="heapsort")
            rk.batch_independent_compares = batched
            lens = []
            orig = rt.greedy1
            rt.greedy1 = lambda seqs: (lens.extend(len(s_) for s_ in seqs), orig(seqs))[1]
            sink = io.StringIO()
            try:
                with contextlib.redirect_stdout(sink):
                    res = rk.rerank(qgold["query"], fresh())
            finally:
                rt.greedy1 = orig
            return rk, [[r.docid, r.score] for r in res], lens, sink.getvalue().count("Unexpected output")
        rk_a, res_a, lens_a, bad_a = run(False)
        rk_b, res_b, lens_b, _ = run(False)
        assert res_a == res_b and lens_a == lens_b                                   # deterministic
        assert len(res_a) == 100 and sorted(d for d, _ in res_a) == sorted(f"d{i}" for i in range(100))
        assert rk_a.total_compare == len(lens_a) and rk_a.total_prompt_tokens == sum(lens_a)
        assert rk_a.total_completion_tokens == sum(lens_a) + len(lens_a)             # prompt + one new token per compare
        assert bad_a <= 0.1 * len(lens_a), bad_a                                     # generations are labels (boosted rows)
        rk_c, res_c, lens_c, _ = run(True)                                           # level-batched build phase
        assert res_c == res_a and sorted(lens_c) == sorted(lens_a)
        assert (rk_c.total_compare, rk_c.total_prompt_tokens, rk_c.total_completion_tokens) == \
               (rk_a.total_compare, rk_a.total_prompt_tokens, rk_a.total_completion_tokens)
        rk_m = SetwiseLlmRanker.from_runtime(rt, tok, num_child=10, k=10, scoring="generation", method="heapsort")
        q2 = qgold["query"].split()
        queries = [qgold["query"], " ".join(reversed(q2)), " ".join(q2[1:] + q2[:1]), qgold["query"]]
        with contextlib.redirect_stdout(io.StringIO()):
            many, counters = rk_m.rerank_many([(q, fresh()) for q in queries])       # four heapsorts in lockstep
        assert [[r.docid, r.score] for r in many[0]] == res_a and [[r.docid, r.score] for r in many[3]] == res_a
        assert tuple(counters[0]) == (rk_a.total_compare, rk_a.total_prompt_tokens, rk_a.total_completion_tokens)
        print(f"[llama8b full depth] setwise query: {rk_a.total_compare} compares, {rk_a.total_prompt_tokens} prompt tokens, "
              f"{bad_a} non-label generations; top-10 {[d for d, _ in res_a[:10]]}")
    eng.close()


def test_flan_t5_large_full_batch_vs_hf_golden():
    """BASELINE.json configs[1] at full size against the reference's arithmetic: the whole bench batch (32 x 184 tokens) and
    a ragged batch (32 passages of 96..184 tokens, the S2 workload) at flan-t5-large dimensions vs HF fp32 logits generated
    once in the build container (tools/make_large_batch_golden.py): probabilities within 1e-3 (north_star's tolerance),
    same order wherever the reference's adjacent scores differ by more than the tolerance.  Third tag (round 6), "outlier": the
    same model with a few stream channels / FFN hidden units two orders of magnitude above the rest (a TRAINED T5's activation
    shape): held to the reference's own fp16-path error against fp32, recorded with the fixture."""
    from llmrankers import _synth
    path = os.path.join(GOLD, "config2_large_batch.npz")
    if not os.path.exists(path):
        pytest.skip("golden not generated")
    g = np.load(path)
    dims = _synth.FLAN_T5_LARGE
    base_state = _synth.synth_state_dict(dims, seed=int(g["seed"]), threads=16)
    eng = _engine(dims, base_state, max_tokens=8192, max_seqs=32, max_dec_len=4)
    ids = g["ids"].tolist()
    assert "outlier.logits" in g.files                     # round 6: the trained-checkpoint-shaped case is part of the fixture
    for tag in ("uniform", "ragged", "outlier"):
        n, lo, hi, seed = (int(x) for x in g[f"{tag}.args"])
        seqs = _synth.synth_token_batch(n, lo, hi, dims.vocab, seed=seed)
        if tag == "outlier":
            # a few stream channels / FFN hidden units two orders of magnitude above the rest (what a trained T5 looks like and
            # what the 1 / 16-scaled fp16 copy of the stream and the fp16 saturation are for): a fresh engine with those weights
            eng.close()
            eng = _engine(dims, _synth.with_outlier_channels(base_state, dims), max_tokens=8192, max_seqs=32, max_dec_len=4)
            print(f"[outlier] HF fp32 stream: max |x| {float(g['outlier.stream_absmax']):.0f}, median {float(g['outlier.stream_median']):.2f}")
            assert float(g["outlier.stream_absmax"]) > 100 * float(g["outlier.stream_median"])
        got, want = eng.score(seqs, [0], ids), g[f"{tag}.logits"]
        if tag == "outlier":
            # With activations this peaked the attention scores run in the hundreds and fp16 q / k alone move them by tenths: 1e-3
            # against fp32 is not what fp16 inference delivers on such a model - the REFERENCE's own accelerator precision (HF
            # torch_dtype=float16 with fp32 `wo`, recorded on the first 8 passages: outlier.logits_hf_fp16) is 0.12 away from fp32
            # at logit scale 1.6.  The engine is held to that: no further from fp32 than 1.5 x the reference's fp16 path on the
            # same passages, 2 x over the whole batch; the probability error likewise.
            ref16 = g["outlier.logits_hf_fp16"]
            n16 = len(ref16)
            ref_err = float(np.abs(ref16 - want[:n16]).max())
            err8, err_all = float(np.abs(got[:n16] - want[:n16]).max()), float(np.abs(got - want).max())
            p_ref_err = float(np.abs(_sigm(ref16[:, 0] - ref16[:, 1]) - _sigm(want[:n16, 0] - want[:n16, 1])).max())
            p_err = float(np.abs(_sigm(got[:, 0] - got[:, 1]) - _sigm(want[:, 0] - want[:, 1])).max())
            print(f"[outlier] max |logit - HF fp32|: engine {err8:.4f} (8 passages) / {err_all:.4f} (32), HF fp16 {ref_err:.4f} (8); "
                  f"max |P(yes) - fp32|: engine {p_err:.4f}, HF fp16 {p_ref_err:.4f}")
            assert ref_err > 10 * SCORE_TOL                      # the case is hard for fp16 (else it pins nothing)
            assert err8 < 1.5 * ref_err and err_all < 2.0 * ref_err, (err8, err_all, ref_err)
            assert p_err < 2.0 * p_ref_err, (p_err, p_ref_err)
            continue
        p_got, p_want = _sigm(got[:, 0] - got[:, 1]), _sigm(want[:, 0] - want[:, 1])
        err = float(np.abs(p_got - p_want).max())
        print(f"[{tag}] max |P(yes) - HF fp32| over {n} passages = {err:.2e}")
        assert err < SCORE_TOL, (tag, err)
        order_got, order_want = np.argsort(-p_got, kind="stable"), np.argsort(-p_want, kind="stable")
        gaps = np.abs(np.diff(p_want[order_want]))
        if gaps.min() > 2 * SCORE_TOL:
            np.testing.assert_array_equal(order_got, order_want)
    eng.close()


def test_llama_pairwise_reference_cases_on_the_engine(ckpt_dirs):
    """PairwiseLlmRanker on a Llama-family checkpoint through its PUBLIC constructor (checkpoint directory -> rk_llama engine):
    the reference's heapsort / bubblesort queries (tests/golden/llama_pairwise_cases.json, ref: pairwise.py:60-77, 104-129) -
    every compare's two outputs, rankings and counters; allpair raises as in the reference."""
    from llmrankers.pairwise import PairwiseLlmRanker
    from llmrankers.rankers import SearchResult
    with open(os.path.join(GOLD, "llama_pairwise_cases.json")) as f:
        gold = json.load(f)
    ck = ckpt_dirs["ckpt_llama"]
    n = 0
    for case in gold["cases"]:
        rk = PairwiseLlmRanker(ck, ck, "cuda", method=case["method"], batch_size=2, k=case["k"])
        log, orig = [], rk.compare
        rk.compare = lambda q, d, _o=orig, _l=log: (_l.append([list(d)]), _l[-1].append(_o(q, d)))[1] or _l[-1][1]
        ranking = [SearchResult(docid=d, score=s, text=t) for d, s, t in case["input"]]
        if case["raises"]:
            with pytest.raises(AttributeError):
                rk.rerank(case["query"], ranking)
        else:
            res = rk.rerank(case["query"], ranking)
            assert log == case["compares"], case["method"]
            assert [[r.docid, r.score] for r in res] == case["result"]
            assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"]
            n += 1
        rk.llm.engine.close()
    assert n >= 4


def test_decoder_attention_per_sequence_kernel_bit_identical_to_per_row_kernel():
    """attn_dec_seq_kernel (one workgroup per (head, sequence), K / V of the head staged in LDS once, a wave per query row) walks
    the per-row kernel's chains and reduction trees: qlm scores (causal self-attention with the unidirectional bias + cross
    attention over the materialised K / V, 33 label positions) and greedy tokens / label logits after a multi-token prefix are the
    SAME BITS with either kernel, at flan-t5-small dims with ragged prompts - also prompts longer than 256 tokens (several keys
    per lane in the sums)."""
    from llmrankers import _synth
    dims = _synth.FLAN_T5_SMALL
    state = _synth.synth_state_dict(dims, seed=929, threads=8)
    eng = _engine(dims, state, max_tokens=8192, max_seqs=16, max_dec_len=40)
    labels = [0] + np.random.RandomState(5).randint(3, dims.vocab, size=32).tolist()
    prefix = [0] + np.random.RandomState(6).randint(3, dims.vocab, size=19).tolist()
    eng.set_option("dec_cross_mfma", 0)                  # (round 6: short sequences' cross-attention has a kernel of its own - next test)
    for seqs in (_synth.synth_token_batch(6, 40, 150, dims.vocab, seed=31), _synth.synth_token_batch(5, 200, 700, dims.vocab, seed=32),
                 _synth.synth_token_batch(1, 64, 64, dims.vocab, seed=33)):
        out = {}
        for flag in (1, 0):
            eng.set_option("dec_attn_seq", flag)
            out[flag] = (eng.qlm(seqs, labels), eng.score(seqs, prefix, [5, 6, 7, 8]))
        np.testing.assert_array_equal(out[1][0], out[0][0])
        np.testing.assert_array_equal(out[1][1], out[0][1])
    eng.set_option("dec_attn_seq", 1)
    eng.set_option("dec_cross_mfma", 1)
    eng.close()


def test_decoder_cross_attention_on_the_matrix_cores_vs_oracle_staged_kernels_and_batch_independence():
    """attn_dec_cross_mfma_kernel (round 6): the cross-attention of long decoder prefixes (qlm) for sequences of at most 192 keys
    on the matrix cores.  qlm scores and multi-token-prefix label logits (1) against the fp32 oracle at the suite's tolerances,
    (2) against the staged fma-chain kernels (option dec_cross_mfma = 0): equal to fp16 noise, (3) which kernel takes a sequence
    follows from ITS key count alone: in a batch that also holds prompts longer than 192 keys (those go to the staged kernel in
    the same call) every sequence has the bits it has alone or in any other batch, (4) 64 < positions: the staged kernels only."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims = _synth.FLAN_T5_SMALL
    state = _synth.synth_state_dict(dims, seed=929, threads=8)
    eng = _engine(dims, state, max_tokens=8192, max_seqs=16, max_dec_len=80)
    orc = T5Oracle(dims, state)
    labels = [0] + np.random.RandomState(5).randint(3, dims.vocab, size=32).tolist()     # 33 positions: two query tiles
    short = [0] + np.random.RandomState(7).randint(3, dims.vocab, size=18).tolist()      # 19 positions: one
    mixed = _synth.synth_token_batch(7, 20, 192, dims.vocab, seed=41) + _synth.synth_token_batch(2, 193, 400, dims.vocab, seed=42)
    only_short = mixed[:7]
    got = eng.qlm(mixed, labels)
    want = orc.qlm(mixed, labels)
    assert np.abs(got - want).max() < 5e-4 * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())
    got19 = eng.qlm(only_short, short)
    want19 = orc.qlm(only_short, short)
    assert np.abs(got19 - want19).max() < 5e-4 * np.abs(want19).max()
    np.testing.assert_array_equal(eng.qlm(only_short, labels), got[:7])                   # alone == beside longer prompts
    np.testing.assert_array_equal(eng.qlm(mixed[7:], labels), got[7:])
    for i in (0, 3, 8):
        np.testing.assert_array_equal(eng.qlm(mixed[i:i + 1], labels)[0], got[i])
    np.testing.assert_array_equal(eng.qlm(mixed[::-1], labels), got[::-1])
    lg = eng.score(only_short, short, [5, 6, 7, 8])
    assert np.abs(lg - orc.score_last(only_short, short, [5, 6, 7, 8])).max() < LOGIT_TOL
    eng.set_option("dec_cross_mfma", 0)
    staged = eng.qlm(mixed, labels)
    eng.set_option("dec_cross_mfma", 1)
    assert np.abs(got - staged).max() < 2e-4 * np.abs(staged).max(), np.abs(got - staged).max()   # (cross- AND self-attention differ in kernel)
    long_labels = [0] + np.random.RandomState(8).randint(3, dims.vocab, size=69).tolist()   # 70 positions > ATTX_MAXQ
    a = eng.qlm(only_short[:3], long_labels)
    eng.set_option("dec_cross_mfma", 0)
    np.testing.assert_array_equal(eng.qlm(only_short[:3], long_labels), a)
    eng.set_option("dec_cross_mfma", 1)
    eng.close()


def test_long_sequence_attention_kernel_vs_oracle_tiled_kernel_and_batch_independence():
    """attn_enc_long_kernel (round 5: sequences longer than 192 keys - the setwise prompts - by LDS-DMA in chunks of 128 keys,
    one online merge per chunk): logits against the fp32 oracle as close as the tiled kernel's, the two kernels within fp16
    noise of each other; the SAME BITS for every workgroup size (the host's free choice), for a sequence alone / among other
    long ones / in a batch with short sequences, and the short sequences of such a batch keep the short kernel's bits."""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims = _synth.FLAN_T5_SMALL
    state = _synth.synth_state_dict(dims, seed=929, threads=8)
    eng = _engine(dims, state, max_tokens=16384, max_seqs=32, max_dec_len=4)
    eng.set_option("dec_gemv", 0)      # (the subject is the ENCODER kernel: one decoder GEMM family for the one-prompt and the batched calls)
    seqs = _synth.synth_token_batch(3, 200, 900, dims.vocab, seed=41) + _synth.synth_token_batch(1, 385, 385, dims.vocab, seed=42) + \
        _synth.synth_token_batch(1, 193, 193, dims.vocab, seed=43) + _synth.synth_token_batch(1, 1300, 1300, dims.vocab, seed=45)
    ids = [5, 6, 7, 8]
    want = T5Oracle(dims, state).score_last(seqs, [0, 9], ids)
    eng.set_option("attn_long", 0)
    tiled = eng.score(seqs, [0, 9], ids)
    eng.set_option("attn_long", 1)
    got = {}
    for nw in (12, 6, 4, 3, 0):
        eng.set_option("attn_long_nw", nw)
        got[nw] = eng.score(seqs, [0, 9], ids)
    for nw in (6, 4, 3, 0):
        np.testing.assert_array_equal(got[12], got[nw], err_msg=f"{nw} waves per workgroup")
    eng.set_option("attn_long_xcd", 0)                              # workgroup -> XCD mapping: the same bits either way
    np.testing.assert_array_equal(eng.score(seqs, [0, 9], ids), got[0])
    eng.set_option("attn_long_xcd", 1)
    scale = np.abs(want).max()
    assert np.abs(got[0] - want).max() < 2e-3 * max(1.0, scale), (np.abs(got[0] - want).max(), scale)
    assert np.abs(got[0] - want).max() < 1.5 * np.abs(tiled - want).max() + 1e-4       # no further from fp32 than the tiled kernel
    assert np.abs(got[0] - tiled).max() < 4e-3 * max(1.0, scale)
    short = _synth.synth_token_batch(4, 30, 192, dims.vocab, seed=44)
    mixed = eng.score(short + seqs + short[:2], [0, 9], ids)
    for i, s_ in enumerate(seqs):
        np.testing.assert_array_equal(mixed[4 + i], eng.score([s_], [0, 9], ids)[0], err_msg=f"long sequence {i} ({len(s_)} tokens)")
    np.testing.assert_array_equal(mixed[4:4 + len(seqs)], got[0])
    eng.set_option("attn_long", 0)
    short_only = eng.score(short, [0, 9], ids)                      # all-short batch: the DMA kernel
    np.testing.assert_array_equal(mixed[:4], short_only)
    np.testing.assert_array_equal(mixed[4 + len(seqs):], short_only[:2])
    eng.set_option("attn_long", 1)
    eng.close()
