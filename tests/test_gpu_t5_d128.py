"""T5 checkpoints with 128-wide heads (t5-3b: monoT5-3B, duoT5-3B) on the HIP engine (MI355X): creation and refusals, the rankers
against the fixtures recorded from the reference's MonoT5LlmRanker and DuoT5LlmRanker on the toy d128 checkpoint
(tools/make_d128_golden.py), batch independence bit for bit, and the real widths (I = 4096, F = 16384) on a one-layer model against
the fp32 oracle with the unchanged 64-wide path as the yardstick."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, load_state
from llmrankers import _synth
from llmrankers._engine import RkEngine, RkError
from llmrankers.rankers import SearchResult

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-3                 # the project's bound on a pointwise score (tests/test_gpu_kernels.py)
ERR_INVALID, ERR_STATE = -1, -4
with open(os.path.join(GOLD, "d128_cases.json")) as _f:
    _GOLD = json.load(_f)
MONO, DUO = _GOLD["monot5"], _GOLD["duot5"]
DUO_IDS = [f"n{len(c['input'])}-k{c['k']}-len{c['model_max_length']}" for c in DUO]

# A compare's decision is the sign of (t0 - f0) - (t1 - f1): four logits enter one margin, so the engine takes the fp32
# reference's decision wherever the recorded margin is at least four times its per-logit error (tests/test_gpu_duot5.py).
# ERR is that error as MEASURED on an MI355X over the four logits of all 246 compares of the d128 golden cases (engine
# rk_t5_compare against the fp32 oracle), rounded up; test_duot5_logit_error_and_margin_floor prints the figure and holds the
# engine to it: 6.350e-3, written up to 6.4e-3; FLOOR = 2.56e-2, below the generator's rule (4e-2, tools/make_duot5_golden.py's, which
# did not have to be raised; the smallest recorded margin is 0.0418).
ERR = 6.4e-3
FLOOR = 4 * ERR


def _ckpt(tmp_path_factory, name):
    with open(os.path.join(GOLD, "d128_ckpts.json")) as f:
        spec = json.load(f)[name]
    path = str(tmp_path_factory.mktemp("d128") / name)
    _synth.write_checkpoint(path, spec, os.path.join(GOLD, "tok"))
    assert _synth.checkpoint_sha256(path) == spec["sha256"], f"{name}: regenerated weights differ from the recorded recipe"
    return path


@pytest.fixture(scope="module")
def mono(tmp_path_factory):
    from transformers import T5Tokenizer
    from llmrankers._runtime import T5Runtime
    path = _ckpt(tmp_path_factory, "ckpt_monot5_d128")
    rt = T5Runtime(path, "cuda", max_tokens=8192, max_seqs=64, max_dec_len=40)
    yield path, rt, T5Tokenizer.from_pretrained(path)
    rt.engine.close()


@pytest.fixture(scope="module")
def duo(tmp_path_factory):
    from transformers import T5Tokenizer
    from llmrankers._runtime import T5Runtime
    path = _ckpt(tmp_path_factory, "ckpt_duot5_d128")
    rt = T5Runtime(path, "cuda", max_tokens=8192, max_seqs=64, max_dec_len=40)
    yield path, rt, T5Tokenizer.from_pretrained(path)
    rt.engine.close()


def ranking_of(case):
    return [SearchResult(docid=d, score=s, text=t) for d, s, t in case["input"]]


def counters(rk):
    return (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens)


def _launches(eng):
    return sum(v["launches"] for v in eng.profile_report().values())


# ---- create and refuse -------------------------------------------------------------------------------------------------------
def test_create_accepts_128_and_refuses_96():
    import dataclasses
    dims = _synth.TOY_MONOT5_D128
    assert dims.d_kv == 128 and _synth.NAMED_DIMS["toy-monot5-d128"] is dims and _synth.NAMED_DIMS["t5-3b"].d_kv == 128
    e = RkEngine(dims, device=0, max_tokens=512, max_seqs=8, max_dec_len=8)
    e.close()
    with pytest.raises(RkError) as ei:
        RkEngine(dataclasses.replace(dims, d_kv=96, n_heads=4), device=0, max_tokens=512, max_seqs=8, max_dec_len=8)
    assert ei.value.code == ERR_INVALID and "d_kv=96" in str(ei.value) and "128" in str(ei.value)


def test_out_of_scope_entry_points_launch_nothing(mono):
    _, rt, _ = mono
    eng = rt.engine
    seqs = _synth.synth_token_batch(3, 5, 40, rt.dims.vocab, seed=3)
    eng.score(seqs, [0], [6136, 1176])                       # (the one-off attribute calls of the first launch are behind us)
    eng.profile(True)
    try:
        eng.profile_reset()
        calls = {
            "rk_t5_score": lambda: eng.score(seqs, [0, 5], [6136, 1176]),
            "rk_t5_qlm": lambda: eng.qlm(seqs, [5, 6, 7]),
            "rk_t5_qlm_many": lambda: eng.qlm_many(seqs, [[5, 6], [7], [8, 9, 10]]),
            "rk_t5_greedy": lambda: eng.greedy(seqs, [0], 2),
            "rk_t5_greedy2": lambda: eng.greedy(seqs, [0, 5], 2, candidates=[7, 8]),
            "rk_t5_generate": lambda: eng.generate(seqs, [0], 4),
        }
        for entry, call in calls.items():
            with pytest.raises(RkError) as ei:
                call()
            assert ei.value.code == ERR_STATE and "d_kv=128" in str(ei.value) and entry in str(ei.value), (entry, str(ei.value))
        for key, bad in (("xattn_direct", 0), ("dec_fuse", 2)):
            eng.set_option(key, bad)
            try:
                for call in (lambda: eng.score(seqs, [0], [6136, 1176]), lambda: eng.compare_pairs(seqs[:2], 0, 6136, 1176)):
                    with pytest.raises(RkError) as ei:
                        call()
                    assert ei.value.code == ERR_STATE and "d_kv=128" in str(ei.value) and key in str(ei.value)
            finally:
                eng.set_option(key, 1)
        assert _launches(eng) == 0, eng.profile_report()
        assert eng.score(seqs, [0], [6136, 1176]).shape == (3, 2)       # and the engine still serves
        assert _launches(eng) > 0
    finally:
        eng.profile(False)


def test_runtime_and_rankers_refuse_what_needs_more_positions(mono):
    from llmrankers.listwise import ListwiseLlmRanker
    from llmrankers.pairwise import DuoT5LlmRanker, PairwiseLlmRanker
    from llmrankers.pointwise import MonoT5LlmRanker, PointwiseLlmRanker
    from llmrankers.setwise import SetwiseLlmRanker
    _, rt, tok = mono
    assert rt.one_position_only
    seqs = _synth.synth_token_batch(2, 5, 20, rt.dims.vocab, seed=4)
    for call in (lambda: rt.qlm(seqs, [5, 6]), lambda: rt.qlm_many(seqs, [[5], [6, 7]]), lambda: rt.greedy(seqs, [0], 2),
                 lambda: rt.generate(seqs, [0], 3), lambda: rt.score(seqs, [0, 5], [6136])):
        with pytest.raises(NotImplementedError, match="d_kv=128"):
            call()
    for build in (lambda: PointwiseLlmRanker.from_runtime(rt, tok, method="qlm"), lambda: SetwiseLlmRanker.from_runtime(rt, tok),
                  lambda: ListwiseLlmRanker.from_runtime(rt, tok), lambda: PairwiseLlmRanker.from_runtime(rt, tok)):
        with pytest.raises(NotImplementedError, match="d_kv=128"):
            build()
    MonoT5LlmRanker.from_runtime(rt, tok)
    PointwiseLlmRanker.from_runtime(rt, tok, method="yes_no")
    DuoT5LlmRanker.from_runtime(rt, tok, method="heapsort")


# ---- golden cases, monoT5 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MONO, ids=[f"n{len(c['input'])}-bs{c['batch_size']}" for c in MONO])
def test_monot5_golden_case(mono, case):
    from llmrankers.pointwise import MonoT5LlmRanker
    _, rt, tok = mono
    rk = MonoT5LlmRanker.from_runtime(rt, tok, method="yes_no", batch_size=case["batch_size"])
    res = rk.rerank(case["query"], ranking_of(case))
    want = dict((d, s) for d, s in case["result"])
    got, ref = np.array([r.score for r in res]), np.array([want[r.docid] for r in res])
    print(f"monoT5 d128 n={len(res)}: largest |score - reference| {np.abs(got - ref).max():.3e}, smallest reference gap {case['min_gap']:.4f}")
    assert np.abs(got - ref).max() < SCORE_TOL, np.abs(got - ref).max()
    assert case["min_gap"] >= _GOLD["mono_min_gap_rule"] >= 4 * SCORE_TOL
    assert [r.docid for r in res] == [d for d, _ in case["result"]]                   # every case: none left out
    assert list(counters(rk)) == case["counters"]


def test_monot5_rerank_many_and_yes_no(mono):
    from llmrankers.pointwise import MonoT5LlmRanker, PointwiseLlmRanker
    _, rt, tok = mono
    for cls, kw in ((MonoT5LlmRanker, dict(method="yes_no", batch_size=4)), (PointwiseLlmRanker, dict(method="yes_no", batch_size=32))):
        want = []
        for c in MONO:
            rk = cls.from_runtime(rt, tok, **kw)
            want.append(([(r.docid, r.score) for r in rk.rerank(c["query"], ranking_of(c))], counters(rk)))
        rk = cls.from_runtime(rt, tok, **kw)
        results, cnts = rk.rerank_many([(c["query"], ranking_of(c)) for c in MONO])
        assert [([(r.docid, r.score) for r in res], tuple(c)) for res, c in zip(results, cnts)] == want, cls.__name__


# ---- golden cases, duoT5 -----------------------------------------------------------------------------------------------------
def make_duo(duo, case, k=None):
    from transformers import T5Tokenizer
    from llmrankers.pairwise import DuoT5LlmRanker
    path, rt, tok = duo
    if case["model_max_length"] is not None:
        tok = T5Tokenizer.from_pretrained(path)
        tok.model_max_length = case["model_max_length"]
    return DuoT5LlmRanker.from_runtime(rt, tok, method="heapsort", batch_size=2, k=case["k"] if k is None else k)


def test_duot5_logit_error_and_margin_floor(duo):
    """the engine's four logits of every recorded compare against the fp32 oracle; every case's margins against FLOOR"""
    from _stub import OracleRuntime
    path, rt, _ = duo
    oracle = OracleRuntime(*load_state(path))
    err, ref_err = 0.0, 0.0
    for case in DUO:
        rk = make_duo(duo, case)
        text = {d: t for d, _, t in case["input"]}
        ids = rk._pair_ids([case["query"]] * len(case["compares"]), [(text[c["pair"][0]], text[c["pair"][1]]) for c in case["compares"]])
        logits, p_true, wins = rt.compare_pairs(ids, 0, rk.FALSE_ID, rk.TRUE_ID)
        want = np.asarray(oracle.score(ids, [0], [rk.FALSE_ID, rk.TRUE_ID]), dtype=np.float64)
        err = max(err, float(np.abs(logits.astype(np.float64) - want).max()))
        recorded = np.asarray([row for c in case["compares"] for row in c["logits"]], dtype=np.float64)
        ref_err = max(ref_err, float(np.abs(want - recorded).max()))
        assert [bool(w) for w in wins] == [c["first_wins"] for c in case["compares"]]
    print(f"duoT5 d128 logit error: engine vs fp32 oracle {err:.3e} (FLOOR would be {4 * err:.3e}); oracle vs the reference's recorded "
          f"logits {ref_err:.3e}; smallest recorded margin {min(c['min_margin'] for c in DUO):.4f}")
    assert 4 * err <= FLOOR, (err, FLOOR)
    for case, tag in zip(DUO, DUO_IDS):                               # no case is left out
        assert min(c["margin"] for c in case["compares"]) >= FLOOR, (tag, case["min_margin"], FLOOR)
    assert FLOOR <= _GOLD["min_margin_rule"]


@pytest.mark.parametrize("case", DUO, ids=DUO_IDS)
def test_duot5_golden_case(duo, case):
    rk = make_duo(duo, case)
    assert rk._batched_ok() and getattr(rk.llm, "supports_compare_pairs", False)
    ranking = ranking_of(case)
    before = list(ranking)
    res = rk.rerank(case["query"], ranking)
    assert [r.docid for r in res] == [d for d, _ in case["result"]]
    assert [r.score for r in res] == [s for _, s in case["result"]]
    assert list(counters(rk)) == case["counters"]
    assert ranking == before


def test_duot5_rerank_many_equals_rerank_one_by_one(duo):
    cases = [DUO[i] for i in (0, 2, 4, 5, 7)]
    want = []
    for c in cases:
        rk = make_duo(duo, c, k=5)
        want.append(([(r.docid, r.score) for r in rk.rerank(c["query"], ranking_of(c))], counters(rk)))
    rk = make_duo(duo, cases[0], k=5)
    results, cnts = rk.rerank_many([(c["query"], ranking_of(c)) for c in cases])
    assert [([(r.docid, r.score) for r in res], c) for res, c in zip(results, cnts)] == want


# ---- batch independence, bit for bit -----------------------------------------------------------------------------------------
def test_a_sequence_s_logits_do_not_depend_on_the_batch(mono):
    _, rt, _ = mono
    eng = rt.engine
    seqs = [_synth.synth_token_batch(1, n, n, rt.dims.vocab, seed=40 + i)[0] for i, n in enumerate((1, 64, 65, 200, 33, 129, 7))]
    out_ids = [6136, 1176, 10]
    whole = eng.score(seqs, [0], out_ids)
    for b, s in enumerate(seqs):
        assert eng.score([s], [0], out_ids).tobytes() == whole[b:b + 1].tobytes(), f"sequence {b} alone gives other logits than in the batch of 7"
    order = [3, 0, 6, 2, 5, 1, 4]
    assert eng.score([seqs[i] for i in order], [0], out_ids).tobytes() == whole[order].tobytes(), "the order of the batch changes a sequence's logits"
    # blocking == staged, on both pipelined slots
    eng.stage(seqs[:4], slot=0)
    eng.score_staged([0], out_ids, slot=0)
    eng.stage(seqs[4:], slot=1)
    eng.score_staged([0], out_ids, slot=1)
    assert np.concatenate([eng.read_scores(0), eng.read_scores(1)]).tobytes() == whole.tobytes()
    # the compare's logits are rk_t5_score's, whatever shares the call
    pairs = seqs[:6]
    logits, p_true, wins = eng.compare_pairs(pairs, 0, 6136, 1176)
    assert logits.tobytes() == whole[:6, :2].tobytes()
    eng.stage(pairs[2:4], slot=1)
    eng.compare_staged(0, 6136, 1176, slot=1)
    l1, p1, w1 = eng.read_scores(1)
    assert l1.tobytes() == logits[2:4].tobytes() and p1.tobytes() == p_true[2:4].tobytes() and list(w1) == list(wins[1:2])


# ---- the real widths, one layer deep -----------------------------------------------------------------------------------------
WIDE = _synth.T5Dims(vocab=6144, d_model=1024, n_heads=32, d_kv=128, d_ff=16384, n_enc=1, n_dec=1, gated=False, tied_head=True)
TWIN = _synth.T5Dims(vocab=6144, d_model=1024, n_heads=64, d_kv=64, d_ff=16384, n_enc=1, n_dec=1, gated=False, tied_head=True)


def test_real_widths_against_the_64_wide_path():
    """I = 4096, F = 16384 (t5-3b's projections: the weight-streaming family at K = 16384, the few-row lines, the ping-pong kernel's K
    split at N = 1024, K = 16384).  The yardstick is the EXISTING path: the twin model with 64 heads of 64 (the same I, F, widths,
    inputs and weights' distribution) through the unchanged 64-wide kernels gives the largest logit error E64 against the fp32
    oracle; the 128-wide model must stay within 2 E64 (a 128-term dot product may carry up to twice the rounding error of a
    64-term one).  Every sub-batch must also give the bytes it has inside the batch of 32: the first MI355X run of this test
    failed exactly there, on the 64-wide twin (2 sequences alone: other logits, |logit - oracle| 1.02e-3) - the ping-pong GEMM's K
    split, decided from the tile count, took the FFN-out of the large call and not of the small one; T5 engines are off that rule
    since (choose_ksplit)."""
    from oracle.t5_numpy import T5Oracle
    seqs = _synth.synth_token_batch(32, 5, 200, WIDE.vocab, seed=77)
    out_ids = [int(x) for x in np.random.RandomState(5).choice(np.arange(3, WIDE.vocab), size=64, replace=False)]
    errs = {}
    for name, dims in (("d_kv=64 x 64 heads", TWIN), ("d_kv=128 x 32 heads", WIDE)):
        state = _synth.synth_state_dict(dims, seed=31, gain=1.0)
        want = T5Oracle(dims, state).score_last(seqs, [0], out_ids)
        eng = RkEngine(dims, device=0, max_tokens=4096, max_seqs=32, max_dec_len=4).load_state(state.items())
        try:
            got = eng.score(seqs, [0], out_ids)
            errs[name] = float(np.abs(got - want).max())
            for n in (2, 1):                               # the few-row and K-split lines: the same logits as in the batch of 32?
                few = eng.score(seqs[:n], [0], out_ids)
                e_few = float(np.abs(few - want[:n]).max())
                print(f"{name}: {n} sequence(s) alone: largest |logit - oracle| {e_few:.3e}")
                errs[name] = max(errs[name], e_few)
                assert few.tobytes() == got[:n].tobytes(), f"{name}: {n} sequence(s) alone give other logits than inside the batch of 32"
        finally:
            eng.close()
        print(f"{name}: largest |logit - fp32 oracle| over 32 sequences x 64 ids = {errs[name]:.3e}")
    e64, e128 = errs["d_kv=64 x 64 heads"], errs["d_kv=128 x 32 heads"]
    print(f"E128 / E64 = {e128 / e64:.2f}")
    assert e128 <= 2 * e64, (e128, e64)
