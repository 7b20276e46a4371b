"""DuoT5LlmRanker on the HIP engine (MI355X) against the fixtures recorded from the reference's DuoT5LlmRanker
(tools/make_duot5_golden.py): docid order and counters of every case, the margin floor, rerank_many and the fp16 host verdict."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, load_state
from llmrankers import _synth
from llmrankers.pairwise import DUO_PROMPT, DuoT5LlmRanker
from llmrankers.rankers import SearchResult

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "duot5_cases.json")) as _f:
    _GOLD = json.load(_f)
CASES = _GOLD["cases"]
IDS = [f"n{len(c['input'])}-k{c['k']}-len{c['model_max_length']}" for c in CASES]

# A compare's decision is the sign of (t0 - f0) - (t1 - f1): four logits enter one margin, so the engine (fp16 weights and
# activations) takes the fp32 reference's decision wherever the recorded margin is at least four times its per-logit error.
# ERR is that error as MEASURED on an MI355X: the largest |engine logit (rk_t5_compare) - fp32 oracle logit
# (oracle/t5_numpy.py)| over the four logits of all 273 compares of the golden cases came to 7.024e-3 (written up to 7.1e-3);
# test_logit_error_and_margin_floor prints the figure and holds the engine to it.  FLOOR = 4 * ERR = 2.84e-2.  The first set of
# cases, generated at margin >= 2e-2, measured 7.774e-3 -> 3.11e-2 > 2e-2, so the generator's rule was raised to 4e-2 and every
# case regenerated; the smallest recorded margin is now 0.0427.
ERR = 7.1e-3
FLOOR = 4 * ERR


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from transformers import T5Tokenizer
    from llmrankers._runtime import T5Runtime
    with open(os.path.join(GOLD, "duot5_ckpt.json")) as f:
        spec = json.load(f)["ckpt_duot5"]
    path = str(tmp_path_factory.mktemp("duot5") / "ckpt_duot5")
    _synth.write_checkpoint(path, spec, os.path.join(GOLD, "tok"))
    assert _synth.checkpoint_sha256(path) == spec["sha256"]
    rt = T5Runtime(path, "cuda", max_tokens=8192, max_seqs=64, max_dec_len=40)
    yield path, rt, T5Tokenizer.from_pretrained(path)
    rt.engine.close()


def make_ranker(stack, case, runtime=None, k=None):
    from transformers import T5Tokenizer
    path, rt, tok = stack
    if case["model_max_length"] is not None:
        tok = T5Tokenizer.from_pretrained(path)
        tok.model_max_length = case["model_max_length"]
    return DuoT5LlmRanker.from_runtime(runtime or rt, tok, method="heapsort", batch_size=2, k=case["k"] if k is None else k)


def ranking_of(case):
    return [SearchResult(docid=d, score=s, text=t) for d, s, t in case["input"]]


def counters(rk):
    return (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens)


def test_logit_error_and_margin_floor(stack):
    """the engine's four logits of every recorded compare against the fp32 oracle; every case's margins against FLOOR"""
    from _stub import OracleRuntime
    path, rt, _ = stack
    oracle = OracleRuntime(*load_state(path))
    assert rt.supports_compare_pairs
    err, ref_err = 0.0, 0.0
    for case in CASES:
        rk = make_ranker(stack, case)
        text = {d: t for d, _, t in case["input"]}
        ids = rk._pair_ids([case["query"]] * len(case["compares"]), [(text[c["pair"][0]], text[c["pair"][1]]) for c in case["compares"]])
        logits, p_true, wins = rt.compare_pairs(ids, 0, rk.FALSE_ID, rk.TRUE_ID)
        want = np.asarray(oracle.score(ids, [0], [rk.FALSE_ID, rk.TRUE_ID]), dtype=np.float64)
        err = max(err, float(np.abs(logits.astype(np.float64) - want).max()))
        recorded = np.asarray([row for c in case["compares"] for row in c["logits"]], dtype=np.float64)
        ref_err = max(ref_err, float(np.abs(want - recorded).max()))
        assert [bool(w) for w in wins] == [c["first_wins"] for c in case["compares"]]
    print(f"duoT5 logit error: engine vs fp32 oracle {err:.3e} (FLOOR would be {4 * err:.3e}); oracle vs the reference's recorded "
          f"logits {ref_err:.3e}; smallest recorded margin {min(c['min_margin'] for c in CASES):.4f}")
    assert 4 * err <= FLOOR, (err, FLOOR)
    for case, tag in zip(CASES, IDS):                               # no case is left out
        assert min(c["margin"] for c in case["compares"]) >= FLOOR, (tag, case["min_margin"], FLOOR)
    assert FLOOR <= _GOLD["min_margin_rule"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_golden_case(stack, case):
    rk = make_ranker(stack, case)
    assert rk._batched_ok() and getattr(rk.llm, "supports_compare_pairs", False)
    ranking = ranking_of(case)
    before = list(ranking)
    res = rk.rerank(case["query"], ranking)
    assert [r.docid for r in res] == [d for d, _ in case["result"]]
    assert [r.score for r in res] == [s for _, s in case["result"]]
    assert list(counters(rk)) == case["counters"]
    assert ranking == before


FIVE = [0, 2, 4, 5, 7]          # golden queries of 2, 3, 7, 12 and 20 candidates


@pytest.mark.parametrize("capacity", ["default", "max_seqs_6"])
def test_rerank_many_equals_rerank_one_by_one(stack, capacity):
    from llmrankers._runtime import T5Runtime
    path, _, _ = stack
    cases = [CASES[i] for i in FIVE]
    rt = T5Runtime(path, "cuda") if capacity == "default" else T5Runtime(path, "cuda", max_tokens=8192, max_seqs=6, max_dec_len=40)
    try:
        want = []
        for c in cases:
            rk = make_ranker(stack, c, runtime=rt, k=5)
            want.append(([(r.docid, r.score) for r in rk.rerank(c["query"], ranking_of(c))], counters(rk)))
        rk = make_ranker(stack, cases[0], runtime=rt, k=5)
        assert rk._can_alternate()
        calls = {"async": 0, "refused": 0, "blocking": 0}
        real_async, real_pairs = rt.compare_async, rt.compare_pairs

        def counted_async(*a):
            h = real_async(*a)
            calls["async" if h is not None else "refused"] += 1
            return h

        def counted_pairs(*a):
            calls["blocking"] += 1
            return real_pairs(*a)

        rt.compare_async, rt.compare_pairs = counted_async, counted_pairs
        items = [(c["query"], ranking_of(c)) for c in cases]
        results, cnts = rk.rerank_many(items)
        assert [([(r.docid, r.score) for r in res], c) for res, c in zip(results, cnts)] == want
        assert counters(rk) == cnts[-1]
        print(f"rerank_many ({capacity}): {calls}")
        if capacity == "default":
            assert calls["async"] > 10 and calls["refused"] == 0 and calls["blocking"] == 0
        else:
            assert calls["refused"] == calls["blocking"] > 0 and calls["async"] > 0      # rounds that did not fit one call of 6 sequences
    finally:
        rt.engine.close()


def test_fp16_scores_takes_the_host_verdict_from_the_same_logits(stack):
    from llmrankers.pointwise import _softmax_first
    path, rt, _ = stack
    case = CASES[5]
    rk = make_ranker(stack, case)
    rk.fp16_scores = True
    seen, real = [], rt.compare_pairs

    def capture(*a):
        out = real(*a)
        seen.append(out)
        return out

    verdicts, orig = [], rk._compare_pairs

    def logged(queries, pairs):
        v, p = orig(queries, pairs)
        verdicts.extend(v)
        return v, p

    rt.compare_pairs, rk._compare_pairs = capture, logged
    try:
        rk.rerank(case["query"], ranking_of(case))
    finally:
        del rt.compare_pairs
    logits = np.concatenate([s[0] for s in seen], axis=0)
    device = np.concatenate([s[2] for s in seen], axis=0)
    p16 = _softmax_first(logits[:, 1], logits[:, 0], fp16=True)
    assert len(verdicts) == len(device) == rk.total_compare > 0
    assert verdicts == [bool(a > b) for a, b in zip(p16[0::2], p16[1::2])]


def test_prompt_is_the_reference_s():
    assert DUO_PROMPT == 'Query: {query} Document0: {doc1} Document1: {doc2} Relevant:'
