"""DuoT5LlmRanker (ref: llmrankers/pairwise.py:296-352) on the fp32 numpy oracle - CPU only: ranking, counters, compare order,
level batching, truncation, rerank_many (alternating, plain and fallback paths), the command line and the defaults, against the
fixtures tools/make_duot5_golden.py recorded from the reference."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLD, REPO, load_state
from _stub import OracleRuntime
from llmrankers import _synth
from llmrankers._batching import default_queries_per_call
from llmrankers.pairwise import DuoT5LlmRanker, PairwiseLlmRanker
from llmrankers.rankers import SearchResult

with open(os.path.join(GOLD, "duot5_cases.json")) as _f:
    CASES = json.load(_f)["cases"]
IDS = [f"n{len(c['input'])}-k{c['k']}-len{c['model_max_length']}" for c in CASES]


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from transformers import T5Tokenizer
    with open(os.path.join(GOLD, "duot5_ckpt.json")) as f:
        spec = json.load(f)["ckpt_duot5"]
    path = str(tmp_path_factory.mktemp("duot5") / "ckpt_duot5")
    _synth.write_checkpoint(path, spec, os.path.join(GOLD, "tok"))
    assert _synth.checkpoint_sha256(path) == spec["sha256"], "regenerated duoT5 fixture weights differ from the recipe's"
    dims, state = load_state(path)
    return path, OracleRuntime(dims, state), T5Tokenizer.from_pretrained(path)


def make_ranker(stack, case, runtime=None, method=None):
    from transformers import T5Tokenizer
    path, rt, tok = stack
    if case["model_max_length"] is not None:               # a tokenizer of its own: the limit is an attribute of the object
        tok = T5Tokenizer.from_pretrained(path)
        tok.model_max_length = case["model_max_length"]
    return DuoT5LlmRanker.from_runtime(runtime or rt, tok, method=method or case["method"], batch_size=2, k=case["k"])


def ranking_of(case):
    return [SearchResult(docid=d, score=s, text=t) for d, s, t in case["input"]]


def logged(rk):
    """Every engine-side compare of the ranker as (docid pair, verdict), whichever path asked for it."""
    log, orig = [], rk._compare_pairs

    def wrapped(queries, pairs):
        verdicts, ptok = orig(queries, pairs)
        log.extend((tuple(p), v) for p, v in zip(pairs, verdicts))
        return verdicts, ptok

    rk._compare_pairs = wrapped
    return log


def counters(rk):
    return [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens]


def test_class_surface():
    assert issubclass(DuoT5LlmRanker, PairwiseLlmRanker)
    assert (DuoT5LlmRanker.FALSE_ID, DuoT5LlmRanker.TRUE_ID) == (6136, 1176) and DuoT5LlmRanker.fp16_scores is False
    assert len(CASES) >= 8 and any(c["k"] > len(c["input"]) for c in CASES) and any(c["model_max_length"] for c in CASES)
    assert {len(c["input"]) for c in CASES} <= {2, 3, 7, 12, 20} and {c["k"] for c in CASES} <= {1, 5, 10}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_golden_case_reference_order(stack, case):
    """level batching off: the reference's ranking, counters and compare sequence, pair for pair; the caller's list untouched"""
    rk = make_ranker(stack, case)
    rk.batch_independent_compares = False
    log = logged(rk)
    ranking = ranking_of(case)
    before = list(ranking)
    res = rk.rerank(case["query"], ranking)
    assert [[r.docid, r.score] for r in res] == case["result"]
    assert counters(rk) == case["counters"] and rk.total_completion_tokens == 0
    assert ranking == before and [r.docid for r in ranking] == case["caller_list_after"]
    text = {d: t for d, _, t in case["input"]}
    assert [(p, v) for p, v in log] == [((text[c["pair"][0]], text[c["pair"][1]]), c["first_wins"]) for c in case["compares"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_golden_case_level_batched(stack, case):
    """level batching on (the default): the same SET of compares, every counter and the ranking"""
    rk = make_ranker(stack, case)
    assert rk._batched_ok()
    log = logged(rk)
    ranking = ranking_of(case)
    before = list(ranking)
    res = rk.rerank(case["query"], ranking)
    assert [[r.docid, r.score] for r in res] == case["result"]
    assert counters(rk) == case["counters"]
    assert ranking == before
    text = {d: t for d, _, t in case["input"]}
    want = sorted(((text[c["pair"][0]], text[c["pair"][1]]), c["first_wins"]) for c in case["compares"])
    assert sorted(log) == want


def test_replaced_compare_gets_the_reference_order(stack):
    case = next(c for c in CASES if len(c["input"]) == 12 and c["model_max_length"] is None)
    rk = make_ranker(stack, case)
    seen, orig = [], rk.compare
    rk.compare = lambda q, docs: (seen.append(tuple(docs)), orig(q, docs))[1]
    assert not rk._batched_ok()
    res = rk.rerank(case["query"], ranking_of(case))
    text = {d: t for d, _, t in case["input"]}
    assert seen == [(text[c["pair"][0]], text[c["pair"][1]]) for c in case["compares"]]
    assert [[r.docid, r.score] for r in res] == case["result"] and counters(rk) == case["counters"]


def test_truncation_rule(stack):
    """tokenizer(inputs, truncation=True): cut to model_max_length with the EOS kept; HF's "no limit" value cuts nothing -
    against the installed transformers itself"""
    from transformers import T5Tokenizer
    path, _, tok = stack
    case = next(c for c in CASES if c["model_max_length"] is not None)
    assert case["prompts_cut"] > 0
    rk = make_ranker(stack, case)
    limit = case["model_max_length"]
    pairs = [(case["input"][0][2], case["input"][1][2]), (case["input"][2][2], case["input"][3][2])]
    ids = rk._pair_ids([case["query"]] * 2, pairs)
    texts = [t for a, b in pairs for t in (f"Query: {case['query']} Document0: {a} Document1: {b} Relevant:",
                                           f"Query: {case['query']} Document0: {b} Document1: {a} Relevant:")]
    hf = T5Tokenizer.from_pretrained(path)
    hf.model_max_length = limit
    assert ids == [list(x) for x in hf(texts, truncation=True)["input_ids"]]
    assert all(len(x) <= limit and x[-1] == hf.eos_token_id for x in ids) and any(len(x) == limit for x in ids)
    free = DuoT5LlmRanker.from_runtime(stack[1], tok, method="heapsort", k=5)      # the fixture tokenizer carries "no limit"
    assert tok.model_max_length > 1e20
    full = free._pair_ids([case["query"]] * 2, pairs)
    assert full == [list(x) for x in tok(texts, truncation=True)["input_ids"]] and max(map(len, full)) > limit


def test_other_methods_raise_after_resetting_the_counters(stack):
    rk = make_ranker(stack, CASES[0], method="allpair")
    rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens = 5, 6, 7
    with pytest.raises(NotImplementedError, match="Method allpair is not implemented."):
        rk.rerank(CASES[0]["query"], ranking_of(CASES[0]))
    assert counters(rk) == [0, 0, 0]


def test_non_t5_runtime_is_refused(stack):
    class Llama:
        model_type = "llama"
    with pytest.raises(NotImplementedError):
        DuoT5LlmRanker.from_runtime(Llama(), stack[2])


class SlotRuntime:
    """The oracle behind T5Runtime's compare interface: compare_pairs, and compare_async / compare_collect over two slots
    (evaluated at collect time; a slot must be collected before it is launched on again)."""
    model_type, decoder_start_token_id, supports_compare_pairs = "t5", 0, True

    def __init__(self, rt, slots=2, fits=lambda seqs: True):
        from types import SimpleNamespace
        self.rt, self.config, self.fits = rt, rt.config, fits
        self.engine = SimpleNamespace(num_slots=slots)
        self.busy, self.calls = {}, {"pairs": 0, "async": 0, "refused": 0}

    def compare_pairs(self, seqs, dec_start, false_id, true_id):
        assert not self.busy, "a blocking call while a slot is in flight"
        self.calls["pairs"] += 1
        return self._compute(seqs, dec_start, false_id, true_id)

    def _compute(self, seqs, dec_start, false_id, true_id):
        assert len(seqs) % 2 == 0
        lg = np.asarray(self.rt.score(seqs, [dec_start], [false_id, true_id]), dtype=np.float32)
        m = lg.max(axis=1)
        p = np.exp(lg[:, 1] - m) / (np.exp(lg[:, 0] - m) + np.exp(lg[:, 1] - m))
        return lg, p, p[0::2] > p[1::2]

    def compare_async(self, seqs, dec_start, false_id, true_id, slot):
        if not self.fits(seqs):
            self.calls["refused"] += 1
            return None
        assert slot not in self.busy and slot < self.engine.num_slots
        self.calls["async"] += 1
        self.busy[slot] = (list(seqs), dec_start, false_id, true_id)
        return slot

    def compare_collect(self, handle):
        return self._compute(*self.busy.pop(handle))


FIVE = [0, 2, 4, 5, 7]          # golden queries of 2, 3, 7, 12 and 20 candidates (k = 5 for all of them below)


def one_by_one(stack, runtime, cases):
    out = []
    for c in cases:
        rk = make_ranker(stack, c, runtime=runtime)
        rk.k = 5
        out.append(([(r.docid, r.score) for r in rk.rerank(c["query"], ranking_of(c))], tuple(counters(rk))))
    return out


@pytest.mark.parametrize("kind", ["alternating", "no_async", "async_refuses", "refuses_later"])
def test_rerank_many_equals_rerank_one_by_one(stack, kind):
    cases = [CASES[i] for i in FIVE]
    assert sorted(len(c["input"]) for c in cases) == [2, 3, 7, 12, 20]
    want = one_by_one(stack, stack[1], cases)
    if kind == "no_async":
        runtime = stack[1]                                             # OracleRuntime: score() only, no slots
    else:
        seen = []
        fits = {"alternating": lambda seqs: True, "async_refuses": lambda seqs: False,
                "refuses_later": lambda seqs: (seen.append(1), len(seen) % 3 != 0)[1]}[kind]        # every third launch
        runtime = SlotRuntime(stack[1], fits=fits)
    rk = make_ranker(stack, cases[0], runtime=runtime)
    rk.k = 5
    items = [(c["query"], ranking_of(c)) for c in cases]
    before = [list(r) for _, r in items]
    results, cnts = rk.rerank_many(items)
    assert [([(r.docid, r.score) for r in res], c) for res, c in zip(results, cnts)] == want
    assert [r for _, r in items] == before                             # the callers' lists are left as they were
    assert tuple(counters(rk)) == cnts[-1]
    if kind == "alternating":
        assert runtime.calls["async"] > 10 and runtime.calls["pairs"] == 0 and not runtime.busy
    elif kind == "async_refuses":
        assert runtime.calls["async"] == 0 and runtime.calls["refused"] == runtime.calls["pairs"] > 10
    elif kind == "refuses_later":                                      # the rounds after a refused one are launched again
        assert runtime.calls["refused"] == runtime.calls["pairs"] > 3 and runtime.calls["async"] >= 2 * runtime.calls["pairs"] - 2
        assert not runtime.busy


def test_rerank_many_small_inputs_and_replaced_compare(stack):
    c = CASES[4]
    rk = make_ranker(stack, c)
    res, cnts = rk.rerank_many([(c["query"], ranking_of(c))])
    assert [[r.docid, r.score] for r in res[0]] == c["result"] and list(cnts[0]) == c["counters"]
    assert rk.rerank_many([]) == ([], [])
    seen, orig = [], rk.compare
    rk.compare = lambda q, docs: (seen.append(1), orig(q, docs))[1]
    res, cnts = rk.rerank_many([(c["query"], ranking_of(c))] * 2)
    assert len(seen) == 2 * c["counters"][0] and [list(x) for x in cnts] == [c["counters"]] * 2


def test_device_verdict_and_fp16_host_verdict(stack):
    """a runtime with compare_pairs: its verdict is used as it is; fp16_scores = True recomputes it from the logits"""
    from llmrankers.pointwise import _softmax_first
    c = CASES[3]
    flipped = SlotRuntime(stack[1])
    real = flipped._compute
    flipped.compare_pairs = lambda *a: (lambda lg, p, w: (lg, p, ~w))(*real(*a))
    rk = make_ranker(stack, c, runtime=flipped)
    a, b = c["input"][0][2], c["input"][1][2]
    want = c["compares"][0]["first_wins"] if c["compares"][0]["pair"] == [c["input"][0][0], c["input"][1][0]] else None
    lg = real(rk._pair_ids([c["query"]], [(a, b)]), 0, 6136, 1176)[0]
    host = _softmax_first(lg[:, 1], lg[:, 0], False)
    assert rk.compare(c["query"], [a, b]) == (not host[0] > host[1])      # the (flipped) device verdict
    if want is not None:
        assert bool(host[0] > host[1]) == want
    rk.fp16_scores = True
    h16 = _softmax_first(lg[:, 1], lg[:, 0], True)
    assert rk.compare(c["query"], [a, b]) == bool(h16[0] > h16[1])


def test_run_py_builds_duot5_for_a_duot5_name(monkeypatch):
    spec = importlib.util.spec_from_file_location("rk_run_duot5", os.path.join(REPO, "run.py"))
    runmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(runmod)
    import llmrankers.pairwise as pw
    built = []

    class Fake:
        def __init__(self, **kw):
            built.append((type(self).__name__, kw))

    monkeypatch.setattr(pw, "DuoT5LlmRanker", type("FakeDuo", (Fake,), {}))
    monkeypatch.setattr(pw, "PairwiseLlmRanker", type("FakePrp", (Fake,), {}))
    parser, commands = runmod.build_parser()
    for name, cls in (("castorini/duot5-base-msmarco", "FakeDuo"), ("google/flan-t5-large", "FakePrp")):
        args = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", name, "--run_path", "r", "--save_path", "s",
                                                    "pairwise", "--method", "heapsort", "--k", "7", "--batch_size", "9"])
        runmod.validate(args)
        runmod.build_ranker(args)
        got, kw = built[-1]
        assert got == cls and kw["method"] == "heapsort" and kw["k"] == 7 and kw["batch_size"] == 2 and kw["model_name_or_path"] == name
    args = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "x/duot5", "--openai_key", "k", "pairwise"])
    with pytest.raises(NotImplementedError):
        runmod.build_ranker(args)


def test_run_py_ranks_with_duot5_through_file_sources(stack, tmp_path, monkeypatch):
    """`run.py run ... pairwise --method heapsort` on the fixture checkpoint (oracle runtime): it ranks, in rerank_many groups"""
    spec = importlib.util.spec_from_file_location("rk_run_duot5b", os.path.join(REPO, "run.py"))
    runmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(runmod)
    path, rt, tok = stack
    monkeypatch.setattr(runmod, "build_ranker", lambda args: DuoT5LlmRanker.from_runtime(rt, tok, method=args.pairwise.method, k=args.pairwise.k))
    case = CASES[3]
    qs = {"q1": case["query"], "q2": CASES[4]["query"]}
    (tmp_path / "q.tsv").write_text("".join(f"{q}\t{t}\n" for q, t in qs.items()))
    (tmp_path / "d.jsonl").write_text("".join(json.dumps({"docid": d, "text": t}) + "\n" for d, _, t in case["input"]))
    (tmp_path / "in.trec").write_text("".join(f"{q} Q0 {d} {r + 1} {s} bm25\n" for q in qs for r, (d, s, _) in enumerate(case["input"])))
    parser, commands = runmod.build_parser()
    args = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "duot5-fixture", "--run_path", str(tmp_path / "in.trec"),
                                                "--save_path", str(tmp_path / "out.trec"), "--query_file", str(tmp_path / "q.tsv"),
                                                "--doc_file", str(tmp_path / "d.jsonl"), "--hits", "7", "--query_length", "64",
                                                "--passage_length", "128", "pairwise", "--method", "heapsort", "--k", str(case["k"])])
    runmod.validate(args)
    runmod.main(args)
    out = [l.split("\t") for l in (tmp_path / "out.trec").read_text().splitlines()]
    assert [l[2] for l in out if l[0] == "q1"] == [d for d, _ in case["result"]]
    assert len([l for l in out if l[0] == "q2"]) == 7


def test_default_queries_per_call():
    assert default_queries_per_call("duot5", 100) > 1 and default_queries_per_call("pairwise", 100) == 1
    # one alternating group (half the queries, one pair each) at 512-token prompts fits one call of T5Runtime's default capacities
    import inspect
    from llmrankers._runtime import T5Runtime
    sig = inspect.signature(T5Runtime.__init__).parameters
    group = -(-default_queries_per_call("duot5", 100) // 2)
    assert 2 * group <= sig["max_seqs"].default and 2 * group * 512 <= sig["max_tokens"].default
