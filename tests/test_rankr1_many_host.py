"""Rank-R1 for several queries on the host: RankR1SetwiseLlmRanker.rerank_many over a decoding pool (scripted completions that
return out of submission order), the pool's scheduler over a fake session, and the CLI's way to the ranker."""
import importlib.util
import os
import random

import pytest

from conftest import GOLD, REPO
from _rankr1_pool_stub import FakeSession, ScriptedRuntime

WORDS = ("neural ranking model search engine index query passage water river mountain forest ocean climate carbon energy market "
         "bank policy language network system city history music science data study result method patient school price trade law "
         "court food soil").split()

SEED = 929


@pytest.fixture(scope="module")
def tok():
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(os.path.join(GOLD, "tok_qwen"))


def _items(n_queries, n_docs=11, seed=7):
    from llmrankers.rankers import SearchResult
    rs = random.Random(seed)
    return [(" ".join(rs.sample(WORDS, 3)),
             [SearchResult(docid=f"q{q}d{d}", score=None, text=" ".join(rs.sample(WORDS, 6 + d % 3))) for d in range(n_docs)])
            for q in range(n_queries)]


def _ranker(tok, method, num_permutation, n_slots=4):
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    rt = ScriptedRuntime(tok, n_slots=n_slots)
    rk = RankR1SetwiseLlmRanker.from_runtime(rt, tok, os.path.join(GOLD, "rankr1_prompt.toml"), num_child=3, k=4, method=method,
                                             num_permutation=num_permutation, max_new_tokens=10)
    return rk, rt


def _snapshot(rk, res, ranking):
    return ([d.docid for d in res], [d.docid for d in ranking], (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens))


@pytest.mark.parametrize("method,num_permutation", [("heapsort", 1), ("heapsort", 2), ("bubblesort", 1), ("bubblesort", 2)])
def test_rerank_many_equals_one_by_one_under_the_per_query_generators(tok, method, num_permutation):
    """6 queries through the pool (4 slots, completions of 1 .. 12 tokens: they return out of order, some name no label, some a label
    beyond the window, two permutations tie) == rerank per query with random.Random(seed_i), seed_i drawn in item order"""
    rk, rt = _ranker(tok, method, num_permutation)
    random.seed(11)
    seeds = [random.getrandbits(64) for _ in range(6)]
    want = []
    for (query, ranking), seed in zip(_items(6), seeds):
        rk.compare_rng = random.Random(seed)
        want.append(_snapshot(rk, rk.rerank(query, ranking), ranking))
    rk.compare_rng = None
    assert rt.log == [] and rt.generate_calls == sum(w[2][0] // num_permutation for w in want)
    many = _items(6)
    random.seed(11)
    results, counters = rk.rerank_many(many)
    got = [([d.docid for d in res], [d.docid for d in ranking], tuple(c)) for res, (_, ranking), c in zip(results, many, counters)]
    assert got == want
    assert (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens) == want[-1][2]
    assert random.getrandbits(32) == _after_seeds(11, 6)             # the module stream gave the six seeds and nothing else
    # the settings bite: rankings moved, counters differ per query, and the pool really interleaved
    assert any(w[0] != [f"q{q}d{d}" for d in range(11)] for q, w in enumerate(want))
    assert len({w[2] for w in want}) > 1
    admits = [e for e in rt.log if e[0] == "admit"]
    assert rt.log[0][0] == "open" and rt.log[-1][0] == "close" and sum(e[0] == "open" for e in rt.log) == 1
    assert len(admits[0][1]) == 4 and len(admits) > 3                # the first admit fills the pool, later ones refill it
    assert sum(len(e[1]) for e in admits) == sum(w[2][0] for w in want)


def _after_seeds(seed, n):
    r = random.Random(seed)
    for _ in range(n):
        r.getrandbits(64)
    return r.getrandbits(32)


def test_single_query_and_runtimes_without_a_pool_keep_the_module_stream(tok):
    """one query, or a runtime that has no open_pool: rerank per query, drawing from the module-level random as before"""
    rk, rt = _ranker(tok, "heapsort", 2)
    (query, ranking), = _items(1)
    random.seed(5)
    want = _snapshot(rk, rk.rerank(query, ranking), ranking)
    (query, ranking), = _items(1)
    random.seed(5)
    results, counters = rk.rerank_many([(query, ranking)])
    assert ([d.docid for d in results[0]], [d.docid for d in ranking], tuple(counters[0])) == want and rt.log == []

    class GenerateOnly:                                              # a runtime with no pool (the oracle runtimes of other tests)
        model_type, generation, generate = rt.model_type, rt.generation, rt.generate

    rk.llm = GenerateOnly()
    its = _items(2)
    random.seed(5)
    want = [_snapshot(rk, rk.rerank(q, r), r) for q, r in its]
    its = _items(2)
    random.seed(5)
    results, counters = rk.rerank_many(its)
    assert [([d.docid for d in res], [d.docid for d in r], tuple(c)) for res, (_, r), c in zip(results, its, counters)] == want


def test_rerank_and_compare_on_the_module_stream_give_what_they_gave(tok):
    """compare's split into prompts / engine call / verdict changed nothing: rerank and compare under a seeded module-level random
    == the values recorded before the split (RECORDED below)"""
    for (method, num_permutation), (ranked, counters, labels) in RECORDED.items():
        rk, rt = _ranker(tok, method, num_permutation)
        its = _items(3)
        random.seed(SEED)
        got_ranked, got_counters = [], []
        for query, ranking in its:
            got_ranked.append([d.docid for d in rk.rerank(query, ranking)])
            got_counters.append((rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens))
        query, ranking = _items(3)[0]
        got_labels = [rk.compare(query, ranking[i:i + 4]) for i in (0, 3, 6)]
        assert (got_ranked, got_counters, got_labels) == (ranked, counters, labels), (method, num_permutation)
        assert rt.log == []                                          # no pool on this path


# ---- the pool's scheduler over a fake session ------------------------------------------------------------------------------------
def _pool(n_slots, lengths, max_tokens=4096, cap=64):
    """a DecodePool whose requests complete after lengths[first prompt id] tokens"""
    from llmrankers._runtime import DecodePool
    log = []
    completion = lambda ids, m: ([7] * lengths[ids[0]])[:m]          # noqa: E731
    return DecodePool(lambda max_len: FakeSession(completion, n_slots, max_len, cap, log), n_slots, max_tokens, cap), log


def test_pool_is_fifo_bounded_and_admits_together():
    lengths = {0: 9, 1: 2, 2: 5, 3: 1, 4: 3, 5: 3, 6: 8}
    pool, log = _pool(3, lengths)
    with pool:
        for r in range(7):
            pool.submit(r, [r] * (10 + r), 64)
        order = []
        while pool.pending():
            done = pool.wait()
            assert done
            for key, tokens in done:
                assert list(tokens) == [7] * lengths[key]
                order.append(key)
        assert pool.wait() == []
    assert sorted(order) == list(range(7)) and order != list(range(7))   # completion order is not submission order
    admits = [e for e in log if e[0] == "admit"]
    assert [n for e in admits for n in e[2]] == [10 + r for r in range(7)]   # FIFO: prompts reach the session in submission order
    assert len(admits[0][1]) == 3                                    # three pending prompts, ONE admit
    assert any(len(e[1]) > 1 for e in admits[1:])                    # two slots freed by one run: refilled together
    assert [e[0] for e in log].count("open") == 1 and log[-1] == ("close", [])
    assert pool.admits == len(admits) and pool.tokens_out == sum(lengths.values())


def test_pool_refuses_what_can_never_fit_and_grows_between_drains():
    pool, log = _pool(2, {0: 4, 1: 4, 2: 4}, max_tokens=2048)
    with pytest.raises(ValueError):
        pool.submit("big", [0] * 2000, 49)                           # len + max_new > the engine's capacity
    with pytest.raises(ValueError):
        pool.submit("cap", [0] * 10, 65)                             # max_new > max_new_cap
    with pool:
        pool.submit("a", [0] * 100, 64)
        pool.submit("b", [1] * 100, 64)
        assert [k for k, _ in pool.wait()] == ["a", "b"]
        pool.submit("c", [2] * 600, 64)                              # needs a longer session than the one that is open
        pool.submit("d", [0] * 100, 64)
        assert [k for k, _ in pool.wait()] == ["c", "d"]
        pool.submit("e", [1] * 100, 64)                              # the larger session stays: nothing is re-opened
        assert [k for k, _ in pool.wait()] == ["e"]
    opens = [e for e in log if e[0] == "open"]
    assert [e[2] for e in opens] == [512, 1024] and pool.opens == 2


def test_an_exception_mid_flight_closes_the_session():
    pool, log = _pool(2, {0: 9, 1: 9, 2: 9})
    with pytest.raises(KeyError):
        with pool:
            for r in range(3):
                pool.submit(r, [r] * 20, 64)
            pool._fill()                                             # two requests decoding, one queued
            assert len(pool.session.busy) == 2
            raise KeyError("caller's error")
    assert log[-1] == ("close", [0, 1]) and pool.session is None and pool.pending() == 0


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runmod():
    spec = importlib.util.spec_from_file_location("rk_run_r1", os.path.join(REPO, "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_builds_the_rankr1_ranker(runmod, monkeypatch):
    import llmrankers.setwise as sw
    made = {}

    class Stub:
        def __init__(self, **kw):
            made.update(kw, cls=type(self).__name__)

    class R1(Stub):
        pass

    class Plain(Stub):
        pass

    monkeypatch.setattr(sw, "RankR1SetwiseLlmRanker", R1)
    monkeypatch.setattr(sw, "SetwiseLlmRanker", Plain)
    parser, commands = runmod.build_parser()
    a = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "m", "--prompt_file", "p.toml", "--lora_name_or_path", "l",
                                             "--max_new_tokens", "77", "setwise", "--num_child", "19", "--k", "5", "--num_permutation", "2"])
    runmod.validate(a)
    assert isinstance(runmod.build_ranker(a), R1)
    assert (made["cls"], made["model_name_or_path"], made["prompt_file"], made["lora_name_or_path"], made["max_new_tokens"],
            made["num_child"], made["k"], made["num_permutation"], made["method"]) == ("R1", "m", "p.toml", "l", 77, 19, 5, 2, "heapsort")
    # the reference's spelling of the adapter flag, and the defaults
    b = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "m", "--prompt_file", "p.toml", "--lora_path_or_name", "x", "setwise"])
    assert (b.run.lora_name_or_path, b.run.max_new_tokens) == ("x", 2048)
    # without --prompt_file nothing changes: the plain setwise ranker with the arguments it always got
    made.clear()
    c = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "m", "setwise"])
    assert c.run.prompt_file is None and c.run.lora_name_or_path is None
    assert isinstance(runmod.build_ranker(c), Plain)
    assert sorted(made) == sorted(["cls", "model_name_or_path", "tokenizer_name_or_path", "device", "cache_dir", "num_child", "scoring",
                                   "method", "num_permutation", "k"])


def test_default_queries_per_call_for_rankr1():
    from llmrankers._batching import default_queries_per_call
    assert default_queries_per_call("rankr1", 100) == 16             # LlamaRuntime's default slot count
    assert default_queries_per_call("rankr1", 100, slots=8) == 8
    assert (default_queries_per_call("setwise", 100), default_queries_per_call("pairwise", 100)) == (32, 1)


# rerank() of _items(3), query after query, under random.seed(SEED), then compare() on three windows of query 0 - recorded on the
# commit before compare was split, with the same stand-in runtime: (method, num_permutation) -> (ranked docids per query,
# (total_compare, total_prompt_tokens, total_completion_tokens) per query, the three labels)
RECORDED = {('bubblesort', 1): ([['q0d9', 'q0d0', 'q0d10', 'q0d3', 'q0d1', 'q0d2', 'q0d4', 'q0d5', 'q0d6', 'q0d7', 'q0d8'],
                      ['q1d0', 'q1d2', 'q1d3', 'q1d1', 'q1d4', 'q1d5', 'q1d6', 'q1d7', 'q1d8', 'q1d9', 'q1d10'],
                      ['q2d0', 'q2d1', 'q2d2', 'q2d3', 'q2d4', 'q2d5', 'q2d6', 'q2d7', 'q2d8', 'q2d9', 'q2d10']],
                     [(13, 961, 94), (7, 496, 32), (7, 496, 42)], ['Unexpected voting.', '[1]', '[1]']),
 ('bubblesort', 2): ([['q0d1', 'q0d0', 'q0d2', 'q0d9', 'q0d3', 'q0d4', 'q0d5', 'q0d6', 'q0d7', 'q0d8', 'q0d10'],
                      ['q1d4', 'q1d0', 'q1d6', 'q1d3', 'q1d1', 'q1d2', 'q1d5', 'q1d7', 'q1d8', 'q1d9', 'q1d10'],
                      ['q2d0', 'q2d1', 'q2d2', 'q2d3', 'q2d4', 'q2d5', 'q2d6', 'q2d7', 'q2d8', 'q2d9', 'q2d10']],
                     [(26, 1914, 189), (26, 1924, 177), (14, 868, 102)], ['[3]', '[4]', '[2]']),
 ('heapsort', 1): ([['q0d0', 'q0d1', 'q0d9', 'q0d8', 'q0d2', 'q0d3', 'q0d4', 'q0d5', 'q0d6', 'q0d7', 'q0d10'],
                    ['q1d0', 'q1d2', 'q1d9', 'q1d8', 'q1d1', 'q1d3', 'q1d4', 'q1d5', 'q1d6', 'q1d7', 'q1d10'],
                    ['q2d0', 'q2d10', 'q2d9', 'q2d1', 'q2d2', 'q2d3', 'q2d4', 'q2d5', 'q2d6', 'q2d7', 'q2d8']],
                   [(8, 599, 47), (8, 597, 46), (8, 600, 61)], ['[2]', 'Unexpected voting.', 'Unexpected voting.']),
 ('heapsort', 2): ([['q0d0', 'q0d10', 'q0d9', 'q0d1', 'q0d2', 'q0d3', 'q0d4', 'q0d5', 'q0d6', 'q0d7', 'q0d8'],
                    ['q1d0', 'q1d10', 'q1d9', 'q1d8', 'q1d1', 'q1d2', 'q1d3', 'q1d4', 'q1d5', 'q1d6', 'q1d7'],
                    ['q2d4', 'q2d10', 'q2d8', 'q2d5', 'q2d0', 'q2d1', 'q2d2', 'q2d3', 'q2d6', 'q2d7', 'q2d9']],
                   [(16, 1200, 114), (14, 1036, 89), (20, 1488, 132)], ['[3]', '[3]', 'Unexpected voting.'])}
