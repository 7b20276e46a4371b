"""Drafting by prompt lookup on the host: the Python reference of the proposer and the accept machine (tests/_draft_ref.py: what the
GPU tests hold the device to) on known answers, and the plumbing - LlamaRuntime.open_pool's draft_tokens, DecodePool.tokens_per_step,
the two Rank-R1 rankers' with_draft_tokens and the command line's --draft_tokens - against the session doubles of the pool tests."""
import importlib.util
import os
import random

import numpy as np
import pytest

import _draft_ref as R
from conftest import GOLD, REPO
from _rankr1_pool_stub import EOS, FakeSession, ScriptedRuntime


# ---- the proposer -------------------------------------------------------------------------------------------------------------------
def test_proposer_known_answers():
    # no match: the last token never occurred before
    assert R.propose([1, 2, 3, 4, 5], 3, 1, 3) == []
    assert R.propose([7], 3, 1, 3) == []                               # nothing in front of the last token
    # a longer n-gram beats a shorter one: the 1-gram [3] was last seen at index 5 (continuation 9), the 2-gram [2, 3] at 1 (-> 4, 5)
    h = [1, 2, 3, 4, 5, 3, 9, 2, 3]
    assert R.propose(h, 2, 1, 3) == [4, 5]
    assert R.propose(h, 2, 1, 1) == [9, 2]
    # the most recent occurrence wins
    assert R.propose([5, 6, 1, 5, 6, 2, 5, 6], 2, 2, 2) == [2, 5]
    # the continuation is clipped at n: the match sits right in front of the tail
    assert R.propose([4, 4], 3, 1, 3) == [4]
    assert R.propose([1, 2, 1, 2, 1, 2], 7, 2, 2) == [1, 2]
    # the tail itself is not a match of itself (i + N < n)
    assert R.propose([1, 2, 3], 3, 3, 3) == []
    # N larger than the history allows is skipped, smaller ones still searched
    assert R.propose([8, 8], 2, 2, 5) == []
    assert R.propose([8, 8], 2, 1, 5) == [8]


def test_draft_limit_clips_by_max_new_max_len_and_cap():
    assert R.draft_limit(n=10, col=1, kd=7, max_new=64, max_len=100) == 7
    assert R.draft_limit(n=10, col=1, kd=7, max_new=5, max_len=100) == 3          # this step's first token, then 3 more: 5 in all
    assert R.draft_limit(n=10, col=4, kd=7, max_new=5, max_len=100) == 0
    assert R.draft_limit(n=97, col=1, kd=7, max_new=64, max_len=100) == 3         # rows at 96 | 97, 98, 99 = max_len - 1
    assert R.draft_limit(n=100, col=1, kd=7, max_new=64, max_len=100) == 0
    assert R.draft_limit(n=10, col=1, kd=7, max_new=64, max_len=100, cap=4) == 2


def test_accept_machine():
    prompt, plain = [1, 2, 3], [10, 11, 12, 13, 14, 15, 16, 17, 18, 19]
    # the table is the plain output: the admit's token, then runs of Kd + 1
    toks, steps, acc = R.run_machine(prompt, plain, 3, (1, 3), 10, [], 64, table=plain)
    assert (toks, steps, acc) == (plain, 3, [4, 4, 1])
    # a wrong draft cuts the run; the row behind it is never looked at
    table = list(plain)
    table[3] = 99
    toks, steps, acc = R.run_machine(prompt, plain, 3, (1, 3), 10, [], 64, table=table)
    assert (toks, steps, acc) == (plain, 3, [3, 4, 2])               # 11 12 13 | 14 15 16 17 | 18 19: the draft for column 3 was wrong
    # garbage: one token per step, the plain session's count
    assert R.run_machine(prompt, plain, 7, (1, 3), 10, [], 64, table=[0] * 10)[1:] == (9, [1] * 9)
    # an EOS inside an accepted run ends the request there; max_new inside one too
    assert R.run_machine(prompt, plain[:4], 7, (1, 3), 10, [13], 64, table=plain)[:2] == (plain[:4], 1)
    assert R.run_machine(prompt, plain[:6], 3, (1, 3), 6, [], 64, table=plain) == (plain[:6], 2, [4, 1])
    # the lookup: a model that repeats its prompt is drafted from the prompt
    prompt = [1, 2, 3, 4, 5, 6, 7, 8]
    plain = [1, 2, 3, 4, 5, 6, 7, 8]
    toks, steps, acc = R.run_machine(prompt, plain, 3, (1, 3), 8, [], 64)
    assert toks == plain and steps == 2 and acc == [4, 3]
    assert R.run_machine(prompt, plain, 0, (1, 3), 8, [], 64)[1] == 7


# ---- the pool -----------------------------------------------------------------------------------------------------------------------
class _Engine:
    """RkLlamaEngine.session's signature over the pool tests' FakeSession; every call is recorded"""

    def __init__(self, completion):
        self.completion, self.calls, self.log = completion, [], []

    def session(self, n_slots, max_len, max_new_cap, eos_ids, pad_id, **kw):
        self.calls.append((n_slots, kw))
        return FakeSession(self.completion, n_slots, max_len, max_new_cap, self.log)


def _runtime(max_seqs=16, completion=None):
    from llmrankers._runtime import LlamaRuntime
    rt = LlamaRuntime.__new__(LlamaRuntime)
    rt.max_seqs, rt.max_tokens = max_seqs, 4096
    rt.engine = _Engine(completion or (lambda ids, m: ([t + 1 for t in ids] + [EOS])[:m]))
    return rt


def test_open_pool_slot_count_and_the_option_reaching_the_engine():
    rt = _runtime()
    for draft, n_slots, want_slots, want_kw in ((0, None, 16, {}), (1, None, 8, {"draft": 1}), (3, None, 4, {"draft": 3}),
                                                (7, None, 2, {"draft": 7}), (3, 1, 1, {"draft": 3}), (0, 5, 5, {})):
        kw = {} if draft == 0 else {"draft_tokens": draft}
        with rt.open_pool(8, [EOS], 0, n_slots=n_slots, **kw) as pool:
            assert pool.n_slots == want_slots and pool.tokens_per_step == 0.0
            pool.submit("a", [5, 6, 7], 8)
            pool.submit("b", [9], 8)
            got = {}
            while pool.pending():
                got.update({k: [int(t) for t in v] for k, v in pool.wait()})
            assert got == {"a": [6, 7, 8, EOS], "b": [10, EOS]}
            assert pool.tokens_per_step == pool.tokens_out / pool.steps and pool.tokens_out == 6
        assert rt.engine.calls[-1] == (want_slots, want_kw), (draft, rt.engine.calls[-1])
    # refusals, before anything is opened
    n = len(rt.engine.calls)
    with pytest.raises(ValueError, match="draft_tokens"):
        rt.open_pool(8, [EOS], 0, n_slots=5, draft_tokens=3)           # 5 x 4 > 16
    for bad in (8, -1, 1.5, "3", None):
        with pytest.raises(ValueError, match="draft_tokens"):
            rt.open_pool(8, [EOS], 0, draft_tokens=bad)
    with pytest.raises(ValueError, match="n_slots"):
        rt.open_pool(8, [EOS], 0, n_slots=17)
    assert len(rt.engine.calls) == n


def test_session_wrapper_calls_the_plain_entry_point_without_drafting():
    """LlamaSession: draft = 0 is rk_llama_session_open, draft > 0 rk_llama_session_open_draft with the n-gram range"""
    from llmrankers._engine import LlamaSession
    calls = []

    class Lib:
        def rk_llama_session_open(self, h, *a):
            calls.append(("open", a[:3], a[-1]))
            return 0

        def rk_llama_session_open_draft(self, h, *a):
            calls.append(("open_draft", a[:3], a[-4:]))
            return 0

        def rk_llama_session_close(self, h):
            return 0

    class Eng:
        lib, h = Lib(), 1

        def _chk(self, rc):
            assert rc == 0

    LlamaSession(Eng(), 4, 64, 8, [2], 0).close()
    LlamaSession(Eng(), 4, 64, 8, [2], 0, draft=0, ngram=(2, 5)).close()
    s = LlamaSession(Eng(), 2, 64, 8, [2], 0, draft=3)
    assert (s.draft, s.ngram) == (3, (1, 3))
    LlamaSession(Eng(), 2, 64, 8, [2], 0, draft=7, ngram=(2, 5)).close()
    assert calls == [("open", (4, 64, 8), 0), ("open", (4, 64, 8), 0), ("open_draft", (2, 64, 8), (0, 3, 1, 3)),
                     ("open_draft", (2, 64, 8), (0, 7, 2, 5))]


# ---- the rankers --------------------------------------------------------------------------------------------------------------------
class _DraftRuntime(ScriptedRuntime):
    """ScriptedRuntime whose pool takes LlamaRuntime.open_pool's draft_tokens and records what it was asked for"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pools = []

    def open_pool(self, max_new_cap, eos_ids, pad_id, n_slots=None, **kw):
        self.pools.append((n_slots, kw))
        return super().open_pool(max_new_cap, eos_ids, pad_id, n_slots=n_slots)


@pytest.fixture(scope="module")
def tok():
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(os.path.join(GOLD, "tok_qwen"))


def _items(n_queries):
    from test_rankr1_many_host import _items as items
    return items(n_queries)


@pytest.mark.parametrize("num_permutation", [1, 2])
def test_rankr1_setwise_single_query_goes_through_a_one_slot_pool(tok, num_permutation):
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    prompt = os.path.join(GOLD, "rankr1_prompt.toml")
    kw = dict(num_child=3, k=4, num_permutation=num_permutation, max_new_tokens=10)
    cls = RankR1SetwiseLlmRanker.with_draft_tokens(3)
    assert issubclass(cls, RankR1SetwiseLlmRanker) and cls.__name__ == "RankR1SetwiseLlmRanker" and cls.draft_tokens == 3
    assert RankR1SetwiseLlmRanker.draft_tokens == 0 and RankR1SetwiseLlmRanker.with_draft_tokens(0) is RankR1SetwiseLlmRanker
    assert RankR1SetwiseLlmRanker.with_draft_tokens(3) is cls
    both = RankR1SetwiseLlmRanker.with_weight_dtype("fp8").with_draft_tokens(2)
    assert (both.weight_dtype, both.draft_tokens) == ("fp8", 2)
    for bad in (8, -1, "x"):
        with pytest.raises(ValueError, match="draft_tokens"):
            RankR1SetwiseLlmRanker.with_draft_tokens(bad)
    plain_rt, draft_rt = _DraftRuntime(tok, n_slots=8), _DraftRuntime(tok, n_slots=8)     # 8 rows: two slots of Kd + 1 = 4
    plain = RankR1SetwiseLlmRanker.from_runtime(plain_rt, tok, prompt, **kw)
    draft = cls.from_runtime(draft_rt, tok, prompt, **kw)
    (query, ranking), = _items(1)
    random.seed(5)
    want = ([d.docid for d in plain.rerank(query, ranking)], plain.total_compare, plain.total_prompt_tokens, plain.total_completion_tokens)
    (query, ranking), = _items(1)
    random.seed(5)
    got = ([d.docid for d in draft.rerank(query, ranking)], draft.total_compare, draft.total_prompt_tokens, draft.total_completion_tokens)
    assert got == want
    # the plain ranker never opened a pool; the drafting one decoded every compare through one of num_permutation slots, no generate
    assert plain_rt.pools == [] and plain_rt.generate_calls > 0
    assert draft_rt.generate_calls == 0 and len(draft_rt.pools) == plain_rt.generate_calls
    assert set(map(repr, draft_rt.pools)) == {repr((num_permutation, {"draft_tokens": 3}))}
    # several queries: the pool of rerank_many carries the option, and the default ranker's call is what it was
    its = _items(3)
    random.seed(9)
    want_many = plain.rerank_many(its)
    its = _items(3)
    random.seed(9)
    got_many = draft.rerank_many(its)
    assert [[d.docid for d in r] for r in got_many[0]] == [[d.docid for d in r] for r in want_many[0]] and got_many[1] == want_many[1]
    assert plain_rt.pools == [(None, {})] and draft_rt.pools[-1] == (None, {"draft_tokens": 3})


def test_r1_listwise_takes_the_option(tok):
    from llmrankers.listwise import R1ListwiseLlmRanker
    from test_mistral_host import PROMPT
    cls = R1ListwiseLlmRanker.with_draft_tokens(7)
    assert issubclass(cls, R1ListwiseLlmRanker) and cls.draft_tokens == 7 and R1ListwiseLlmRanker.draft_tokens == 0
    plain_rt, draft_rt = _DraftRuntime(tok), _DraftRuntime(tok)
    (query, ranking), = _items(1)
    out = []
    for c, rt in ((R1ListwiseLlmRanker, plain_rt), (cls, draft_rt)):
        rk = c.from_runtime(rt, tok, PROMPT, window_size=4, step_size=2, max_new_tokens=10)
        res = rk.rerank(query, list(ranking))
        out.append(([d.docid for d in res], rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens))
    assert out[0] == out[1]
    assert plain_rt.pools == [] and draft_rt.generate_calls == 0 and draft_rt.pools and all(p == (1, {"draft_tokens": 7}) for p in draft_rt.pools)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runmod():
    spec = importlib.util.spec_from_file_location("rk_run_draft", os.path.join(REPO, "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_draft_tokens(runmod, monkeypatch):
    import llmrankers.listwise as lw
    import llmrankers.setwise as sw
    made = {}

    class Stub:
        weight_dtype, draft_tokens = "fp16", 0

        def __init__(self, **kw):
            made.clear()
            made.update(kw, cls=type(self), draft=type(self).draft_tokens, dtype=type(self).weight_dtype)

        @classmethod
        def with_weight_dtype(cls, wd):
            return type(cls.__name__, (cls,), {"weight_dtype": wd})

        @classmethod
        def with_draft_tokens(cls, n):
            return type(cls.__name__, (cls,), {"draft_tokens": n})

    stubs = {}
    for mod, names in ((sw, ("SetwiseLlmRanker", "RankR1SetwiseLlmRanker")), (lw, ("ListwiseLlmRanker", "R1ListwiseLlmRanker"))):
        for n in names:
            stubs[n] = type(n, (Stub,), {})
            monkeypatch.setattr(mod, n, stubs[n])
    parser, commands = runmod.build_parser()
    head = ["run", "--model_name_or_path", "m"]
    for name, tail in (("RankR1SetwiseLlmRanker", ["setwise"]), ("R1ListwiseLlmRanker", ["listwise"])):
        a = runmod.parse_args(parser, commands, head + ["--prompt_file", "p.toml"] + tail)
        assert a.run.draft_tokens == 0
        runmod.build_ranker(a)
        assert made["cls"] is stubs[name] and made["draft"] == 0 and "draft_tokens" not in made      # the default: the class as it is
        a = runmod.parse_args(parser, commands, head + ["--prompt_file", "p.toml", "--draft_tokens", "3"] + tail)
        runmod.build_ranker(a)
        assert issubclass(made["cls"], stubs[name]) and made["draft"] == 3 and "draft_tokens" not in made
        a = runmod.parse_args(parser, commands, head + ["--prompt_file", "p.toml", "--draft_tokens", "7", "--weight_dtype", "fp8"] + tail)
        runmod.build_ranker(a)
        assert (made["draft"], made["dtype"]) == (7, "fp8")
    for bad in ("8", "-1", "x"):
        with pytest.raises(SystemExit):
            runmod.parse_args(parser, commands, head + ["--draft_tokens", bad, "setwise"])
    # without --prompt_file the flag has no ranker to go to: refused by name, and 0 changes nothing
    for tail in (["setwise"], ["listwise"], ["pointwise"], ["pairwise"]):
        a = runmod.parse_args(parser, commands, head + ["--draft_tokens", "2"] + tail)
        with pytest.raises(NotImplementedError, match="draft_tokens"):
            runmod.build_ranker(a)
    a = runmod.parse_args(parser, commands, head + ["--draft_tokens", "0", "setwise"])
    runmod.build_ranker(a)
    assert made["cls"] is stubs["SetwiseLlmRanker"]
