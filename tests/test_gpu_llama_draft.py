"""Drafting by prompt lookup on the Llama engine's decoding session (rk_llama_session_open_draft): Kd extra rows per slot and step,
fed with drafted tokens, accepted on the device.  The contract: a request's tokens, and where it finishes, are bit for bit the plain
session's - only the number of steps differs, and that number is the reference machine's (tests/_draft_ref.py) exactly.

Every engine form the step has: toy-llama (128 wide, R = 2), toy-qwen2 (bias, 7 heads on one kv head: R = 1, and R = 7 under
llama_dec_r = 2), toy-qwen3 (q / k head norm), toy-mistral (window 64), the 64-wide llama / qwen2 / mistral and toy-llama on one kv head (128 wide, R = 4).  Prompt lengths 28,
60 and 124 put a step's rows across positions 31 / 32 (a wave's keys), 63 / 64 (the Mistral toys' window: the first visible key
moves inside one step's rows) and 127 / 128 (LDC_CHUNK)."""
import dataclasses

import numpy as np
import pytest

import _draft_ref as R

pytestmark = pytest.mark.gpu

PAD = 0
LENS = (5, 28, 60, 124)
MAX_NEW, MAX_LEN = 24, 160
FORMS = [("toy-llama", 0), ("toy-qwen2", 0), ("toy-qwen2", 2), ("toy-qwen3", 0), ("toy-mistral", 0), ("toy-llama-hd64", 0),
         ("toy-qwen2-hd64", 0), ("toy-mistral-hd64", 0), ("toy-llama-g4", 0)]
G4 = "toy-llama-g4"                 # toy-llama with ONE kv head: four query heads per kv head at width 128, the R = 4 entries Llama-3-8B runs


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 4096)
    kw.setdefault("max_seqs", 32)
    return RkLlamaEngine(dims, device=0, **kw).load_state(state.items())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _decode(eng, prompts, max_new, eos, kd=0, tables=None, max_len=MAX_LEN, cap=MAX_NEW, n_slots=None, ngram=(1, 3), rows=True):
    """All prompts admitted at once, one step per run -> per prompt (tokens, steps its request was active in, {column: the
    final-normed row that produced it}).  tables: rk_debug_session_drafts per slot (None: the lookup)."""
    n = len(prompts)
    hidden, g1 = eng.dims.hidden, kd + 1
    got_rows = [dict() for _ in prompts]
    with eng.session(n_slots or n, max_len, cap, eos, PAD, draft=kd, ngram=ngram) as s:
        if tables is not None:
            for b, t in enumerate(tables):
                s.set_drafts(b, t)
        s.admit(prompts, list(range(n)), list(max_new))
        done = set(s.run(0)[0])
        guard = 0
        while len(done) < n:
            before = s.stats()["slot_cols"].copy()
            finished, steps = s.run(1)
            assert steps == 1
            done.update(finished)
            after = s.stats()["slot_cols"]
            if rows:
                last = eng.debug_read("llama_last", s.n_slots * g1 * hidden).reshape(-1, hidden)
                for b in range(n):
                    for j in range(int(after[b] - before[b])):
                        got_rows[b][int(before[b]) + j] = last[b * g1 + j].copy()
            guard += 1
            assert guard <= max(max_new) + 2, "the session does not finish"
        st = s.stats()
        steps = [int(x) for x in st["slot_steps"][:n]]
        toks = [[int(t) for t in s.read(b)] for b in range(n)]
    return toks, steps, got_rows


@pytest.fixture(scope="module", params=FORMS, ids=lambda f: f"{f[0]}-r{f[1]}")
def form(request):
    """engine, prompts and the PLAIN session's tokens, rows and steps for them, without EOS - computed once, never modified"""
    from llmrankers import _synth
    name, dec_r = request.param
    dims = dataclasses.replace(_synth.TOY_LLAMA, n_kv_heads=1) if name == G4 else _synth.NAMED_DIMS[name]
    state = _synth.synth_state_dict(dims, seed=929)
    base = _synth.synth_token_batch(1, 200, 200, dims.vocab, seed=17)[0]
    prompts = [[int(t) for t in base[7 * i:7 * i + n]] for i, n in enumerate(LENS)]
    eng = _engine(dims, state)
    if dec_r:
        eng.set_option("llama_dec_r", dec_r)
    toks, steps, rows = _decode(eng, prompts, [MAX_NEW] * len(prompts), [])
    assert [len(t) for t in toks] == [MAX_NEW] * len(prompts) and steps == [MAX_NEW - 1] * len(prompts)
    yield eng, dims, prompts, toks, rows
    eng.close()


def _garbage(plain, vocab):
    return [(t + 1 + (i % 3)) % vocab for i, t in enumerate(plain)]      # differs from the plain token in every column


def _third(plain, vocab):
    return [(t + 1) % vocab if i % 3 == 2 else t for i, t in enumerate(plain)]


def _check(eng, dims, prompts, plain, plain_rows, kd, tables, eos, max_new, what, **kw):
    """draft session against the plain one: tokens, finish columns, reference steps, accepted rows bit for bit"""
    toks, steps, rows = _decode(eng, prompts, max_new, eos, kd=kd, tables=tables, rows=plain_rows is not None, **kw)
    for b, p in enumerate(prompts):
        assert toks[b] == plain[b], (what, kd, b, toks[b], plain[b])
        ref_toks, ref_steps, _ = R.run_machine(p, plain[b], kd, (1, 3), max_new[b], eos, kw.get("max_len", MAX_LEN), kw.get("cap", MAX_NEW),
                                               table=None if tables is None else tables[b])
        assert ref_toks == plain[b]
        assert steps[b] == ref_steps, (what, kd, b, steps[b], ref_steps)
        if plain_rows is not None:
            for c, row in rows[b].items():
                if c >= 1:
                    assert np.array_equal(_bits(row), _bits(plain_rows[b][c])), (what, kd, b, c)
            assert set(rows[b]) == set(range(1, len(plain[b])))
    return steps


@pytest.mark.parametrize("kd", [1, 3, 7])
def test_oracle_drafts(form, kd):
    """Check 1: tables = the plain output (all accepted), every third token replaced (runs cut), garbage (nothing accepted)"""
    eng, dims, prompts, plain, plain_rows = form
    mn = [MAX_NEW] * len(prompts)
    steps = _check(eng, dims, prompts, plain, plain_rows, kd, [list(t) for t in plain], [], mn, "all")
    assert all(s < len(t) for s, t in zip(steps, plain)), steps
    assert steps == [-(-(MAX_NEW - 1) // (kd + 1))] * len(prompts), steps
    steps = _check(eng, dims, prompts, plain, plain_rows, kd, [_third(t, dims.vocab) for t in plain], [], mn, "third")
    assert all(-(-(MAX_NEW - 1) // (kd + 1)) < s < MAX_NEW - 1 for s in steps), steps
    steps = _check(eng, dims, prompts, plain, plain_rows, kd, [_garbage(t, dims.vocab) for t in plain], [], mn, "garbage")
    assert steps == [MAX_NEW - 1] * len(prompts), steps


def test_boundaries(form):
    """Check 2: an EOS inside an accepted run (nothing behind it is emitted), max_new inside an accepted run, and requests whose
    last rows reach position max_len - 1 with Kd rows that would pass it (dead rows: no write, nothing accepted past the end)"""
    eng, dims, prompts, plain, plain_rows = form
    kd = 7
    # EOS: the plain session WITH the eos set is the reference (column 10 of prompt 1 and whatever else holds that id)
    eos = [plain[1][10]]
    toks, _, _ = _decode(eng, prompts, [MAX_NEW] * len(prompts), eos, rows=False)
    assert len(toks[1]) <= 11 and toks[1][-1] == eos[0]
    _check(eng, dims, prompts, toks, None, kd, [list(t) for t in plain], eos, [MAX_NEW] * len(prompts), "eos")
    # max_new 6, 7, 10, 13: inside the runs of 8 that the all-accepted table gives
    mn = [6, 7, 10, 13]
    short = [t[:m] for t, m in zip(plain, mn)]
    steps = _check(eng, dims, prompts, short, None, kd, [list(t) for t in plain], [], mn, "max_new")
    assert steps == [1, 1, 2, 2], steps
    # the end of the cache: len + max_new == max_len for the longest, two slots so that a write past a row would land in the next
    two = [prompts[3], prompts[3][:-1] + [(prompts[3][-1] + 1) % dims.vocab]]
    ref, _, _ = _decode(eng, two, [12, 12], [], rows=False, max_len=LENS[3] + 12, cap=12)
    for tab in ([list(t) for t in ref], [_third(t, dims.vocab) for t in ref]):
        _check(eng, dims, two, ref, None, kd, tab, [], [12, 12], "max_len", max_len=LENS[3] + 12, cap=12)
    assert ref[0] == plain[3][:12]


def test_lookup_proposer(form):
    """Check 3: no table: the device lookup.  Steps and tokens equal the Python reference's; prompts that repeat themselves and 64
    new tokens, and at least one case where the reference alone accepts drafts (steps < tokens - 1)."""
    eng, dims, prompts, plain, _ = form
    rep = [(prompts[1][:9] * 4)[:n] for n in (30, 36)] + [prompts[2]]
    mn = [64] * len(rep)
    ref, _, _ = _decode(eng, rep, mn, [], rows=False, max_len=MAX_LEN, cap=64)
    want = [R.run_machine(p, t, 3, (1, 3), 64, [], MAX_LEN, 64)[1] for p, t in zip(rep, ref)]
    print("lookup: reference steps", want, "tokens", [len(t) for t in ref])
    assert any(w < len(t) - 1 for w, t in zip(want, ref)), (want, ref)
    for kd, ngram in ((3, (1, 3)), (7, (2, 4))):
        toks, steps, _ = _decode(eng, rep, mn, [], kd=kd, rows=False, cap=64, ngram=ngram)
        assert toks == ref, (kd, toks, ref)
        assert steps == [R.run_machine(p, t, kd, ngram, 64, [], MAX_LEN, 64)[1] for p, t in zip(rep, ref)], (kd, steps)


def test_independence_refill_hygiene_and_graphs(form):
    """Checks 4 and 5: alone / beside others / after a refill of a slot whose last request left rejected drafts' keys behind;
    sessions of equal sizes replay one graph, another Kd has its own"""
    eng, dims, prompts, plain, _ = form
    kd = 3
    eng.session(2, MAX_LEN, MAX_NEW, [], PAD, draft=kd + 1).close()       # the largest buffers of this test first: no key moves below
    g0 = eng.graph_stats()
    # alone, one slot, garbage drafts first (stale keys beyond every accepted position), then shorter prompts in the same slot
    order = [3, 0, 2, 1]
    with eng.session(1, MAX_LEN, MAX_NEW, [], PAD, draft=kd) as s:
        for i, r in enumerate(order):
            s.set_drafts(0, _garbage(plain[r], dims.vocab) if i % 2 == 0 else None)
            s.admit([prompts[r]], [0], [MAX_NEW])
            while not s.run()[0]:
                pass
            assert [int(t) for t in s.read(0)] == plain[r], r
        st = s.stats()
        assert st["steps"] >= st["tokens"] // (kd + 1) and st["tokens"] == 4 * (MAX_NEW - 1)
    g1 = eng.graph_stats()
    # two slots, four requests: refills beside a running row, lookup drafts
    with eng.session(2, MAX_LEN, MAX_NEW, [], PAD, draft=kd) as s:
        owner, nxt, got = {}, 0, {}
        while nxt < 4 or s.busy:
            for slot in s.free_slots():
                if nxt < 4:
                    s.admit([prompts[nxt]], [slot], [MAX_NEW - 3 * nxt])
                    owner[slot] = nxt
                    nxt += 1
            for slot in s.run()[0]:
                got[owner[slot]] = [int(t) for t in s.read(slot)]
    assert got == {r: plain[r][:MAX_NEW - 3 * r] for r in range(4)}
    # the same sizes again: no new capture; another Kd: a key of its own
    with eng.session(1, MAX_LEN, MAX_NEW, [], PAD, draft=kd) as s:
        s.admit([prompts[0]], [0], [MAX_NEW])
        while not s.run()[0]:
            pass
        s.read(0)
    g2 = eng.graph_stats()
    with eng.session(1, MAX_LEN, MAX_NEW, [], PAD, draft=kd + 1) as s:
        s.admit([prompts[0]], [0], [MAX_NEW])
        while not s.run()[0]:
            pass
        assert [int(t) for t in s.read(0)] == plain[0]
    g3 = eng.graph_stats()
    assert g1["captures"] == g0["captures"] + 1 and g2["captures"] == g1["captures"] + 1      # (1 slot, 2 slots)
    assert g2["n_keys"] == g1["n_keys"] + 1 and g2["replays"] > g1["replays"]
    assert g3["n_keys"] == g2["n_keys"] + 1 and g3["captures"] == g2["captures"] + 1


@pytest.mark.parametrize("name", ["toy-llama", "toy-qwen2"])
def test_fp8_step_weights(name):
    """Check 4, FP8: drafting on an engine with FP8 step weights against the plain session of that engine"""
    from llmrankers import _synth
    dims = dataclasses.replace(_synth.TOY_LLAMA, n_kv_heads=1) if name == G4 else _synth.NAMED_DIMS[name]
    state = _synth.synth_state_dict(dims, seed=929)
    base = _synth.synth_token_batch(1, 200, 200, dims.vocab, seed=17)[0]
    prompts = [[int(t) for t in base[7 * i:7 * i + n]] for i, n in enumerate(LENS)]
    eng = _engine(dims, state, weight_fp8=True)
    mn = [MAX_NEW] * len(prompts)
    plain, _, rows = _decode(eng, prompts, mn, [])
    for kd in (3, 7):
        _check(eng, dims, prompts, plain, rows, kd, [_third(t, dims.vocab) for t in plain], [], mn, "fp8 third")
    _check(eng, dims, prompts, plain, rows, 3, None, [], mn, "fp8 lookup")
    eng.close()


def test_refusals():
    """Check 6"""
    from llmrankers import _synth
    from llmrankers._engine import RkError
    dims = _synth.TOY_LLAMA
    eng = _engine(dims, _synth.synth_state_dict(dims, seed=929), max_seqs=16)

    def refused(code, words, fn):
        with pytest.raises(RkError) as ex:
            fn()
        assert ex.value.code == code and all(w in str(ex.value) for w in words), (ex.value.code, str(ex.value))

    refused(-1, ["draft"], lambda: eng.session(1, 64, 8, [], PAD, draft=8))
    refused(-1, ["draft"], lambda: eng.session(1, 64, 8, [], PAD, draft=-1))
    for ngram in ((0, 3), (1, 9), (3, 2)):
        refused(-1, ["ngram"], lambda: eng.session(1, 64, 8, [], PAD, draft=2, ngram=ngram))
    refused(-6, ["max_seqs", "step rows"], lambda: eng.session(5, 64, 8, [], PAD, draft=3))       # 5 x 4 > 16
    eng.session(4, 64, 8, [], PAD, draft=3).close()                                              # 4 x 4 == 16
    eng.set_sampling(0.7, 0, 1.0)
    refused(-4, ["sampling"], lambda: eng.session(1, 64, 8, [], PAD, draft=2))
    eng.session(1, 64, 8, [], PAD).close()                                                       # (a plain sampled session opens)
    eng.set_sampling(0.0, 0, 1.0)
    with eng.session(1, 64, 8, [], PAD, draft=2) as s:
        refused(-4, ["drafting"], lambda: s.admit([[1, 2, 3]], [0], [4], seeds=[5]))
        refused(-6, ["table"], lambda: s.set_drafts(0, [1] * 9))
        refused(-1, ["slot"], lambda: s.set_drafts(1, [1]))
        s.admit([[1, 2, 3]], [0], [4])                                                           # the refused calls touched nothing
        while not s.run()[0]:
            pass
        assert len(s.read(0)) == 4
    with eng.session(1, 64, 8, [], PAD) as s:
        refused(-4, ["drafting"], lambda: s.set_drafts(0, [1]))
        assert s.stats()["steps"] == 0
    eng.close()


@pytest.mark.parametrize("kd", [3, 7])
def test_rankers_with_drafting_give_the_recorded_cases(tmp_path, kd):
    """Check 7: the recorded Rank-R1 setwise and R1 listwise cases (what the rankers without drafting give: test_gpu_rankr1.py,
    test_gpu_mistral.py) through rankers with drafting on: every compare's output, the ranking, the scores and the three counters"""
    import contextlib
    import io
    import json
    import os
    import random
    from conftest import GOLD
    from transformers import AutoTokenizer
    from llmrankers import _synth
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.listwise import R1ListwiseLlmRanker
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import RankR1SetwiseLlmRanker

    def run(rk, case):
        outs, real = [], rk.compare
        rk.compare = lambda q, docs: outs.append(real(q, docs)) or outs[-1]
        if "random_seed" in case:
            random.seed(case["random_seed"])
        with contextlib.redirect_stdout(io.StringIO()):
            res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
        tag = (kd, case["qid"])
        assert outs == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag

    with open(os.path.join(GOLD, "rankr1_cases.json")) as f:
        gold = json.load(f)
    path, adir = str(tmp_path / "toy-qwen2"), str(tmp_path / "adapter")
    _synth.write_checkpoint(path, gold["ckpt"], os.path.join(GOLD, gold["tokenizer"]))
    _synth.write_lora_adapter(adir, _synth.NAMED_DIMS[gold["ckpt"]["dims"]], gold["adapter"])
    rt = LlamaRuntime(path, "cuda", max_tokens=4096, max_seqs=16, accept_model_types=("qwen2",), adapter_dir=adir)
    tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, gold["tokenizer"]))
    cls = RankR1SetwiseLlmRanker.with_draft_tokens(kd)
    opened = []
    real_pool = rt.open_pool
    rt.open_pool = lambda *a, **kw: opened.append((kw.get("n_slots"), kw.get("draft_tokens"))) or real_pool(*a, **kw)
    for case in gold["cases"]:
        run(cls.from_runtime(rt, tok, os.path.join(GOLD, "rankr1_prompt.toml"), num_child=case["num_child"], k=case["k"], method=case["method"],
                             num_permutation=case["num_permutation"], max_new_tokens=case["max_new_tokens"]), case)
    assert opened and all(d == kd and 1 <= n <= 16 // (kd + 1) for n, d in opened), opened[:4]
    rt.engine.close()

    with open(os.path.join(GOLD, "r1_listwise_cases.json")) as f:
        gold = json.load(f)
    ckpt, adir, tokdir = str(tmp_path / "ckpt"), str(tmp_path / "adapter_l"), os.path.join(GOLD, gold["tokenizer"])
    _synth.write_checkpoint(ckpt, gold["ckpt"], tokdir)
    _synth.write_lora_adapter(adir, _synth.NAMED_DIMS[gold["ckpt"]["dims"]], gold["adapter"])
    rt = LlamaRuntime(ckpt, "cuda", max_tokens=4096, max_seqs=16, accept_model_types=("mistral",), adapter_dir=adir)
    tok = AutoTokenizer.from_pretrained(tokdir)
    cls = R1ListwiseLlmRanker.with_draft_tokens(kd)
    for case in gold["cases"]:
        run(cls.from_runtime(rt, tok, gold["prompt"], window_size=case["window_size"], step_size=case["step_size"],
                             num_repeat=case["num_repeat"], max_new_tokens=case["max_new_tokens"]), case)
    rt.engine.close()
