"""The decoding session of the Llama engine (rk_llama_session_*): fixed cache slots, prompts admitted into free slots while the other
slots decode, one replayed step graph.  The property everything rests on: a prompt's tokens from a session equal, token for token,
what rk_llama_generate gives for that prompt alone - whatever shares the session, whichever slot it lands in, whatever the slot held
before.  On toy-qwen2 (7 query heads on 1 kv head, q / k / v biases) and toy-llama (2 query heads per kv head)."""
import itertools
import os
import random

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu

LENS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 300)
# max_new cycles through 1, 2, 5, 40 in the order that gives 127 + 5 and 128 + 2 (rows that cross a 128-key chunk boundary while
# they decode) and 255 + 40
MAX_NEW = tuple((40, 5, 2, 1)[i % 4] for i in range(len(LENS)))
CAP, MAX_LEN, PAD = 40, 384, 0


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 4096)
    kw.setdefault("max_seqs", 16)
    return RkLlamaEngine(dims, device=0, **kw).load_state(state.items())


def _alone(eng, prompt, max_new, eos):
    """the reference: rk_llama_generate on the prompt alone -> its new tokens, the EOS that ended it included"""
    toks, steps = eng.generate([prompt], max_new, eos, PAD)
    row = [int(t) for t in toks[0, :steps]]
    stop = next((i for i, t in enumerate(row) if t in eos), None)
    return row if stop is None else row[:stop + 1]


def _fifo(eng, prompts, max_new, n_slots, eos, max_len=MAX_LEN, cap=CAP):
    """The requests in order through a session of n_slots: free slots are filled (lowest first, ONE admit) whenever there are any,
    then the session runs until something finishes.  -> ({request: tokens}, admits made while another slot was mid-row, steps)"""
    got, refills, nxt = {}, 0, 0
    with eng.session(n_slots, max_len, cap, eos, PAD) as s:
        owner = {}
        while nxt < len(prompts) or s.busy:
            free = s.free_slots()
            take = list(range(nxt, min(nxt + len(free), len(prompts))))
            if take:
                # every busy slot is mid-row here: the last run's finished slots were all read
                refills += bool(s.busy)
                slots = free[:len(take)]
                s.admit([prompts[r] for r in take], slots, [max_new[r] for r in take])
                owner.update(zip(slots, take))
                nxt += len(take)
            finished, _ = s.run()
            assert finished, "a run with busy slots must end with a finish"
            for slot in finished:
                got[owner.pop(slot)] = [int(t) for t in s.read(slot)]
        assert s.run() == ([], 0)                                     # nothing active: no step
        steps = s.steps
    return got, refills, steps


@pytest.fixture(scope="module", params=["toy-qwen2", "toy-llama"])
def model(request):
    """dims, state, the ten prompts, their no-EOS references and the EOS set taken from them with its references - computed once"""
    from llmrankers import _synth
    dims = _synth.NAMED_DIMS[request.param]
    state = _synth.synth_state_dict(dims, seed=929)
    base = _synth.synth_token_batch(1, 300, 300, dims.vocab, seed=17)[0]
    prompts = [list(base[:n]) for n in LENS]
    eng = _engine(dims, state)
    plain = [_alone(eng, p, m, []) for p, m in zip(prompts, MAX_NEW)]
    assert [len(r) for r in plain] == list(MAX_NEW)
    # column 0 of one prompt (it ends at admit), column 3 of a 5-token one (early), column 20 of a 40-token one (late)
    eos = sorted({plain[2][0], plain[5][3], plain[8][20]})
    stopped = [_alone(eng, p, m, eos) for p, m in zip(prompts, MAX_NEW)]
    eng.close()
    assert len(stopped[2]) == 1 and len(stopped[5]) <= 4 and len(stopped[8]) <= 21
    assert all(r[-1] in eos or len(r) == m for r, m in zip(stopped, MAX_NEW))
    return dims, state, prompts, {"plain": ([], plain), "eos": (eos, stopped)}


@pytest.mark.parametrize("which", ["plain", "eos"])
def test_session_tokens_equal_the_prompt_alone(model, which):
    """Check 1: the same FIFO schedule with 1, 4 and 16 slots: every request's tokens and count equal rk_llama_generate's for the
    prompt alone, without EOS and with an EOS set that ends rows at admit, early and late (the EOS is part of the row)."""
    dims, state, prompts, refs = model
    eos, want = refs[which]
    eng = _engine(dims, state)
    refills = {}
    for n_slots in (1, 4, 16):
        got, refills[n_slots], steps = _fifo(eng, prompts, MAX_NEW, n_slots, eos)
        for r, w in enumerate(want):
            assert got[r] == w, (which, n_slots, r, LENS[r], got[r], w)
        print(f"{which}: {n_slots} slots, {steps} steps, {refills[n_slots]} admits beside running rows")
    # the session is gone: the engine's other calls are back, and give what they gave
    assert _alone(eng, prompts[3], MAX_NEW[3], eos) == want[3]
    eng.close()
    assert refills[4] >= 2, refills                                   # else the schedule did not test refill
    assert refills[1] == 0 and refills[16] == 0


def test_run_step_counts_follow_the_host_model(model):
    """The steps a plain session's run() issues, its finished set and the stats' columns and step total, after every run, against a
    host model made from the alone-references only.  The FIFO schedule of _fifo with 4 slots and with 1, max_steps cycling through
    1, 3 and unlimited, on the EOS set (a row that ends at its admit, one early, one late).  The model: nothing is issued while a
    finish is unreported or nothing is active; else min(max_steps, live, f + 2) steps, live = the most columns an active slot may
    still take, f = the steps before the first finish - one step is queued behind the finish before the host sees its word."""
    dims, state, prompts, refs = model
    eos, want = refs["eos"]
    eng = _engine(dims, state)
    branches = set()
    for n_slots in (4, 1):
        budgets = itertools.cycle((1, 3, 1 << 30))
        with eng.session(n_slots, MAX_LEN, CAP, eos, PAD) as s:
            owner, col, untold, total, nxt = {}, {}, set(), 0, 0      # per busy slot: its request, its column; finishes not yet reported
            while nxt < len(prompts) or s.busy:
                free = s.free_slots()
                take = list(range(nxt, min(nxt + len(free), len(prompts))))
                if take:
                    slots = free[:len(take)]
                    s.admit([prompts[r] for r in take], slots, [MAX_NEW[r] for r in take])
                    for slot, r in zip(slots, take):
                        owner[slot], col[slot] = r, 1                 # the admit's token is column 0
                        if len(want[r]) == 1:
                            untold.add(slot)
                    nxt += len(take)
                max_steps = next(budgets)
                n = {b: len(want[owner[b]]) for b in col}
                active = [b for b in col if col[b] < n[b]]
                steps = 0
                if active and not untold:
                    live = max(MAX_NEW[owner[b]] - col[b] for b in active)
                    f = min(n[b] - col[b] - 1 for b in active)
                    steps = min(max_steps, live, f + 2)
                    if steps == max_steps < min(live, f + 2):
                        branches.add("limit")
                    if steps == f + 2 < min(max_steps, live):
                        branches.add("queued")
                    for b in active:
                        col[b] = min(col[b] + steps, n[b])
                    untold = {b for b in active if col[b] == n[b]}
                total += steps
                finished, issued = s.run(max_steps)
                st = s.stats()
                print(f"{n_slots} slots, run({max_steps}): {issued} steps (model {steps}), finished {finished} (model {sorted(untold)})")
                assert issued == steps, (n_slots, max_steps, issued, steps)
                assert finished == sorted(untold), (n_slots, finished, untold)
                assert [int(c) for c in st["slot_cols"]] == [col.get(b, 0) for b in range(n_slots)]
                assert st["steps"] == total == s.steps
                for slot in finished:
                    assert [int(t) for t in s.read(slot)] == want[owner[slot]]
                    del owner[slot], col[slot]
                untold = set()
            assert s.run() == ([], 0)
    eng.close()
    assert branches == {"limit", "queued"}, branches                  # else the schedule stopped exercising one of them


def test_slot_reuse_reads_no_stale_keys(model):
    """Check 2: one slot: a 300-token prompt with 40 new tokens, then a 2-token prompt in the same slot == its standalone run"""
    dims, state, prompts, refs = model
    eng = _engine(dims, state)
    short, long_ = prompts[1], prompts[9]
    want = [_alone(eng, long_, 40, []), _alone(eng, short, 40, [])]
    got, _, _ = _fifo(eng, [long_, short], [40, 40], 1, [])
    eng.close()
    assert got[0] == want[0] and got[1] == want[1]


def test_rowscale_consumer_path_with_idle_slots():
    """Check 3: hidden 2 304 = 72 block sums per row, more than the consumer's epilogue stages (64): the step's GEMMs take their row
    factors from rowscale_kernel.  4 slots, 2 prompts (two slots idle throughout): tokens equal the prompts alone."""
    from llmrankers import _synth
    dims = _synth.LlamaDims(vocab=512, hidden=2304, n_heads=18, n_kv_heads=2, head_dim=128, intermediate=512, n_layers=1)
    state = _synth.synth_state_dict(dims, seed=31)
    prompts = [list(s) for s in _synth.synth_token_batch(2, 70, 140, dims.vocab, seed=3)]
    eng = _engine(dims, state, max_tokens=1024, max_seqs=4)
    want = [_alone(eng, p, m, []) for p, m in zip(prompts, (12, 7))]
    got, _, _ = _fifo(eng, prompts, [12, 7], 4, [], max_len=256, cap=16)
    eng.close()
    assert [got[0], got[1]] == want


def test_contract(model):
    """Check 4: refused admits leave the session working; run with nothing active; the engine's other Llama calls during a session;
    a second open"""
    from llmrankers._engine import RkError
    dims, state, prompts, refs = model
    _, want = refs["plain"]
    eng = _engine(dims, state)
    logits = eng.last_logits([prompts[3]], [1, 2, 3])
    first = eng.greedy1([prompts[3]])
    s = eng.session(4, 320, CAP, [], PAD)
    assert s.run() == ([], 0)

    def refused(code, seqs, slots, max_new):
        with pytest.raises(RkError) as ex:
            s.admit(seqs, slots, max_new)
        assert ex.value.code == code, (ex.value.code, str(ex.value))

    s.admit([prompts[5]], [1], [MAX_NEW[5]])
    refused(-4, [prompts[0]], [1], [3])                               # busy
    refused(-1, [prompts[0], prompts[1]], [2, 2], [3, 3])             # named twice
    refused(-1, [prompts[0]], [4], [3])                               # out of range
    refused(-6, [prompts[9]], [0], [CAP])                             # len + max_new > max_len (300 + 40 > 320)
    refused(-6, [prompts[0]], [0], [CAP + 1])                         # max_new > max_new_cap
    assert s.busy == {1}
    for call in (lambda: eng.generate([prompts[0]], 2, [], PAD), lambda: eng.greedy1([prompts[0]]),
                 lambda: eng.last_logits([prompts[0]], [1, 2])):
        with pytest.raises(RkError) as ex:
            call()
        assert ex.value.code == -4
    with pytest.raises(RkError) as ex:
        eng.session(2, 256, 8, [], PAD)
    assert ex.value.code == -4
    with pytest.raises(RkError) as ex:                                # a slot that is still decoding cannot be read
        s.read(1)
    assert ex.value.code == -4
    s.admit([prompts[6], prompts[0]], [0, 3], [MAX_NEW[6], MAX_NEW[0]])
    got = {}
    owner = {1: 5, 0: 6, 3: 0}
    while s.busy:
        finished, _ = s.run()
        assert finished
        for slot in finished:
            got[owner[slot]] = [int(t) for t in s.read(slot)]
    assert got == {r: want[r] for r in (5, 6, 0)}
    s.close()
    s.close()                                                         # (closing twice is harmless)
    np.testing.assert_array_equal(eng.last_logits([prompts[3]], [1, 2, 3]).view(np.uint32), logits.view(np.uint32))
    np.testing.assert_array_equal(eng.greedy1([prompts[3]]), first)
    assert _alone(eng, prompts[5], MAX_NEW[5], []) == want[5]
    with pytest.raises(RkError) as ex:                                # capacities of the engine
        eng.session(17, MAX_LEN, CAP, [], PAD)
    assert ex.value.code == -6
    with pytest.raises(RkError) as ex:
        eng.session(4, 4097, CAP, [], PAD)
    assert ex.value.code == -6
    eng.close()


def test_rerank_many_on_the_device(tmp_path):
    """Check 5: RankR1SetwiseLlmRanker.rerank_many through the pool on the toy-qwen2 engine (the recorded Rank-R1 checkpoint with its
    adapter: completions that name labels): 5 queries x 12 passages, three stop ids that the completions contain (rows of different
    lengths) == per-query rerank under the per-query generators: rankings, the callers' lists and all three counters; the same with
    two permutations per compare for two of the queries."""
    import json
    from transformers import AutoTokenizer
    from llmrankers import _synth
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    with open(os.path.join(GOLD, "rankr1_cases.json")) as f:
        gold = json.load(f)
    path, adir = str(tmp_path / "toy-qwen2"), str(tmp_path / "adapter")
    _synth.write_checkpoint(path, gold["ckpt"], os.path.join(GOLD, gold["tokenizer"]))
    _synth.write_lora_adapter(adir, _synth.NAMED_DIMS[gold["ckpt"]["dims"]], gold["adapter"])
    rt = LlamaRuntime(path, "cuda", max_tokens=8192, max_seqs=8, accept_model_types=("qwen2",), adapter_dir=adir)
    eng = rt.engine
    tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, "tok_qwen"))
    words = sorted({w for case in gold["cases"] for _, text in case["docs"] for w in text.split()})
    rs = random.Random(5)

    def items(n_queries):
        return [(" ".join(rs.sample(words, 4)),
                 [SearchResult(docid=f"q{q}d{d}", score=None, text=" ".join(rs.sample(words, 9))) for d in range(12)]) for q in range(n_queries)]

    def ranker(num_permutation):
        return RankR1SetwiseLlmRanker.from_runtime(rt, tok, os.path.join(GOLD, "rankr1_prompt.toml"), num_child=3, k=3,
                                                   max_new_tokens=24, num_permutation=num_permutation)

    def one_by_one(rk, its, seed):
        """rerank per query with the generator rerank_many gives it: seeds drawn in item order from the seeded module stream"""
        random.seed(seed)
        seeds = [random.getrandbits(64) for _ in its]
        out = []
        for (query, ranking), s in zip(its, seeds):
            rk.compare_rng = random.Random(s)
            res = rk.rerank(query, ranking)
            out.append(([d.docid for d in res], [d.docid for d in ranking],
                        (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens)))
        rk.compare_rng = None
        return out

    # stop ids the completions contain: from one standalone compare's new tokens
    rt.generation["eos_token_ids"] = []
    rk = ranker(1)
    its = items(5)
    seen = []
    real = rt.generate
    rt.generate = lambda *a, **k: seen.append(np.asarray(real(*a, **k))) or seen[-1]
    random.seed(3)
    rk.compare(its[0][0], its[0][1][:4])
    rt.generate = real
    row = [int(t) for t in seen[0][0]]
    rt.generation["eos_token_ids"] = sorted({row[2], row[9], row[17]})
    for num_permutation, n_queries in ((1, 5), (2, 2)):
        rk = ranker(num_permutation)
        base = its[:n_queries]
        copy = lambda: [(q, list(r)) for q, r in base]                # noqa: E731
        want = one_by_one(rk, copy(), 41)
        many = copy()
        random.seed(41)
        results, counters = rk.rerank_many(many)
        got = [([d.docid for d in res], [d.docid for d in ranking], tuple(c)) for res, (_, ranking), c in zip(results, many, counters)]
        assert got == want, num_permutation
        assert len({c[2] / c[0] for _, _, c in want}) > 1             # completions of different lengths
    eng.close()
