"""Sampling for the Llama path, host side (no GPU): the Philox reference against the published known answers, the fp64 filter
reference (tests/_sampling_ref.py) against the installed transformers' logits warpers, the generation settings and the ranker's
plumbing of sample_seed on a stand-in runtime."""
import json
import logging

import numpy as np
import pytest

import _sampling_ref as ref


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr,key,want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    got = ref.philox4x32_10(np.array([_words(ctr)]), np.array([_words(key)]))[0]
    assert [int(w) for w in got] == _words(want)


def test_uniform_is_the_first_word_on_the_24_bit_grid():
    seeds = np.array([0, 0x299f31d0a4093822, 2 ** 64 - 1], np.uint64)
    u = ref.uniform(seeds, [0, 0x243f6a88, 7])
    assert u[0] == (0x6627e8d5 >> 8) * 2.0 ** -24
    x0 = ref.philox4x32_10(np.array([[0x243f6a88, 0, 0, 0]]), np.array([[0xa4093822, 0x299f31d0]]))[0, 0]
    assert u[1] == (int(x0) >> 8) * 2.0 ** -24
    assert np.all((u >= 0) & (u < 1)) and np.all(u * 2 ** 24 == np.floor(u * 2 ** 24))


@pytest.mark.parametrize("T,k,p", [(0.6, 50, 0.9), (1.0, 0, 0.6), (0.9, 5, 1.0)])
def test_filter_reference_keeps_what_transformers_keeps(T, k, p):
    torch = pytest.importorskip("torch")
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    rng = np.random.default_rng(20261019)
    x = (rng.normal(0.0, 2.5, (24, 1000))).astype(np.float32)
    s = torch.from_numpy(x.copy())
    ids = torch.zeros((x.shape[0], 1), dtype=torch.long)
    if T != 1.0:
        s = TemperatureLogitsWarper(T)(ids, s)
    if k > 0:
        s = TopKLogitsWarper(k)(ids, s)
    if p < 1.0:
        s = TopPLogitsWarper(p)(ids, s)
    hf_kept = torch.isfinite(s).numpy()
    for r in range(x.shape[0]):
        row = ref.filter_row(x[r], T, k, p)
        assert np.array_equal(row.kept, hf_kept[r]), (r, int(row.kept.sum()), int(hf_kept[r].sum()))
        assert row.kept.sum() >= 1 and row.kept[np.argmax(x[r])]


def test_reference_draw_walks_the_cdf_in_vocabulary_order():
    x = np.array([0.0, -np.inf, 1.0, 1.0, -3.0, 0.5], np.float32)
    row = ref.filter_row(x, 1.0, 4, 1.0)
    assert list(np.flatnonzero(row.kept)) == [0, 2, 3, 5]
    w = np.exp(np.array([0.0, 1.0, 1.0, 0.5]) - 1.0)
    assert np.allclose(row.Z, w.sum())
    cuts = np.cumsum(w) / w.sum()
    assert [int(row.draw(u)) for u in (0.0, cuts[0] - 1e-9, cuts[0] + 1e-9, cuts[1] + 1e-9, cuts[2] + 1e-9, 1 - 1e-12)] == [0, 0, 2, 3, 5, 5]
    tie = ref.filter_row(np.full(7, 1.5, np.float32), 0.7, 3, 0.5)            # ties at both thresholds: every id stays
    assert tie.kept.all() and tie.k_gap == 0


# ---- generation settings ---------------------------------------------------------------------------------------------------
def test_generation_settings_carry_the_sampling_parameters(tmp_path):
    from llmrankers._runtime import generation_plan, read_generation_settings, sampling_plan

    def settings(gc=None):
        d = tmp_path / f"c{len(list(tmp_path.iterdir()))}"
        d.mkdir()
        if gc is not None:
            (d / "generation_config.json").write_text(json.dumps(gc))
        return read_generation_settings(str(d), {"eos_token_id": 2})

    class RT:
        def __init__(self, g):
            self.generation = g

    s = settings()
    assert (s["temperature"], s["top_k"], s["top_p"], s["do_sample"]) == (1.0, 50, 1.0, False)        # HF's GenerationConfig defaults
    assert sampling_plan(RT(s)) is None
    s = settings({"do_sample": True, "temperature": 0.6, "top_p": 0.9})                                # Llama-3-Instruct's
    assert (s["temperature"], s["top_k"], s["top_p"], s["do_sample"]) == (0.6, 50, 0.9, True)
    assert sampling_plan(RT(s)) == (0.6, 50, 0.9)
    s = settings({"do_sample": False, "temperature": 0.6, "top_k": 7})
    assert s["top_k"] == 7 and sampling_plan(RT(s)) is None
    # a dict built by hand (the stand-in runtimes of the other test modules) has no such keys
    hand = {"eos_token_ids": [2], "pad_token_id": 2, "max_new_tokens": 7, "max_length": None, "do_sample": True}
    assert sampling_plan(RT(hand)) == (1.0, 50, 1.0)
    assert generation_plan(RT(dict(hand, do_sample=False)), [5]) == {"max_new": 7, "max_total": 0, "eos_ids": [2], "pad_id": 2}
    assert generation_plan(RT(settings({"max_new_tokens": 7})), [5]) == {"max_new": 7, "max_total": 0, "eos_ids": [2], "pad_id": 2}


# ---- the ranker's plumbing -------------------------------------------------------------------------------------------------
class _Tok:
    eos_token_id = 2

    def apply_chat_template(self, messages, add_generation_prompt=True, return_dict=False, **kw):
        return [1] + [3 + (len(m["content"]) % 50) for m in messages]

    def decode(self, ids, skip_special_tokens=True):
        return "[2] > [1] > [3]"


class _Runtime:
    """a runtime that records how it is called; `generate` has the greedy stand-ins' signature plus the trailing seeds"""
    model_type = "llama"

    def __init__(self, do_sample):
        self.generation = {"eos_token_ids": [2], "pad_token_id": 0, "max_new_tokens": 4, "max_length": None, "do_sample": do_sample,
                           "temperature": 0.6, "top_k": 50, "top_p": 0.9}
        self.calls, self.sampling = [], []

    def set_sampling(self, *a):
        self.sampling.append(a)
        self.sampling_on = a[0] > 0

    def generate(self, *args, **kw):
        self.calls.append((args, kw))
        return np.full((len(args[0]), args[1]), 5, np.int32)


def _rank(rt, **kw):
    from llmrankers.listwise import ListwiseLlmRanker
    from llmrankers.rankers import SearchResult
    rk = ListwiseLlmRanker.from_runtime(rt, _Tok(), window_size=3, step_size=1, **kw)
    docs = [SearchResult(docid=str(i), score=None, text=f"passage {i} " * (i + 1)) for i in range(5)]
    rk.rerank("a query", docs)
    return rk


def test_ranker_without_sample_seed_calls_what_it_called_before(caplog):
    with caplog.at_level(logging.WARNING, logger="llmrankers"):
        rt = _Runtime(do_sample=True)
        _rank(rt)
    assert rt.sampling == [] and len(rt.calls) == 3
    for args, kw in rt.calls:                                   # (ids, max_new, eos_ids, pad_id, max_total), nothing by keyword
        assert kw == {} and len(args) == 5 and args[1:] == (4, [2], 0, 0)
    assert sum("greedily" in r.getMessage() for r in caplog.records) == 1


def test_ranker_with_sample_seed_sets_the_checkpoints_parameters_and_seeds_every_compare(caplog):
    with caplog.at_level(logging.WARNING, logger="llmrankers"):
        a, b, c = _Runtime(True), _Runtime(True), _Runtime(True)
        _rank(a, sample_seed=11)
        _rank(b, sample_seed=11)
        _rank(c, sample_seed=12)
    assert not any("greedily" in r.getMessage() for r in caplog.records)
    assert a.sampling == [(0.6, 50, 0.9)]
    seeds = [[kw["seeds"] for _, kw in rt.calls] for rt in (a, b, c)]
    assert all(len(s) == 3 and all(len(row) == 1 for row in s) for s in seeds)
    import random
    rng = random.Random(11)
    assert seeds[0] == [[rng.getrandbits(64)] for _ in range(3)]                 # compare order, one stream per ranker
    assert seeds[0] == seeds[1] and seeds[0] != seeds[2]
    assert len({s[0] for s in seeds[0]}) == 3
    for args, kw in a.calls:
        assert len(args) == 5 and set(kw) == {"seeds"}


def test_sample_seed_on_a_greedy_checkpoint_changes_nothing(caplog):
    with caplog.at_level(logging.WARNING, logger="llmrankers"):
        rt = _Runtime(do_sample=False)
        _rank(rt, sample_seed=11)
    assert rt.sampling == [] and all(kw == {} for _, kw in rt.calls) and not caplog.records


def test_rerank_many_draws_one_seed_per_window_in_call_order():
    from llmrankers.listwise import ListwiseLlmRanker
    from llmrankers.rankers import SearchResult
    rt = _Runtime(True)
    rk = ListwiseLlmRanker.from_runtime(rt, _Tok(), window_size=3, step_size=1, sample_seed=5)
    items = [(f"q{j}", [SearchResult(docid=str(i), score=None, text=f"p{i}") for i in range(4)]) for j in range(2)]
    rk.rerank_many(items)
    import random
    rng = random.Random(5)
    for args, kw in rt.calls:
        assert kw["seeds"] == [rng.getrandbits(64) for _ in args[0]]


# ---- the pool --------------------------------------------------------------------------------------------------------------
class _Session:
    def __init__(self, n_slots):
        self.n_slots, self.busy, self.admits = n_slots, set(), []

    def admit(self, *args, **kw):
        self.admits.append((args, kw))
        self.busy.update(args[1])

    def run(self):
        return sorted(self.busy), 1

    def read(self, slot):
        self.busy.discard(slot)
        return np.array([7, 2], np.int32)

    def close(self):
        pass


def test_pool_passes_seeds_only_when_its_requests_carry_them():
    from llmrankers._runtime import DecodePool
    made = []

    def open_session(max_len):
        made.append(_Session(2))
        return made[-1]

    pool = DecodePool(open_session, 2, 4096, 8)
    pool.submit("a", [1, 2, 3], 4)
    pool.submit("b", [1, 2], 4)
    assert sorted(k for k, _ in pool.wait()) == ["a", "b"]
    (args, kw), = made[0].admits
    assert kw == {} and len(args) == 3                          # the greedy call shape, positionally
    pool.submit("c", [1, 2, 3], 4, seed=99)
    pool.submit("d", [1, 2], 4, seed=100)
    with pytest.raises(ValueError, match="seed"):
        pool.submit("e", [1], 4)
    pool.wait()
    args, kw = made[0].admits[1]
    assert kw == {"seeds": [99, 100]} and len(args) == 3
