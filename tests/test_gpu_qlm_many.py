"""rk_t5_qlm_many on the GPU: several queries' passages in one engine call, every passage scored against its OWN query's
labels.  The contract under test: a sequence's score is BIT FOR BIT what rk_t5_qlm gives that sequence with those labels,
whatever shares the call and in whatever order - across every class of label counts (1 | 2..4 | 5..16 | 17..64 | 65..), with
the matrix-core and the staged attention kernels, at toy and at flan-t5-xl dimensions, and through the ranker."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, load_state

pytestmark = pytest.mark.gpu

# label counts of the 24 sequences: every class edge {1, 2, 4, 5, 16, 17, 33, 64, 65, 72} plus repeats; the even positions
# alone (the "every second sequence" call) still hold more than 4 rows of the class 2..4
COUNTS = [1, 2, 4, 5, 16, 17, 33, 64, 65, 72, 2, 3, 4, 1, 9, 40, 17, 64, 66, 3, 12, 30, 4, 8]
LONG_PROMPTS = {3: 205, 6: 230, 7: 200, 9: 210, 16: 250}      # above 192 tokens: the staged cross-attention kernels' sequences


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _ragged_inputs(vocab, seed):
    rng = np.random.default_rng(seed)
    seqs, labels = [], []
    for i, n in enumerate(COUNTS):
        L = LONG_PROMPTS.get(i, int(rng.integers(5, 120)))
        seqs.append(rng.integers(2, vocab, size=L).astype(np.int32).tolist())
        labels.append(rng.integers(2, vocab, size=n).astype(np.int32).tolist())
    return seqs, labels


def _few_row_class_rows(counts):
    return sum(n for n in counts if 2 <= n <= 4)


@pytest.fixture(scope="module")
def toy72(ckpt_dirs):
    from llmrankers._engine import RkEngine
    out = {}
    for name in ("ckpt_gated_untied", "ckpt_relu_tied"):
        dims, state = load_state(ckpt_dirs[name])
        out[name] = (dims, state, RkEngine(dims, device=0, max_tokens=8192, max_seqs=64, max_dec_len=72).load_state(state.items()))
    yield out
    for _, _, e in out.values():
        e.close()


def _check_bit_equal_to_single_label_calls(eng, seqs, labels, what):
    # the reference: rk_t5_qlm on THREE copies of the sequence - more than 4 rows for every count >= 2, so the pass stays
    # off the few-row GEMV family (the one documented exception to batch independence)
    want = np.array([eng.qlm([s, s, s], l)[0] for s, l in zip(seqs, labels)], dtype=np.float32)
    assert np.isfinite(want).all()
    got = eng.qlm_many(seqs, labels)
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (what, "whole call", [(int(i), COUNTS[i], float(got[i]), float(want[i])) for i in bad[:8]])
    perm = np.random.default_rng(5).permutation(len(seqs))
    got_p = eng.qlm_many([seqs[i] for i in perm], [labels[i] for i in perm])
    bad = np.nonzero(_bits(got_p) != _bits(want[perm]))[0]
    assert bad.size == 0, (what, "shuffled", [(int(perm[i]), COUNTS[perm[i]]) for i in bad[:8]])
    half = list(range(0, len(seqs), 2))
    assert _few_row_class_rows([COUNTS[i] for i in half]) > 4
    got_h = eng.qlm_many([seqs[i] for i in half], [labels[i] for i in half])
    bad = np.nonzero(_bits(got_h) != _bits(want[half]))[0]
    assert bad.size == 0, (what, "every second sequence", [(half[i], COUNTS[half[i]]) for i in bad[:8]])
    return want


@pytest.mark.parametrize("ckpt", ["ckpt_gated_untied", "ckpt_relu_tied"])
def test_qlm_many_bit_equal_to_qlm_for_every_label_count_class(toy72, ckpt):
    dims, _, eng = toy72[ckpt]
    assert {1, 2, 4, 5, 16, 17, 33, 64, 65, 72} <= set(COUNTS) and len(COUNTS) == 24 and _few_row_class_rows(COUNTS) > 4
    seqs, labels = _ragged_inputs(dims.vocab, seed=11)
    _check_bit_equal_to_single_label_calls(eng, seqs, labels, "default kernels")
    for key in ("dec_cross_mfma", "dec_attn_seq"):        # the cross-check kernels' ragged forms
        eng.set_option(key, 0)
        try:
            _check_bit_equal_to_single_label_calls(eng, seqs, labels, f"{key} = 0")
        finally:
            eng.set_option(key, 1)


def test_qlm_many_argument_errors(toy72):
    from llmrankers._engine import RkError
    dims, _, eng = toy72["ckpt_gated_untied"]
    seqs = [[5, 6, 7], [8, 9]]
    for labels, code in (([[3], []], -6), ([[3], [4] * 73], -6), ([[3], [dims.vocab]], -1)):
        with pytest.raises(RkError) as ei:
            eng.qlm_many(seqs, labels)
        assert ei.value.code == code
    with pytest.raises(ValueError):
        eng.qlm_many(seqs, [[3]])
    assert np.isfinite(eng.qlm_many(seqs, [[3], [4, 5]])).all()       # the engine is usable after the refusals


@pytest.mark.parametrize("ckpt", ["ckpt_gated_untied", "ckpt_relu_tied"])
def test_qlm_many_vs_fp32_oracle_per_class(toy72, ckpt):
    """Measured, not bounded here: parity with the reference is rk_t5_qlm's (bit-equality above) and the ranker-level tests
    below hold the grouped path to the recorded references at the tolerances the suite already uses."""
    from oracle.t5_numpy import T5Oracle
    dims, state, eng = toy72[ckpt]
    seqs, labels = _ragged_inputs(dims.vocab, seed=11)
    got = eng.qlm_many(seqs, labels)
    orc = T5Oracle(dims, state)
    want = np.array([orc.qlm([s], l)[0] for s, l in zip(seqs, labels)], dtype=np.float64)
    assert np.isfinite(got).all()
    for lo, hi in ((1, 1), (2, 4), (5, 16), (17, 64), (65, 72)):
        idx = [i for i, n in enumerate(COUNTS) if lo <= n <= hi]
        err = np.abs(got[idx] - want[idx])
        print(f"[qlm_many vs oracle] {ckpt} label counts {lo}..{hi}: {len(idx)} sequences, max abs error {err.max():.3e}, "
              f"max relative {np.max(err / np.abs(want[idx])):.3e}")


def test_rerank_many_qlm_on_the_recorded_cases_is_one_engine_call_per_group(ckpt_dirs):
    from transformers import T5Tokenizer
    from llmrankers._runtime import T5Runtime
    from llmrankers.pointwise import PointwiseLlmRanker
    from llmrankers.rankers import SearchResult
    with open(os.path.join(GOLD, "rerank_cases.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["kind"] == "pointwise" and c["method"] == "qlm" and not c.get("raises")]
    groups = {}
    for c in cases:
        groups.setdefault((c["ckpt"], c["batch_size"]), []).append(c)
    assert len(groups) >= 4
    for ckpt in sorted({k[0] for k in groups}):
        rt, tok = T5Runtime(ckpt_dirs[ckpt], "cuda", max_tokens=8192, max_seqs=64, max_dec_len=40), T5Tokenizer.from_pretrained(ckpt_dirs[ckpt])
        try:
            calls = {"qlm": 0, "qlm_many": 0}
            eng_qlm, eng_many = rt.engine.qlm, rt.engine.qlm_many
            rt.engine.qlm = lambda *a: (calls.__setitem__("qlm", calls["qlm"] + 1), eng_qlm(*a))[1]
            rt.engine.qlm_many = lambda *a: (calls.__setitem__("qlm_many", calls["qlm_many"] + 1), eng_many(*a))[1]
            for (ck, bs), grp in groups.items():
                if ck != ckpt:
                    continue
                calls.update(qlm=0, qlm_many=0)
                rk = PointwiseLlmRanker.from_runtime(rt, tok, method="qlm", batch_size=bs)
                rankings = [[SearchResult(docid=d, score=s, text=t) for d, s, t in c["input"]] for c in grp]
                got, counters = rk.rerank_many([(c["query"], r) for c, r in zip(grp, rankings)])
                assert calls == {"qlm": 0, "qlm_many": 1}, calls
                for c, res, cnt in zip(grp, got, counters):
                    want = dict((d, s) for d, s in c["result"])
                    err = max(abs(r.score - want[r.docid]) for r in res)
                    print(f"[rerank_many qlm] {ckpt} batch_size {bs}: max abs error vs the recorded reference {err:.3e}")
                    assert err < 5e-2, (ckpt, bs, err)
                    assert list(cnt) == c["counters"]
        finally:
            rt.engine.close()


def test_flan_t5_xl_dims_grouped_qlm_across_the_16_17_line_equals_one_query_at_a_time():
    from transformers import T5Tokenizer
    from llmrankers import _synth
    from llmrankers._engine import RkEngine
    from llmrankers._runtime import T5Runtime
    from llmrankers.pointwise import PointwiseLlmRanker
    from llmrankers.rankers import SearchResult
    with open(os.path.join(GOLD, "xl_qlm_query.json")) as f:
        gold = json.load(f)
    tok = T5Tokenizer.from_pretrained(os.path.join(GOLD, "tok"))
    words = gold["query"].split()
    queries = [gold["query"]] + [" ".join((words * 3)[k:k + n]) for k, n in ((1, 18), (3, 24), (5, 30))]
    n_labels = [len(tok.encode(f"<pad> {q}", add_special_tokens=False)) for q in queries]
    assert n_labels[0] == 15 and all(17 <= n <= 33 for n in n_labels[1:]), n_labels
    dims = _synth.NAMED_DIMS[gold["dims"]]
    state = _synth.synth_state_dict(dims, seed=gold["weight_seed"], threads=min(32, os.cpu_count() or 8))
    eng = RkEngine(dims, 0, max_tokens=16384, max_seqs=128, max_dec_len=48).load_state(state.items())
    del state
    n = len(gold["docs"])
    bs = gold["batch_size"]

    def fresh():
        return [[SearchResult(docid=f"d{i}", score=float(n - i), text=t) for i, t in enumerate(gold["docs"])] for _ in queries]

    try:
        rt = T5Runtime.from_engine(eng, dims)
        one = PointwiseLlmRanker.from_runtime(rt, tok, method="qlm", batch_size=bs)
        want, want_cnt = [], []
        for q, ranking in zip(queries, fresh()):
            res = one.rerank(q, ranking)
            want.append(([d.docid for d in res], _bits([d.score for d in ranking]).tolist()))
            want_cnt.append((one.total_compare, one.total_prompt_tokens, one.total_completion_tokens))
        rankings = fresh()
        got, cnt = PointwiseLlmRanker.from_runtime(rt, tok, method="qlm", batch_size=bs).rerank_many(list(zip(queries, rankings)))
        assert [([d.docid for d in res], _bits([d.score for d in ranking]).tolist()) for res, ranking in zip(got, rankings)] == want
        assert cnt == want_cnt
        ref = np.array(gold["scores"])
        err = np.abs(np.array([d.score for d in rankings[0]]) - ref)
        rel = float(err.max() / np.abs(ref).max())
        print(f"[xl grouped qlm] label counts {n_labels}: golden query max abs error {err.max():.4f}, relative {rel:.2e}")
        assert rel < 2e-4, (err.max(), rel)
        assert list(cnt[0]) == gold["counters"]
        # candidate sharding over a one-rank communicator: the same bits, ONE gather for the four queries
        eng.comm_init(eng.comm_unique_id(), 0, 1, 1024)
        gathers = []
        real_gather = eng.comm_all_gather_appended
        eng.comm_all_gather_appended = lambda nf: (gathers.append(nf), real_gather(nf))[1]
        rankings = fresh()
        sharded = PointwiseLlmRanker.from_runtime(rt, tok, method="qlm", batch_size=bs, shard_candidates=True)
        got, cnt = sharded.rerank_many(list(zip(queries, rankings)))
        assert len(gathers) == 1, gathers
        assert [([d.docid for d in res], _bits([d.score for d in ranking]).tolist()) for res, ranking in zip(got, rankings)] == want
        assert cnt == want_cnt
    finally:
        if getattr(eng, "comm_capacity", 0):
            eng.comm_destroy()
        eng.close()
