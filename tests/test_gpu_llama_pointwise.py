"""Pointwise scoring on decoder-only checkpoints on the HIP engine: rk_llama_qlm against the fp64 continuation log-likelihood of
tests/_llama_pointwise_ref.py on six toy engines (Llama, Llama with a vocabulary that ends inside a 32-column block, Qwen2 with
biases and seven query heads per kv head, Qwen3 with the q / k head norm, Mistral with a window of 8 keys, 64-wide heads), bit-exact
independence of what shares a call, the one-label case against the old head path (rk_llama_last_logits), the refusals and what they
leave behind, and PointwiseLlmRanker end to end on LlamaRuntime.

Tolerances (derived in _llama_pointwise_ref.py from BOUND = 4e-3 x logit scale, the Llama prefill's bound): a qlm score
2 n_labels BOUND scale, P(yes) BOUND scale / 2.  Measured on the MI355X, the largest error / tolerance over each engine's cases is
printed by the tests (DESIGN.md section 3 quotes them)."""
import dataclasses
import os

import numpy as np
import pytest

import _llama_pointwise_ref as P
from conftest import GOLD

pytestmark = pytest.mark.gpu
RK_ERR_INVALID, RK_ERR_STATE, RK_ERR_CAPACITY = -1, -4, -6


def _dims(name):
    from llmrankers import _synth
    return {"llama": _synth.TOY_LLAMA, "llama-vocab260": dataclasses.replace(_synth.TOY_LLAMA, vocab=260), "qwen2": _synth.TOY_QWEN2,
            "qwen3": _synth.TOY_QWEN3, "mistral-w8": dataclasses.replace(_synth.TOY_MISTRAL, sliding_window=8),
            "llama-hd64": _synth.TOY_LLAMA_HD64}[name]


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 4096)
    kw.setdefault("max_seqs", 16)
    return RkLlamaEngine(dims, device=0, **kw).load_state(state.items())


def _cases(vocab):
    """[(ids, n_labels)]: lengths 2 (one prompt token, one label), 17, 129 and 300 (past one 128-key tile, past 256), n_labels 1, 3
    and len - 1; then labels that include the vocabulary's first and last id"""
    from llmrankers import _synth
    out = []
    for L, counts in ((2, (1,)), (17, (1, 3, 16)), (129, (1, 3, 128)), (300, (1, 3, 299))):
        for n in counts:
            out.append(([int(t) for t in _synth.synth_token_batch(1, L, L, vocab, seed=1000 + 7 * L + n)[0]], n))
    edge = [int(t) for t in _synth.synth_token_batch(1, 17, 17, vocab, seed=77)[0]]
    out.append((edge[:-3] + [0, vocab - 1, 0], 3))
    out.append((edge[:-1] + [vocab - 1], 1))
    return out


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module", params=["llama", "llama-vocab260", "qwen2", "qwen3", "mistral-w8", "llama-hd64"])
def world(request):
    """One toy engine with everything the tests of this module read, computed once and never modified: the cases, the reference's
    (score, scale) of each, and the engine's scores of every case alone, of a ragged five, of all cases in one call and of the
    reversed call."""
    from types import SimpleNamespace
    from llmrankers import _synth
    dims = _dims(request.param)
    state = _synth.synth_state_dict(dims, seed=929)
    orc = P.family_oracle(dims, state)
    cases = _cases(dims.vocab)
    ref = [P.loglik(orc, ids, n) for ids, n in cases]
    five = [0, 2, 6, 9, 10]                                         # lengths 2, 17, 129, 300, 17: n_labels 1, 3, 128, 299, 3
    eng = _engine(dims, state)
    seqs, counts = [c[0] for c in cases], [c[1] for c in cases]
    alone = np.concatenate([eng.qlm([s], [n]) for s, n in cases])
    got5 = eng.qlm([seqs[i] for i in five], [counts[i] for i in five])
    batch = eng.qlm(seqs, counts)
    rev = eng.qlm(seqs[::-1], counts[::-1])[::-1]
    w = SimpleNamespace(name=request.param, dims=dims, state=state, orc=orc, cases=cases, ref=ref, eng=eng, five=five, alone=alone, got5=got5,
                        batch=batch, rev=rev)
    yield w
    eng.close()


def test_qlm_against_the_reference(world):
    w = world
    worst = 0.0
    for k, ((ids, n), (want, scale)) in enumerate(zip(w.cases, w.ref)):
        tol = P.qlm_tolerance(n, scale)
        for what, got in (("alone", w.alone[k]), ("all in one call", w.batch[k])):
            err = abs(float(got) - want)
            worst = max(worst, err / tol)
            assert np.isfinite(got) and err < tol, (w.name, what, len(ids), n, float(got), want, err, tol)
    assert w.alone.dtype == np.float32 and w.alone.shape == (len(w.cases),)
    print(f"{w.name}: {len(w.cases)} cases, largest |score - reference| / tolerance = {worst:.3f}")


def test_a_score_does_not_depend_on_what_shares_its_call(world):
    """alone, in the ragged five, in the whole batch, in the reversed batch: the same bits"""
    w = world
    assert (_u32(w.batch) == _u32(w.alone)).all(), (w.name, w.batch, w.alone)
    assert (_u32(w.rev) == _u32(w.alone)).all(), (w.name, w.rev, w.alone)
    assert (_u32(w.got5) == _u32(w.alone[w.five])).all(), (w.name, w.got5, w.alone[w.five])


def test_one_label_equals_the_log_softmax_of_last_logits(world):
    """n_labels = 1 through the new head path (tiled GEMM, log-sum-exp in the epilogue) against the fp64 log-softmax of the old one:
    the full-vocabulary logits of rk_llama_last_logits behind the prompt, fetched 64 vocabulary rows at a time"""
    w = world
    v = w.dims.vocab
    ones = [k for k, (_, n) in enumerate(w.cases) if n == 1]
    assert len(ones) >= 5
    prompts = [w.cases[k][0][:-1] for k in ones]
    z = np.concatenate([w.eng.last_logits(prompts, list(range(v0, min(v0 + 64, v)))) for v0 in range(0, v, 64)], axis=1).astype(np.float64)
    assert z.shape == (len(ones), v)
    worst = 0.0
    for row, k in zip(z, ones):
        lab = w.cases[k][0][-1]
        want = row[lab] - (row.max() + np.log(np.exp(row - row.max()).sum()))
        tol = P.qlm_tolerance(1, w.ref[k][1])
        worst = max(worst, abs(float(w.alone[k]) - want) / tol)
        assert abs(float(w.alone[k]) - want) < tol, (w.name, k, float(w.alone[k]), want, tol)
    print(f"{w.name}: one label, largest |qlm - log_softmax(last_logits)| / tolerance = {worst:.2e}")


def _session_tokens(eng, prompts, poke=None):
    """a session of two slots decoded to its end -> the slots' tokens; poke() runs once after the admit and once after the first run"""
    out = {}
    with eng.session(2, 64, 6, [], 0) as s:
        s.admit(prompts, [0, 1], [6, 3])
        if poke:
            poke()
        first = True
        while s.busy:
            fin, _ = s.run()
            for slot in fin:
                out[slot] = [int(t) for t in s.read(slot)]
            if poke and first:
                poke()
            first = False
    return out


def test_refusals_leave_the_engine_as_it_was():
    from llmrankers import _synth
    from llmrankers._engine import RkEngine, RkError, RkLlamaEngine
    dims = _synth.TOY_LLAMA
    state = _synth.synth_state_dict(dims, seed=929)
    eng = _engine(dims, state, max_tokens=512, max_seqs=4)
    seqs = [[int(t) for t in s] for s in _synth.synth_token_batch(3, 5, 40, dims.vocab, seed=31)]
    ids = list(range(0, 64))
    try:
        g0, l0 = eng.greedy1(seqs).tobytes(), eng.last_logits(seqs, ids).tobytes()      # before the first qlm call

        def untouched(after):
            assert eng.greedy1(seqs).tobytes() == g0 and eng.last_logits(seqs, ids).tobytes() == l0, f"greedy1 / last_logits moved after {after}"

        def refused(code, what, s, n):
            with pytest.raises(RkError) as ei:
                eng.qlm(s, n)
            assert ei.value.code == code, (what, ei.value)
            untouched(what)

        refused(RK_ERR_INVALID, "n_labels 0", seqs, [1, 0, 2])
        refused(RK_ERR_INVALID, "n_labels = len", seqs, [1, len(seqs[1]), 2])
        refused(RK_ERR_INVALID, "a token id outside the vocabulary", [seqs[0][:-1] + [dims.vocab]], [1])
        refused(RK_ERR_CAPACITY, "more sequences than max_seqs", seqs + seqs[:2], [1] * 5)
        refused(RK_ERR_CAPACITY, "more tokens than max_tokens", [[3] * 300, [4] * 300], [1, 1])
        with pytest.raises(ValueError):
            eng.qlm(seqs, [1, 1])
        # an open session: refused, and the session's tokens are those of an undisturbed run
        prompts = [seqs[0], seqs[2]]
        quiet = _session_tokens(eng, prompts)

        def poke():
            with pytest.raises(RkError) as ei:
                eng.qlm(seqs, [1, 1, 1])
            assert ei.value.code == RK_ERR_STATE, ei.value

        assert _session_tokens(eng, prompts, poke) == quiet and sorted(quiet) == [0, 1] and (len(quiet[0]), len(quiet[1])) == (6, 3)
        untouched("a refusal under an open session")
        # a successful call shares the prefill's buffers with them: still the same bytes, and the call itself repeats bit for bit
        a = eng.qlm(seqs, [1, 3, 2])
        untouched("a successful qlm call")
        assert eng.qlm(seqs, [1, 3, 2]).tobytes() == a.tobytes()
    finally:
        eng.close()
    # a T5 engine
    t5 = _synth.TOY_GATED_UNTIED
    t5eng = RkEngine(t5, device=0, max_tokens=256, max_seqs=4, max_dec_len=4).load_state(_synth.synth_state_dict(t5, seed=11).items())
    try:
        with pytest.raises(RkError) as ei:
            RkLlamaEngine.qlm(t5eng, [[5, 6, 7]], [1])
        assert ei.value.code == RK_ERR_STATE, ei.value
    finally:
        t5eng.close()


@pytest.mark.parametrize("key", sorted(P.E2E_SEEDS))
def test_ranker_end_to_end(key):
    """PointwiseLlmRanker on LlamaRuntime: rerank and rerank_many give the reference's ranking (every query's smallest reference gap
    exceeds 4 tolerances: none is left out), scores within the tolerance, counters exact"""
    from transformers import AutoTokenizer
    from llmrankers import _synth
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.pointwise import PointwiseLlmRanker
    from llmrankers.rankers import SearchResult
    toy, tok_name, method = key
    dims = _synth.NAMED_DIMS[toy]
    state = _synth.synth_state_dict(dims, seed=929)
    orc = P.family_oracle(dims, state)
    tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, tok_name))
    queries, passages = P.e2e_inputs(P.E2E_SEEDS[key])
    eng = _engine(dims, state, max_tokens=2048, max_seqs=4)          # four prompts per call: two queries' six passages take two
    try:
        rk = PointwiseLlmRanker.from_runtime(LlamaRuntime.from_engine(eng, dims), tok, method=method, batch_size=2)
        assert rk.decoder_only

        def docs():
            return [SearchResult(docid=f"d{i}", score=0.0, text=t) for i, t in enumerate(passages)]

        items = [(q, docs()) for q in queries]
        many, counters = rk.rerank_many(items)
        worst = 0.0
        for (q, mdocs), mres, cnt in zip(items, many, counters):
            want, tol, lens, dec_len = P.e2e_expected(tok, orc, method, q, passages)
            assert P.min_gap(want) > P.E2E_MIN_GAP * tol, (key, q)
            order = [f"d{i}" for i in sorted(range(len(passages)), key=lambda i: -want[i])]
            ones = docs()
            res = rk.rerank(q, ones)
            one_cnt = (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens)
            assert [d.docid for d in res] == order and [d.docid for d in mres] == order, (key, q)
            assert [d.score for d in ones] == [d.score for d in mdocs]                        # bit for bit, whatever shared the call
            err = float(np.abs(np.asarray([d.score for d in ones]) - want).max())
            worst = max(worst, err / tol)
            assert err < tol, (key, q, err, tol)
            exp_cnt = (2, 2 * max(lens[:2]) + lens[2] + 3 * dec_len, 0)                       # batches of 2 and 1, batch-longest padding
            assert one_cnt == exp_cnt and tuple(cnt) == exp_cnt, (key, q, one_cnt, tuple(cnt), exp_cnt)
        print(f"{key}: largest |score - reference| / tolerance = {worst:.3f}")
    finally:
        eng.close()
