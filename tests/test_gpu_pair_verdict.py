"""pair_verdict_kernel through rk_t5_compare / rk_t5_compare_slot (the tail of a duoT5 compare on the device) on an MI355X:
logits bit for bit rk_t5_score's, the two-way softmax against fp64, the strict verdict, batch independence, the staged form and
the error statuses.

Shapes: d_model 128 (one 512-column pass of the dot product, 48 lanes idle; tied head, so the final norm carries head_scale),
d_model 768 (two passes, the second half filled; tied) and an untied gated model (scale 1, ids inside its small vocabulary).
Pair counts 1, 3 and max_seqs / 2."""
import ctypes as C

import numpy as np
import pytest

from llmrankers import _synth

pytestmark = pytest.mark.gpu

MAX_SEQS = 16
RK_ERR_INVALID, RK_ERR_STATE, RK_ERR_CAPACITY = -1, -4, -6
# fp32 eps is 1.19e-7; P(true) is two expf, one add and one divide on values <= 1: about 4 ulp = 5e-7, doubled
P_TOL = 1e-6

SHAPES = {
    "d128-tied": (_synth.NAMED_DIMS["toy-monot5"], 6136, 1176),
    "d768-tied": (_synth.T5Dims(vocab=6144, d_model=768, n_heads=12, d_kv=64, d_ff=1024, n_enc=2, n_dec=2, gated=False, tied_head=True),
                  6136, 1176),
    "d128-untied": (_synth.NAMED_DIMS["toy-gated-untied"], 41, 42),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_pairs(vocab, n_pairs, seed):
    """n_pairs pairs of token sequences; the two orderings of a pair differ in length in every second pair, and pair 1 (when
    there is one) holds the same sequence twice: the prompt of two documents with identical text."""
    rs = np.random.RandomState(seed)
    seqs = []
    for p in range(n_pairs):
        la = int(rs.randint(5, 70))
        lb = la if p % 2 else int(rs.randint(5, 70))
        a = [int(t) for t in rs.randint(3, vocab, size=la)] + [1]
        b = [int(t) for t in rs.randint(3, vocab, size=lb)] + [1]
        seqs += [a, list(a)] if p == 1 else [a, b]
    return seqs


@pytest.fixture(scope="module", params=list(SHAPES))
def rig(request):
    from llmrankers._engine import RkEngine
    dims, false_id, true_id = SHAPES[request.param]
    state = _synth.synth_state_dict(dims, seed=515, gain=2.0)
    eng = RkEngine(dims, 0, max_tokens=4096, max_seqs=MAX_SEQS, max_dec_len=8).load_state(state.items())
    del state
    # the largest batch once, shared by the tests below: compare and score on the same sequences
    seqs = make_pairs(dims.vocab, MAX_SEQS // 2, seed=7)
    big = eng.compare_pairs(seqs, 0, false_id, true_id)
    score = eng.score(seqs, [0], [false_id, true_id])
    yield eng, dims, false_id, true_id, seqs, big, score
    eng.close()


@pytest.mark.parametrize("n_pairs", [1, 3, MAX_SEQS // 2])
def test_logits_probabilities_and_verdicts(rig, n_pairs):
    eng, dims, false_id, true_id, seqs, big, score = rig
    sub = seqs[:2 * n_pairs]
    assert any(len(sub[2 * p]) != len(sub[2 * p + 1]) for p in range(n_pairs))
    logits, p_true, wins = eng.compare_pairs(sub, 0, false_id, true_id)
    assert logits.shape == (2 * n_pairs, 2) and p_true.shape == (2 * n_pairs,) and wins.shape == (n_pairs,) and wins.dtype == bool
    ref = eng.score(sub, [0], [false_id, true_id])
    assert np.array_equal(bits(logits), bits(ref)), "logits differ from rk_t5_score's"
    lg = logits.astype(np.float64)
    m = lg.max(axis=1)
    want = np.exp(lg[:, 1] - m) / (np.exp(lg[:, 0] - m) + np.exp(lg[:, 1] - m))
    err = float(np.abs(p_true.astype(np.float64) - want).max())
    print(f"n_pairs={n_pairs} d={dims.d_model}: max |P(true) - fp64 softmax| = {err:.3g}, logits span {lg.min():.3f}..{lg.max():.3f}")
    assert err <= P_TOL
    assert np.array_equal(wins, p_true[0::2] > p_true[1::2])
    # a pair's seven floats alone and inside the largest batch
    assert np.array_equal(bits(logits), bits(big[0][:2 * n_pairs])) and np.array_equal(bits(p_true), bits(big[1][:2 * n_pairs]))
    assert np.array_equal(wins, big[2][:n_pairs])


def test_largest_batch_matches_score_and_is_not_degenerate(rig):
    eng, dims, false_id, true_id, seqs, big, score = rig
    assert np.array_equal(bits(big[0]), bits(score))
    assert len(np.unique(bits(big[0]))) > MAX_SEQS, "logits are (nearly) all equal: the test would show nothing"
    assert np.all(np.isfinite(big[1])) and np.all((big[1] > 0) & (big[1] < 1))


def test_identical_documents_tie_and_lose(rig):
    """pair 1 holds the same prompt twice: bitwise-equal probabilities, and the strict rule gives verdict 0"""
    eng, dims, false_id, true_id, seqs, big, score = rig
    assert seqs[2] == seqs[3]
    assert bits(big[1][2]) == bits(big[1][3]) and np.array_equal(bits(big[0][2]), bits(big[0][3]))
    assert not big[2][1]
    alone = eng.compare_pairs(seqs[2:4], 0, false_id, true_id)
    assert not alone[2][0] and np.array_equal(bits(alone[1]), bits(big[1][2:4]))


def test_a_later_pair_alone_equals_its_place_in_the_batch(rig):
    eng, dims, false_id, true_id, seqs, big, score = rig
    for p in (4, MAX_SEQS // 2 - 1):
        lg, pt, w = eng.compare_pairs(seqs[2 * p:2 * p + 2], 0, false_id, true_id)
        assert np.array_equal(bits(lg), bits(big[0][2 * p:2 * p + 2])) and np.array_equal(bits(pt), bits(big[1][2 * p:2 * p + 2]))
        assert w[0] == big[2][p]


def test_staged_form_agrees_with_the_blocking_form(rig):
    eng, dims, false_id, true_id, seqs, big, score = rig
    for slot, n_pairs in ((0, MAX_SEQS // 2), (1, 3)):
        eng.stage(seqs[:2 * n_pairs], slot=slot)
        eng.compare_staged(0, false_id, true_id, slot=slot)
        lg, pt, w = eng.read_scores(slot)
        assert np.array_equal(bits(lg), bits(big[0][:2 * n_pairs])) and np.array_equal(bits(pt), bits(big[1][:2 * n_pairs]))
        assert np.array_equal(w, big[2][:n_pairs])
    # the raw buffer: 7 floats per pair, verdicts as 1.0f / 0.0f, and not one float more
    eng.stage(seqs[:6], slot=0)
    eng.compare_staged(0, false_id, true_id, slot=0)
    raw = np.empty(22, np.float32)
    fp = C.POINTER(C.c_float)
    assert eng.lib.rk_t5_read_scores_slot(eng.h, 0, raw.ctypes.data_as(fp), 22) == RK_ERR_INVALID
    assert eng.lib.rk_t5_read_scores_slot(eng.h, 0, raw.ctypes.data_as(fp), 21) == 0
    assert np.array_equal(bits(raw[:12]), bits(big[0][:6]).reshape(-1)) and np.array_equal(bits(raw[12:18]), bits(big[1][:6]))
    assert [float(x) for x in raw[18:21]] == [1.0 if v else 0.0 for v in big[2][:3]]
    # both slots in flight at once
    eng.stage(seqs[:8], slot=0)
    eng.stage(seqs[8:], slot=1)
    eng.compare_staged(0, false_id, true_id, slot=0)
    eng.compare_staged(0, false_id, true_id, slot=1)
    second, first = eng.read_scores(1), eng.read_scores(0)
    assert np.array_equal(bits(first[1]), bits(big[1][:8])) and np.array_equal(bits(second[1]), bits(big[1][8:]))
    assert np.array_equal(first[2], big[2][:4]) and np.array_equal(second[2], big[2][4:])


def test_error_statuses_launch_nothing(rig):
    from llmrankers._engine import RkError, pack_ragged
    eng, dims, false_id, true_id, seqs, big, score = rig
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def still_answers():
        lg, pt, w = eng.compare_pairs(seqs[:6], 0, false_id, true_id)
        assert np.array_equal(bits(lg), bits(big[0][:6])) and np.array_equal(bits(pt), bits(big[1][:6])) and np.array_equal(w, big[2][:3])

    def code(fn, *args):
        with pytest.raises(RkError) as exc:
            fn(*args)
        return exc.value.code

    # ids outside the vocabulary, equal ids
    assert code(eng.compare_pairs, seqs[:4], 0, dims.vocab, true_id) == RK_ERR_INVALID
    assert code(eng.compare_pairs, seqs[:4], 0, false_id, -1) == RK_ERR_INVALID
    assert code(eng.compare_pairs, seqs[:4], dims.vocab, false_id, true_id) == RK_ERR_INVALID
    assert code(eng.compare_pairs, seqs[:4], 0, true_id, true_id) == RK_ERR_INVALID
    still_answers()
    # n_pairs <= 0 (the binding never sends it: the C entry point itself)
    tok, off = pack_ragged(seqs[:2])
    lg, pt, w = np.zeros(4, np.float32), np.zeros(2, np.float32), np.zeros(1, np.int32)
    for n in (0, -3):
        assert eng.lib.rk_t5_compare(eng.h, tok.ctypes.data_as(ip), off.ctypes.data_as(ip), n, 0, false_id, true_id,
                                     lg.ctypes.data_as(fp), pt.ctypes.data_as(fp), w.ctypes.data_as(ip)) == RK_ERR_INVALID
    # capacity, as rk_t5_score: too many sequences, too many tokens
    assert code(eng.compare_pairs, seqs + seqs[:2], 0, false_id, true_id) == RK_ERR_CAPACITY
    assert code(eng.compare_pairs, [[5] * 2100 + [1], [5] * 2100 + [1]], 0, false_id, true_id) == RK_ERR_CAPACITY
    still_answers()
    # the staged form: an odd batch; no staged batch (the stage before it failed)
    eng.stage(seqs[:3], slot=1)
    assert code(eng.compare_staged, 0, false_id, true_id, 1) == RK_ERR_INVALID
    assert code(eng.stage, seqs + seqs[:2], 1) == RK_ERR_CAPACITY
    assert code(eng.compare_staged, 0, false_id, true_id, 1) == RK_ERR_STATE
    assert eng.lib.rk_t5_compare_slot(eng.h, 7, 0, false_id, true_id) == RK_ERR_INVALID
    still_answers()
    assert np.array_equal(bits(eng.score(seqs, [0], [false_id, true_id])), bits(score))       # and rk_t5_score is what it was


def test_llama_engine_is_refused():
    from llmrankers._engine import RkError, RkLlamaEngine
    dims = _synth.NAMED_DIMS["toy-llama"]
    eng = RkLlamaEngine(dims, device=0, max_tokens=1024, max_seqs=4).load_state(_synth.synth_state_dict(dims, seed=3).items())
    try:
        with pytest.raises(RkError) as exc:
            eng.compare_pairs([[5, 6, 1], [7, 8, 1]], 0, 41, 42)
        assert exc.value.code == RK_ERR_STATE
        assert eng.lib.rk_t5_compare_slot(eng.h, 0, 0, 41, 42) == RK_ERR_STATE
        assert list(eng.greedy1([[5, 6, 7, 8]])) == list(eng.greedy1([[5, 6, 7, 8]]))       # the engine still answers
    finally:
        eng.close()
