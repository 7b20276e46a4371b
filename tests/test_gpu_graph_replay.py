"""Decoder chains replayed as HIP graphs (csrc/rk_engine.hip: run_graphed) against the same chains launched eagerly.

A replay carries the launch arguments of the call it was captured from: it is right only while the graph's key holds every value
those arguments depend on and everything else a chain reads lives in device memory.  Every test here primes a key on a default
engine G (three calls: eager, captured, replayed), then replays it on a TWIN - a call with the same key that differs in what the
key leaves out (every length but the longest, the token count, which row is the longest, the prefix / output / candidate / eos /
pad ids, the prompt lengths of a Llama step, a new session of the same sizes) - and then on the first call again.  The reference is
always E, an engine created with dec_graph = 0 (its kernels are held to fp64 and to the oracles elsewhere in the suite); every
comparison is bit for bit, on the call's results and on the decoder's hidden rows read back after it.  rk_debug_graph_stats is
asserted around every step: what was expected to replay did replay and did nothing else, no key ever failed to capture, and the
table gained a key exactly where the test says so.  The last tests are the options epoch and the bound of the table.

Engines are never flipped between graphs and eager launches: set_option starts a new epoch."""
import os
import re

import numpy as np
import pytest

from _graph_util import (DEC17_A, DEC17_B, LEN_A, LEN_B, LEN_C, LEN_LA, LEN_LB, LEN_MA, LEN_MB, LLAMA_CKPTS, _compare, _delta, _differ, _eager,
                         _generate, _greedy, _llama_generate, _llama_pair, _prime, _report, _same, _score, _score_slot1,
                         _session_script, _step, _tokens, _unused_id, llama_checkpoint, t5_checkpoint, t5_engine)
from conftest import REPO

pytestmark = pytest.mark.gpu

def _prime_then_twins(G, E, calls, keys=1, what=""):
    """calls: name -> call(engine) -> outputs; the first is A, the others its twins.  A, A, A (the third is a replay), every twin, A
    again: each replays and does nothing else.  Every twin must differ from A on E (else the inputs prove nothing)."""
    names = list(calls)
    ref = {n: _eager(E, calls[n]) for n in names}
    a = names[0]
    for n in names[1:]:
        assert _differ(ref[n][0], ref[a][0]), f"{what}: twin {n} gives A's result on the eager engine: the inputs need changing"
    _prime(G, calls[a], ref[a][0], ref[a][1], keys, f"{what} {a}")
    for n in names[1:] + [a]:
        _step(G, calls[n], ref[n][0], f"{what} {n} (a replay of {a}'s graph)", replays=ref[n][1])
    return ref


# ---------------------------------------------------------------- engines ----------------------------------------------------------

@pytest.fixture(scope="module")
def t5(ckpt_dirs):
    """(dims, G, E): the default engine and one created for dec_graph = 0, on the committed gated / untied toy checkpoint"""
    dims, state = t5_checkpoint(ckpt_dirs)
    G, E = t5_engine(dims, state), t5_engine(dims, state, graphs=False)
    yield dims, G, E
    for e in (G, E):
        e.close()


@pytest.fixture(scope="module", params=LLAMA_CKPTS)
def llama(request, ckpt_dirs, tmp_path_factory):
    """(dims, G, E) on the committed toy Llama (128-wide heads) and toy Qwen2 (64-wide heads, q / k / v biases) checkpoints"""
    dims, state = llama_checkpoint(request.param, ckpt_dirs, tmp_path_factory.mktemp("graph_replay"))
    G, E = _llama_pair(dims, state)
    yield dims, G, E
    for e in (G, E):
        e.close()


# ---------------------------------------------------------------- T5 calls ---------------------------------------------------------

@pytest.mark.parametrize("dec_len", [1, 2])
def test_score_query_side_replays_on_other_lengths_and_ids(t5, dec_len):
    """GK_T5_SCORE over the raw encoder states: the key holds the chunk count.  Replayed with the host's T, longest row or shortest
    sequence of the capture in a launch argument (a grid, a row count, an offset), B and C lose rows or read A's; with a prefix or
    output id in an argument instead of the slot's index buffers, B's scores are A's columns.  Slot 1 holds its own buffers: its
    first launch of the same shape is a NEW key, and its graph replays on B like slot 0's."""
    dims, G, E = t5
    since = G.graph_stats()
    v = dims.vocab
    pre = {1: ([0], [5], [0]), 2: ([0, 7], [4, 11], [0, 19])}[dec_len]
    ids = ([21, 22, 23], [30, 31, 32], [23, 40, 21])
    calls = {n: _score(_tokens(lens, v, 100 + i), pre[i], ids[i]) for i, (n, lens) in enumerate((("A", LEN_A), ("B", LEN_B), ("C", LEN_C)))}
    ref = _prime_then_twins(G, E, calls, what=f"score dec_len {dec_len}")
    slot1 = {n: _score_slot1(_tokens(lens, v, 100 + i), pre[i], ids[i]) for i, (n, lens) in enumerate((("A", LEN_A), ("B", LEN_B), ("C", LEN_C)))}
    want = {n: (ref[n][0][0],) for n in slot1}                          # E's blocking scores: a slot changes nothing in the bits
    _step(G, slot1["A"], want["A"], "slot 1: the slot is part of the key", eager=1, n_keys=1)
    _step(G, slot1["A"], want["A"], "slot 1 captured", captures=1, n_ready=1)
    for n in ("A", "B", "C", "A"):
        _step(G, slot1[n], want[n], f"slot 1 {n} replayed", replays=1)
    _step(G, calls["B"], ref["B"][0], "slot 0 again, behind slot 1's launches", replays=1)
    _report(G, since, f"GK_T5_SCORE query side, dec_len {dec_len}, slots 0 and 1")


@pytest.mark.parametrize("lens_a,lens_b", [(LEN_MA, LEN_MB), (LEN_LA, LEN_LB)], ids=["longest128", "rows_above_192_keys"])
def test_score_materialised_kv_replays_on_other_lengths(t5, lens_a, lens_b):
    """GK_T5_SCORE at 17 decoder positions: cross-attention over the materialised K / V, the key holds the longest sequence itself
    (the staged kernels' LDS and grid follow from it).  The twin keeps the longest and changes its row, T and every other length; in
    the second pair the rows above 192 keys - the staged kernel's, the others are the matrix-core kernel's - sit elsewhere: a
    replay that carried the capture's choice per ROW instead of per key count would give B's rows 0 and 2 to the wrong kernel."""
    dims, G, E = t5
    since = G.graph_stats()
    assert max(lens_a) == max(lens_b) and sorted(lens_a) != sorted(lens_b)
    calls = {"A": _score(_tokens(lens_a, dims.vocab, 200), DEC17_A, [21, 22, 23, 24]),
             "B": _score(_tokens(lens_b, dims.vocab, 201), DEC17_B, [33, 22, 50, 24])}
    ref = _prime_then_twins(G, E, calls, what=f"score dec_len 17, longest {max(lens_a)}")
    # another longest sequence in the same chunk count: with materialised K / V a NEW key (the staged kernels' LDS follows from it)
    lens_d = tuple(min(n, max(lens_b) - 7) for n in lens_b)
    assert (max(lens_d) + 63) // 64 == (max(lens_b) + 63) // 64
    other = _score(_tokens(lens_d, dims.vocab, 202), DEC17_B, [33, 22, 50, 24])
    want, _ = _eager(E, other)
    _step(G, other, want, "another longest sequence: a first sighting", eager=1, n_keys=1)
    _step(G, calls["B"], ref["B"][0], "B again", replays=1)
    _report(G, since, f"GK_T5_SCORE materialised K / V, longest {max(lens_a)}")


def test_compare_replays_on_other_pairs_and_new_ids_are_a_new_key(t5):
    """GK_T5_COMPARE: pair_verdict_kernel takes false_id / true_id as launch arguments, so they are part of the key - a call with
    other ids must NOT replay (it would return the first ids' logits); other lengths and another start id must."""
    dims, G, E = t5
    since = G.graph_stats()
    v = dims.vocab
    a, b = _tokens(LEN_A + (77,), v, 300), _tokens(LEN_B + (40,), v, 301)
    calls = {"A": _compare(a, 0, 40, 41), "B": _compare(b, 6, 40, 41)}
    ref = _prime_then_twins(G, E, calls, what="compare")
    other = _compare(b, 6, 41, 52)
    want, n = _eager(E, other)
    assert n == 1 and _differ(want, ref["B"][0]), "other (false_id, true_id) give the same logits on the eager engine: the inputs need changing"
    _step(G, other, want, "compare with other ids: a first sighting", eager=1, n_keys=1)
    _step(G, calls["B"], ref["B"][0], "compare B, the first ids again", replays=1)
    _report(G, since, "GK_T5_COMPARE")


def test_greedy_steps_replay_on_other_lengths_and_prefix(t5):
    """GK_T5_GREEDY_STEP: rk_t5_greedy with max_new 3 recomputes the prefix every step, one key per step (1, 2, 3 positions).  The
    twin has other lengths in the same chunk count and another prefix id; its rows are written by the host between the steps, so
    a replay that kept the capture's ids would repeat A's tokens."""
    dims, G, E = t5
    since = G.graph_stats()
    v = dims.vocab
    a, b = _tokens(LEN_A, v, 400), _tokens(LEN_B, v, 401)
    free = [E.greedy(s, p, 3, eos_id=v - 1)[0] for s, p in ((a, [0]), (b, [9]))]
    eos = _unused_id(free, v)                                          # no row finishes: all three steps run, on both engines
    calls = {"A": _greedy(a, [0], 3, eos, 0, 3), "B": _greedy(b, [9], 3, eos, 5, 3)}
    ref = _prime_then_twins(G, E, calls, keys=3, what="greedy")
    assert ref["A"][1] == 3 and ref["B"][1] == 3 and int(ref["A"][0][1]) == 3
    _report(G, since, "GK_T5_GREEDY_STEP")


def test_greedy2_replays_on_other_candidates_and_falls_back(t5):
    """GK_T5_GREEDY2: the speculative pass (prefix rows + one row per candidate, the tree form).  The candidate ids are decoder
    input ids in the slot's index buffer: a twin with other candidates of the same count, another prefix and other lengths replays
    A's graph.  A first token outside the candidates takes one ordinary greedy step behind the replayed pass: that step is a key
    of its own (first sighting, then captured, then both chains replay)."""
    dims, G, E = t5
    since = G.graph_stats()
    v = dims.vocab
    a, b = _tokens(LEN_A[:4], v, 500), _tokens(LEN_C[:4], v, 501)    # four sequences: the fallback step's key is not rk_t5_greedy's above
    pa, pb, n_cand = [0, 9], [0, 31], 5
    eos = _unused_id([E.greedy(s, p, 2, eos_id=v - 1)[0] for s, p in ((a, pa), (b, pb))], v)
    first = [E.greedy(s, p, 2, eos_id=eos)[0] for s, p in ((a, pa), (b, pb))]   # the plain loop's tokens, no row finished
    assert all((f != eos).all() for f in first)

    def cands(toks, hit):
        t1 = sorted(set(int(t) for t in toks[:, 0]))
        spare = [i for i in range(60, 60 + 2 * n_cand + len(t1)) if i not in t1 and i != eos]
        return (t1 + spare)[:n_cand] if hit else spare[:n_cand]

    rows = len(pa) + n_cand
    calls = {"A": _greedy(a, pa, 2, eos, 0, rows, cands(first[0], True)), "B": _greedy(b, pb, 2, eos, 0, rows, cands(first[1], True))}
    ref = _prime_then_twins(G, E, calls, what="greedy2")
    for n, f in (("A", first[0]), ("B", first[1])):                    # (and the speculative pass gives the plain loop's tokens)
        np.testing.assert_array_equal(ref[n][0][0], f)
    miss = _greedy(b, pb, 2, eos, 0, rows, cands(first[1], False))
    want, n = _eager(E, miss)
    assert n == 2, "the first tokens are among the candidates: the fallback step did not run, the inputs need changing"
    np.testing.assert_array_equal(want[0], first[1])
    _step(G, miss, want, "greedy2 miss: replayed pass + the fallback step's first sighting", replays=1, eager=1, n_keys=1)
    _step(G, miss, want, "greedy2 miss: fallback step captured", replays=1, captures=1, n_ready=1)
    _step(G, miss, want, "greedy2 miss: both chains replayed", replays=2)
    _step(G, calls["A"], ref["A"][0], "greedy2 A again", replays=1)
    _report(G, since, "GK_T5_GREEDY2 (and its fallback step)")


@pytest.mark.parametrize("dec_len", [1, 3])
def test_generate_step_replays_within_and_across_calls(t5, dec_len):
    """GK_T5_GENERATE_STEP: one graph per (n_seq, chunks, dec_len, max_new), replayed inside a call from its third step on;
    position, finished rows, next ids, eos and pad live in the call's int block on the device.  The twin has other lengths and
    prefix ids, an eos id that one of its rows emits at column 1 (the row finishes early and pads) and another pad id: an eos, pad
    or prefix id carried as a launch argument would leave the row running, pad with A's id or feed A's prefix."""
    dims, G, E = t5
    since = G.graph_stats()
    v = dims.vocab
    a, b = _tokens(LEN_A, v, 600 + dec_len), _tokens(LEN_B, v, 610 + dec_len)
    pa, pb = ([0], [8]) if dec_len == 1 else ([0, 7, 12], [3, 30, 4])
    free = [E.generate(s, p, 6, eos_id=v - 1)[0] for s, p in ((a, pa), (b, pb))]
    eos_a = _unused_id(free, v)
    eos_b = int(free[1][0, 1])                                          # what E emitted for B's row 0 at column 1
    calls = {"A": _generate(a, pa, 6, eos_a, 0), "B": _generate(b, pb, 6, eos_b, 3)}
    ref = _prime_then_twins(G, E, calls, what=f"generate dec_len {dec_len}")
    ta, tb = ref["A"][0][0], ref["B"][0][0]
    assert int(ref["A"][0][1]) == 6 and ref["A"][1] >= dec_len - 1 + 6
    k = int(np.argmax(tb[0] == eos_b))
    assert tb[0, k] == eos_b and k <= 1 and (tb[0, k + 1:] == 3).all(), "B's row 0 does not finish early and pad: the inputs need changing"
    assert (ta != eos_a).all()
    _report(G, since, f"GK_T5_GENERATE_STEP dec_len {dec_len}")


# ---------------------------------------------------------------- Llama calls ------------------------------------------------------

def test_llama_step_replays_on_other_prompt_lengths_eos_and_pad(llama):
    """GK_LLAMA_STEP: the key holds (n_seq, P = longest prompt + max_new).  The twin keeps the longest prompt (in another row) and
    changes the other lengths (one prompt of a single token), has two eos ids where A has none, another pad id and a max_total
    that cuts its longest row short: lengths, positions, eos, pad and max_total live in the call's int block, and a replay that
    carried one of them as a launch argument would write B's keys at A's positions or never finish B's rows."""
    dims, G, E = llama
    since = G.graph_stats()
    v = dims.vocab
    a, b = _tokens((40, 23, 9), v, 700), _tokens((1, 40, 17), v, 701)
    free = E.generate(b, 6, [], 0)[0]
    eos_b = [int(free[0, 2]), _unused_id([free], v)]                    # what row 0 emits at column 2, and an id nothing emits
    assert eos_b[0] not in free[1, :3], f"the eos id would end the longest row before max_total does ({free.tolist()}): the inputs need changing"
    calls = {"A": _llama_generate(a, 6, [], 0), "B": _llama_generate(b, 6, eos_b, 5, max_total=43)}
    ref = _prime_then_twins(G, E, calls, what="llama generate")
    ta, tb = ref["A"][0][0], ref["B"][0][0]
    assert int(ref["A"][0][1]) == 6 and ref["A"][1] == 5               # column 0 is the prefill's: five steps
    np.testing.assert_array_equal(tb[1], list(free[1, :3]) + [5, 5, 5], err_msg="max_total 43 cuts the 40-token prompt after three tokens")
    k = int(np.argmax(tb[0] == eos_b[0]))                               # row 0 ends at the eos id, then pads
    assert k <= 2 and (tb[0, :k + 1] == free[0, :k + 1]).all() and (tb[0, k + 1:] == 5).all(), (tb[0], free[0])
    _report(G, since, f"GK_LLAMA_STEP head_dim {dims.head_dim}")


def test_llama_session_step_replays_in_a_second_session(llama):
    """GK_LLAMA_SESSION_STEP: the key holds (n_slots, max_len, cap).  A second session of the same sizes - other prompts, eos and pad
    ids - replays the first session's graph from its FIRST step: eos, pad, every slot's length, column and position live in the
    session's int block.  A generate between the two (buffers sized beforehand, so none moves) leaves both keys as they were."""
    dims, G, E = llama
    since = G.graph_stats()
    v = dims.vocab
    p1, p2 = _tokens((30, 12, 5), v, 800), _tokens((7, 41, 1), v, 801)
    gen = _llama_generate(_tokens((20, 33), v, 802), 5, [], 0)
    eos2 = int(E.generate([p2[1]], 3, [], 0)[0][0, 1])                 # ends the second session's slot 2 a column early (or at its admit)
    assert eos2 not in E.generate([p2[0]], 8, [], 0)[0], "slot 0 must outlast the late admit: the inputs need changing"
    s1, s2 = _session_script(p1, [], 0), _session_script(p2, [eos2], 7)
    want1, n1 = _eager(E, s1)
    want_gen, n_gen = _eager(E, gen)
    want2, n2 = _eager(E, s2)
    assert len(want1) != len(want2) or _differ(want1, want2), "the two sessions give the same log on the eager engine: the inputs need changing"
    # size the cache, the partials and the int block for both callers first: a buffer that grows later would (rightly) change the keys
    G.generate(_tokens((20, 33), v, 802), 5, [], 0)
    G.session(3, 96, 8, [], 0).close()
    before = G.graph_stats()
    _same(s1(G), want1, "session 1")
    d = _delta(G, before)
    assert d == dict(n_keys=1, n_ready=1, eager=1, captures=1, replays=n1 - 2, failed=0, evictions=0), d
    _prime(G, gen, want_gen, n_gen, 1, "generate between the sessions")
    _step(G, s2, want2, "session 2: a replay from its first step", replays=n2)
    _step(G, gen, want_gen, "generate behind the second session", replays=n_gen)
    _step(G, s1, want1, "the first session's script again", replays=n1)
    _report(G, since, f"GK_LLAMA_SESSION_STEP head_dim {dims.head_dim} (with the generate calls between the sessions)")


# ---------------------------------------------------------------- eager paths, options epoch, the bound ----------------------------

def test_documented_eager_paths(t5):
    """qlm and qlm_many launch outside run_graphed: no key, no counter moves.  With profiling on a replayable key runs eagerly (the
    per-kernel events), with the same bits, and replays again once profiling is off."""
    dims, G, E = t5
    since = G.graph_stats()
    v = dims.vocab
    seqs = _tokens(LEN_A, v, 900)
    labels = [11, 12, 13, 14, 1]
    many = [[11, 12, 1], [13, 1], [14, 15, 16, 17, 1], [18, 1], [19, 20, 1]]
    for what, call in (("qlm", lambda e: (e.qlm(seqs, labels),)), ("qlm_many", lambda e: (e.qlm_many(seqs, many),))):
        want, n = _eager(E, call)
        assert n == 0
        for i in range(3):
            _step(G, call, want, f"{what} call {i}")
    call = _score(seqs, [0], [21, 22, 23, 24, 25, 26])
    want, _ = _eager(E, call)
    _prime(G, call, want, 1, 1, "score")
    G.profile(True)
    try:
        _step(G, call, want, "profiling on: eager", eager=1)
        _step(G, call, want, "profiling on: eager again", eager=1)
    finally:
        G.profile(False)
    _step(G, call, want, "profiling off: the graph again", replays=1)
    _report(G, since, "qlm, qlm_many, profiling")


@pytest.mark.parametrize("option,prefix", [("dec_gemv", [0, 7]), ("dec_cross_mfma", DEC17_A)], ids=["dec_gemv", "dec_cross_mfma"])
def test_options_epoch_keeps_old_graphs_from_replaying(t5, option, prefix):
    """Two sequences: at two positions four decoder rows, the few-row GEMV family (dec_gemv); at 17 positions the matrix-core
    cross-attention over the materialised K / V (dec_cross_mfma).  A graph captured under the option's default holds that family's
    kernels; after set_option the same call must be a first sighting under the new epoch and give the OTHER family's bits."""
    dims, G, E = t5
    since = G.graph_stats()
    seqs = _tokens((90, 120), dims.vocab, 1000)
    call = _score(seqs, prefix, [21, 22])
    try:
        on, _ = _eager(E, call)
        E.set_option(option, 0)
        off, _ = _eager(E, call)
        assert _differ(on, off), f"{option} 1 and 0 give the same bits on the eager engine: the inputs need changing"
        _prime(G, call, on, 1, 1, f"{option} = 1")
        G.set_option(option, 0)
        _step(G, call, off, f"{option} = 0: a first sighting under the new epoch", eager=1, n_keys=1)
        _step(G, call, off, f"{option} = 0: captured", captures=1, n_ready=1)
        _step(G, call, off, f"{option} = 0: replayed", replays=1)
    finally:
        G.set_option(option, 1)
        E.set_option(option, 1)
    _step(G, call, on, f"{option} = 1 again: a third epoch", eager=1, n_keys=1)
    assert _eager(E, call)[0][0].tobytes() == on[0].tobytes()
    _report(G, since, f"options epoch, {option}")


def test_graph_table_is_bounded_and_evicted_keys_come_back(t5):
    """The table holds at most RK_GRAPH_CACHE_KEYS keys.  K0 is primed, then enough other keys are sighted once each (cheap eager
    calls: n_out 1 .. 64 x n_seq 1 .. 5 at one position) to pass the bound, and one more key is sighted twice (a capture).  By then
    an eviction has happened and the table is under the bound again - at EVERY return, in fact; K0 still gives E's bits throughout,
    is captured again on its second sighting after the eviction, replays from then on, and the next capture of another key does
    not evict it again.  Blocking calls only: nothing is in flight at an eviction."""
    dims, G, E = t5
    since = G.graph_stats()
    v = dims.vocab
    bound = G.graph_stats()["max_keys"]
    with open(os.path.join(REPO, "include", "rk_engine.h")) as f:
        stated = re.search(r"#define\s+RK_GRAPH_CACHE_KEYS\s+(\d+)", f.read())
    assert stated and int(stated.group(1)) == bound and bound >= 8
    k0 = _score(_tokens(LEN_A, v, 1100), [0], [21, 22, 23, 24, 25, 26, 27])
    want, _ = _eager(E, k0)
    _prime(G, k0, want, 1, 1, "K0")
    short = _tokens((9, 17, 5, 33, 12), v, 1101)                        # one chunk: none of these is a key of another test
    others = [(n_seq, n_out) for n_out in range(1, 65) for n_seq in range(1, 6)]
    start = G.graph_stats()
    need = bound - start["n_keys"] + 1                                  # new keys that take the table past the bound
    assert need <= len(others) - 2
    sighted = 0
    for n_seq, n_out in others[:need]:
        G.score(short[:n_seq], [0], list(range(40, 40 + n_out)))
        sighted += 1
        now = G.graph_stats()
        assert now["n_keys"] <= bound, f"{now['n_keys']} keys after {sighted} new ones: the table passed its bound of {bound}"
        if sighted == need - 1:                                         # the table is full and nothing was evicted yet
            assert now["n_keys"] == bound and now["evictions"] == start["evictions"]
            _step(G, k0, want, "K0 in a full table", replays=1)
    k1 = _score(short[:others[need][0]], [0], list(range(40, 40 + others[need][1])))
    want1, _ = _eager(E, k1)
    _same(k1(G), want1, "K1 first sighting")
    _same(k1(G), want1, "K1 captured")
    now = G.graph_stats()
    assert now["evictions"] > start["evictions"] and now["n_keys"] <= bound and now["failed"] == 0, now
    assert now["n_keys"] < start["n_keys"] + need, "the eviction erased nothing"
    assert now["eager"] - start["eager"] == need + 1 and now["captures"] - start["captures"] == 1, now
    _step(G, k0, want, "K0 after the eviction: a first sighting", eager=1, n_keys=1)
    _step(G, k0, want, "K0 captured again", captures=1, n_ready=1)
    _step(G, k0, want, "K0 replayed", replays=1)
    k2 = _score(short[:others[need + 1][0]], [0], list(range(40, 40 + others[need + 1][1])))
    want2, _ = _eager(E, k2)
    _step(G, k2, want2, "K2 first sighting", eager=1, n_keys=1)
    _step(G, k2, want2, "K2 captured: the table is under its bound, nothing is evicted", captures=1, n_ready=1)
    _step(G, k0, want, "K0 behind another key's capture: still its graph", replays=1)
    _step(G, k1, want1, "K1 too", replays=1)
    _report(G, since, f"eviction at a bound of {bound} keys")
