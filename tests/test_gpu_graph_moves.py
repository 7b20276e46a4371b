"""Cached decoder graphs across buffer moves, and evictions / moves / option changes with launches in flight.

A replayed graph carries raw device addresses.  Some belong to buffers that are freed and reallocated when a call needs more of
them (csrc/rk_engine.hip: Grown<T>::reserve): the arg-max pair, rk_t5_generate's K / V cache, the Llama family's K / V cache,
attention partials and int block.  What keeps a graph from replaying onto freed memory is a move counter in its key (amax_gen,
kv_gen, lkv_gen); what keeps a move or an eviction from freeing memory under the OTHER slot's queued decoder is the drain in front
of it.  test_gpu_graph_replay.py sizes every buffer before it captures; here the buffers move AFTER a capture.

Every move case: prime call A on a fresh default engine G (eager, captured, replayed); call B moves a NAMED buffer - rk_debug_buffers
says which buffers were reallocated, which were not, and which counter stepped by how much; then A must be a first sighting, a
capture and a replay again, with the reference's bits each time.  The reference is E (dec_graph = 0, held to fp64 and the oracles
elsewhere), bit for bit on the call's results and the rows rk_debug_read gives; A and B must differ on E; B is held to E too.
rk_debug_graph_stats is asserted around every step (failed == 0 throughout), and gen_buf - which no counter guards - must stay
where its first allocation put it over every call of this file."""
import numpy as np
import pytest

from _graph_util import (COUNTERS, LEN_A, LEN_B, LLAMA_CKPTS, _differ, _eager, _generate, _greedy, _llama_generate, _prime, _report, _same,
                         _score, _session_script, _step, _tokens, _unused_id, llama_checkpoint, llama_engine, t5_checkpoint, t5_engine)

pytestmark = pytest.mark.gpu

GENS = ("amax_gen", "kv_gen", "lkv_gen")
AMAX = ("amax_val", "amax_idx")
DEC17 = [0] + [5 + 3 * i for i in range(16)]
LONG5, LONG5B = (120, 97, 118, 64, 109), (101, 120, 66, 119, 93)      # two chunks, a long decoder chain at 17 positions


# ---------------------------------------------------------------- bookkeeping ------------------------------------------------------

def _names():
    from llmrankers._engine import BUFFER_NAMES
    return BUFFER_NAMES


def _moved(G, before, names, what, **gens):
    """exactly `names` were reallocated since `before` (= G.buffers()) and the counters stepped by exactly `gens`.  A buffer was
    reallocated if its address OR its capacity changed: reserve only ever replaces a buffer by a larger one, and the allocator may
    hand the old address out again."""
    now = G.buffers()
    moved = {n for n in _names() if now[n] != before[n]}
    print(f"[buffers] {what}: " + (", ".join(f"{n} {before[n]['cap']} -> {now[n]['cap']}" + ("" if now[n]["addr"] != before[n]["addr"] else " (same address)")
                                             for n in _names() if n in moved) or "nothing moved")
          + "; " + ", ".join(f"{k} +{now[k] - before[k]}" for k in GENS))
    assert moved == set(names), f"{what}: {sorted(moved)} were reallocated, expected {sorted(names)}"
    for n in names:
        assert now[n]["cap"] > before[n]["cap"] and now[n]["addr"] != 0, (what, n, before[n], now[n])
    exp = dict.fromkeys(GENS, 0)
    exp.update(gens)
    assert {k: now[k] - before[k] for k in GENS} == exp, f"{what}: the counters stepped by { {k: now[k] - before[k] for k in GENS} }, expected {exp}"
    return now


def _gen_buf_stays(G, fn, what):
    """gen_buf has no counter: its size is a function of max_dec_len and max_seqs alone, so once allocated it never moves"""
    before = G.buffers()["gen_buf"]
    out = fn()
    if before["addr"]:
        assert G.buffers()["gen_buf"] == before, f"{what}: gen_buf was reallocated ({before} -> {G.buffers()['gen_buf']}): GK_T5_GENERATE_STEP needs a counter for it"
    return out


def _mstep(G, call, want, what, **expect):
    _gen_buf_stays(G, lambda: _step(G, call, want, what, **expect), what)


def _mprime(G, call, want, chains, keys, what):
    _gen_buf_stays(G, lambda: _prime(G, call, want, chains, keys, what), what)


def _sighting(keys, chains, nth):
    """what the nth call (0: the first) of a call with `keys` keys, each met chains / keys times, does to the counters: a key's first
    meeting runs eagerly and enters the table, its second is captured, every later one replays"""
    m = chains // keys
    assert m * keys == chains and m >= 1
    d = dict.fromkeys(COUNTERS, 0)
    for i in range(nth * m, (nth + 1) * m):
        for k in {0: ("eager", "n_keys"), 1: ("captures", "n_ready")}.get(i, ("replays",)):
            d[k] += keys
    return {k: n for k, n in d.items() if n}


def _again(G, call, want, chains, keys, what):
    """steps 4 - 6 of a move case: behind the move A is a first sighting, then captured, then replayed"""
    first = _sighting(keys, chains, 0)
    assert first["eager"] == keys and first["n_keys"] == keys
    for i, name in enumerate(("a first sighting", "captured", "replayed")):
        _mstep(G, call, want, f"{what}: A behind the move, {name}", **_sighting(keys, chains, i))


def _move_case(G, E, A, B, names, gens, what, keys_a=1, keys_b=1):
    """the whole case; A / B: call(engine) -> outputs.  -> (E's outputs and chain count for A, for B)"""
    (wa, na), (wb, nb) = _eager(E, A), _eager(E, B)
    assert _differ(wa, wb), f"{what}: A and B give the same result on the eager engine: the inputs need changing"
    _mprime(G, A, wa, na, keys_a, f"{what}: A")
    before = G.buffers()
    _mstep(G, B, wb, f"{what}: B (its own first sighting)", **_sighting(keys_b, nb, 0))
    _moved(G, before, names, what, **gens)
    _again(G, A, wa, na, keys_a, what)
    return (wa, na), (wb, nb)


# ---------------------------------------------------------------- engines ----------------------------------------------------------

@pytest.fixture(scope="module")
def t5_ref(ckpt_dirs):
    """(dims, state, E): E is shared and never holds a key; every test creates its own G, so its buffers start unallocated"""
    dims, state = t5_checkpoint(ckpt_dirs)
    E = t5_engine(dims, state, graphs=False)
    yield dims, state, E
    E.close()


@pytest.fixture
def t5(t5_ref):
    dims, state, E = t5_ref
    G = t5_engine(dims, state)
    yield dims, G, E
    G.close()


@pytest.fixture(scope="module", params=LLAMA_CKPTS)
def llama_ref(request, ckpt_dirs, tmp_path_factory):
    dims, state = llama_checkpoint(request.param, ckpt_dirs, tmp_path_factory.mktemp("graph_moves"))
    E = llama_engine(dims, state, graphs=False)
    yield dims, state, E
    E.close()


@pytest.fixture
def llama(llama_ref):
    dims, state, E = llama_ref
    G = llama_engine(dims, state)
    yield dims, G, E
    G.close()


# ---------------------------------------------------------------- T5: moves --------------------------------------------------------

def _greedy3(E, seqs, prefix, rows, v):
    """greedy with max_new 3 and an eos id nothing emits: all three steps run, one key each"""
    eos = _unused_id([E.greedy(seqs, prefix, 3, eos_id=v - 1)[0]], v)
    return _greedy(seqs, prefix, 3, eos, 0, rows)


def test_amax_move_under_greedy_step(t5):
    """GK_T5_GREEDY_STEP's key ends in amax_gen: a greedy call with 6 sequences behind one with 3 reallocates both arg-max buffers
    (two reserves: the counter steps by 2), and the 3-sequence call's three graphs - which hold the old addresses in the head
    GEMM's and the block reduction's arguments - must not replay."""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    A = _greedy3(E, _tokens(LEN_A[:3], v, 2000), [0], 3, v)
    B = _greedy3(E, _tokens(LEN_B + (77,), v, 2001), [9], 3, v)
    (_, na), (_, nb) = _move_case(G, E, A, B, AMAX, dict(amax_gen=2), "greedy 3 -> 6 sequences", keys_a=3, keys_b=3)
    assert na == 3 and nb == 3
    _report(G, since, "amax move under GK_T5_GREEDY_STEP")


def test_amax_move_under_greedy2(t5):
    """GK_T5_GREEDY2 (the speculative pass: one chain, one key, rows = sequences x (1 + candidates) arg-max rows): 6 sequences behind
    3 reallocate the arg-max pair.  The candidates hold every first token, so no fallback step runs."""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    a, b = _tokens(LEN_A[:3], v, 2010), _tokens(LEN_B + (77,), v, 2011)
    pa, pb, n_cand = [0, 9], [0, 31], 5
    eos = _unused_id([E.greedy(s, p, 2, eos_id=v - 1)[0] for s, p in ((a, pa), (b, pb))], v)

    def cands(seqs, prefix):
        t1 = sorted(set(int(t) for t in E.greedy(seqs, prefix, 2, eos_id=eos)[0][:, 0]))
        return (t1 + [i for i in range(60, 60 + 2 * n_cand + len(t1)) if i not in t1 and i != eos])[:n_cand]

    rows = len(pa) + n_cand
    A, B = _greedy(a, pa, 2, eos, 0, rows, cands(a, pa)), _greedy(b, pb, 2, eos, 0, rows, cands(b, pb))
    (_, na), (_, nb) = _move_case(G, E, A, B, AMAX, dict(amax_gen=2), "greedy2 3 -> 6 sequences")
    assert na == 1 and nb == 1, "a fallback step ran: the inputs need changing"
    _report(G, since, "amax move under GK_T5_GREEDY2")


def test_amax_move_under_generate_step(t5):
    """GK_T5_GENERATE_STEP's key holds amax_gen AND kv_gen.  A greedy call with 6 sequences behind a 3-sequence generate moves the
    arg-max pair and nothing else: the K / V cache stays, kv_gen stays, and the generate key must change all the same."""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    a = _tokens(LEN_A[:3], v, 2020)
    eos = _unused_id([E.generate(a, [0], 4, eos_id=v - 1)[0]], v)
    A = _generate(a, [0], 4, eos, 0)
    B = _greedy3(E, _tokens(LEN_B + (77,), v, 2021), [9], 3, v)
    (_, na), _ = _move_case(G, E, A, B, AMAX, dict(amax_gen=2), "generate 3 sequences, then greedy 6", keys_b=3)
    assert na >= 3
    _report(G, since, "amax move under GK_T5_GENERATE_STEP")


def test_kv_cache_only_move(t5):
    """kv_gen alone: behind a wide greedy call (the arg-max pair is large enough for everything after it), generate with 2 sequences
    and max_new 4, then the same sequences with max_new 12: the cache needs 13 positions per sequence where it had 5 and moves;
    the arg-max pair and gen_buf stay."""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    wide = _greedy3(E, _tokens((30, 9, 50, 12, 64, 3, 41, 20), v, 2030), [0], 3, v)
    _mstep(G, wide, _eager(E, wide)[0], "the wide greedy", eager=3, n_keys=3)
    a = _tokens((90, 128), v, 2031)
    eos = _unused_id([E.generate(a, [0], 12, eos_id=v - 1)[0]], v)
    A, B = _generate(a, [0], 4, eos, 0), _generate(a, [0], 12, eos, 0)
    _move_case(G, E, A, B, ("kv_cache",), dict(kv_gen=1), "generate max_new 4 -> 12")
    _report(G, since, "kv_cache-only move under GK_T5_GENERATE_STEP")


def test_gen_buf_never_moves(t5):
    """gen_buf (rk_t5_generate's int block) has no counter in any key: it is safe only because its size follows from max_seqs and
    max_dec_len alone.  After the first generate its address and capacity stay through a generate with max_seqs sequences, one
    with max_dec_len positions (16 prefix ids + 24 new), and the first call again - which, the other buffers having moved, is a
    first sighting - each with E's bits.  (_mstep asserts the same around every other call of this file.)"""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    assert G.buffers()["gen_buf"] == dict(addr=0, cap=0)
    a = _tokens((70, 33), v, 2040)
    eos = _unused_id([E.generate(a, [0], 4, eos_id=v - 1)[0]], v)
    A = _generate(a, [0], 4, eos, 0)
    wa, na = _eager(E, A)
    _mprime(G, A, wa, na, 1, "the first generate")
    first = G.buffers()
    assert first["gen_buf"]["addr"] and first["gen_buf"]["cap"]
    n_max, l_max = G.desc.max_seqs, G.desc.max_dec_len
    wide = _generate(_tokens((3,) * n_max, v, 2041), [0], 2, eos, 0)
    long_ = _generate(_tokens((40, 12), v, 2042), [0] + list(range(30, 30 + l_max - 25)), 24, eos, 0)
    for what, call in ((f"{n_max} sequences", wide), (f"{l_max} positions", long_)):
        want, n = _eager(E, call)
        _mstep(G, call, want, f"generate with {what}", **_sighting(1, n, 0))
    _moved(G, first, AMAX + ("kv_cache",), "max_seqs sequences, then max_dec_len positions", amax_gen=2, kv_gen=1)
    _again(G, A, wa, na, 1, "the first generate")
    assert G.buffers()["gen_buf"] == first["gen_buf"]
    _report(G, since, "gen_buf through max_seqs sequences and max_dec_len positions")


def test_logits_grow_and_keep_nothing_captured(t5):
    """logits (the qlm head's block statistics) has no counter either: qlm launches outside run_graphed, so no graph holds it.  A
    qlm with 6 sequences behind one with 2 reallocates logits, moves no counter of the table, and a primed score key replays
    unchanged behind it."""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    score = _score(_tokens(LEN_A, v, 2050), [0], [21, 22, 23])
    ws, ns = _eager(E, score)
    _mprime(G, score, ws, ns, 1, "score")
    small, big = _tokens((40, 77), v, 2051), _tokens(LEN_B + (90,), v, 2052)
    q2, q6 = (lambda e: (e.qlm(small, [11, 12, 1]),)), (lambda e: (e.qlm(big, [13, 14, 15, 1]),))
    (w2, n2), (w6, n6) = _eager(E, q2), _eager(E, q6)
    assert n2 == 0 and n6 == 0
    _mstep(G, q2, w2, "qlm, 2 sequences")
    before = G.buffers()
    assert before["logits"]["addr"]
    _mstep(G, q6, w6, "qlm, 6 sequences")
    _moved(G, before, ("logits",), "qlm 2 -> 6 sequences")
    _mstep(G, score, ws, "score behind the move of logits", replays=1)
    _mstep(G, q2, w2, "qlm, 2 sequences again")
    _report(G, since, "logits move (qlm), score replayed behind it")


# ---------------------------------------------------------------- Llama: moves -----------------------------------------------------

def _pregrow_amax(G, E, v):
    """the arg-max pair sized for 8 rows first, so that the cases about lkv / lpart / lints move nothing else"""
    wide = _tokens((5, 9, 3, 12, 7, 4, 8, 6), v, 2100)
    np.testing.assert_array_equal(G.greedy1(wide), E.greedy1(wide))


def _session_sighting(G, script, want, n, what, nth):
    _mstep(G, script, want, what, **_sighting(1, n, nth))


def test_llama_lints_only_move_at_equal_n_seq_and_P(llama):
    """One counter for three buffers, and max_new is not in GK_LLAMA_STEP's key {n_seq, P, amax_gen, lkv_gen}.  A: prompts of 40 and
    23 tokens, max_new 8 (P 48).  B: prompts of 24 and 11, max_new 24 (P 48): the cache and the partials fit, the int block
    [... | out[n_seq][max_new]] does not and moves; only lkv_gen keeps A's graph - which holds the old block's address in
    every argument of the advance kernel - from replaying.
    Behind the move A and B have the SAME key (same n_seq, P and counters), so the first sighting of that key is B's call, not A's
    next one: the assertion that no stale graph replays is B's (one new key, one eager step, one capture; with lkv_gen out of the
    key B would be all replays and no new key).  A then replays B's graph with its own shorter max_new (read from the block, not
    from an argument) and gives its own bits, as does B again, and A again.  A second move of lints alone with NO call sighting the
    new key - a session opened and closed - then makes A itself the first sighting."""
    dims, G, E = llama
    since, v = G.graph_stats(), dims.vocab
    _pregrow_amax(G, E, v)
    A, B = _llama_generate(_tokens((40, 23), v, 2110), 8, [], 0), _llama_generate(_tokens((24, 11), v, 2111), 24, [], 0)
    (wa, na), (wb, nb) = _eager(E, A), _eager(E, B)
    assert _differ(wa, wb) and na == 7 and nb == 23
    _mprime(G, A, wa, na, 1, "A")
    before = G.buffers()
    _mstep(G, B, wb, "B: the key's first sighting behind the move (a replay here would be A's stale graph)", **_sighting(1, nb, 0))
    _moved(G, before, ("lints",), "generate max_new 8 -> 24 at P 48", lkv_gen=1)
    _mstep(G, A, wa, "A on the larger block: B's graph, A's own max_new", replays=na)
    _mstep(G, B, wb, "B again", replays=nb)
    _mstep(G, A, wa, "A again", replays=na)
    before = G.buffers()
    G.session(2, 48, 60, [], 0).close()                                 # 16 + 18 + 2 x 60 ints (a capacity: nothing is decoded), 2 x 48 cache positions
    _moved(G, before, ("lints",), "a session of (2, 48, 60) opened and closed", lkv_gen=1)
    _again(G, A, wa, na, 1, "lints moved by a session")
    _report(G, since, f"lints-only move under GK_LLAMA_STEP, head_dim {dims.head_dim}")


@pytest.mark.parametrize("case", ["n_seq", "P", "lpart_without_lkv"])
def test_llama_lkv_and_lpart_moves(llama, case):
    """n_seq 2 -> 3 at P 48: cache, partials and int block all move (three reserves: lkv_gen + 3).  P 48 -> 138 at n_seq 2: the cache
    and - two chunks of 128 keys where there was one - the partials move, the int block (n_seq x max_new) stays.  lpart WITHOUT
    lkv: the partials go by n_seq x ceil(P / 128), the cache by n_seq x P, so 2 x 128 positions, then 3 x 80: 240 cache positions
    fit in 256, three partial chunks do not fit in two (the int block moves with them: 3 x 8 outputs where there were 2 x 8)."""
    dims, G, E = llama
    since, v = G.graph_stats(), dims.vocab
    _pregrow_amax(G, E, v)
    lens_a, lens_b, names, step = {"n_seq": ((40, 23), (40, 9, 31), ("lkv", "lpart", "lints"), 3),
                                   "P": ((40, 23), (130, 17), ("lkv", "lpart"), 2),
                                   "lpart_without_lkv": ((120, 61), (72, 30, 5), ("lpart", "lints"), 2)}[case]
    A, B = _llama_generate(_tokens(lens_a, v, 2120), 8, [], 0), _llama_generate(_tokens(lens_b, v, 2121), 8, [], 0)
    _move_case(G, E, A, B, names, dict(lkv_gen=step), f"generate {lens_a} -> {lens_b}")
    _report(G, since, f"{case} move under GK_LLAMA_STEP, head_dim {dims.head_dim}")


def test_llama_session_reopened_with_the_same_size_behind_a_move_of_lints(llama):
    """GK_LLAMA_SESSION_STEP's key is {n_slots, max_len, cap, amax_gen, lkv_gen}.  A session of (3, 96, 8) runs its script twice (a
    first sighting and a capture, then replays), closes; a generate with 2 prompts and max_new 8 needs 96 ints where the session
    needed 67 and moves lints alone; the session reopened with the same sizes starts as a first sighting, and its log is E's."""
    dims, G, E = llama
    since, v = G.graph_stats(), dims.vocab
    _pregrow_amax(G, E, v)
    s1 = _session_script(_tokens((30, 12, 5), v, 2130), [], 0)
    gen = _llama_generate(_tokens((40, 23), v, 2131), 8, [], 0)
    (w1, n1), (wg, ng) = _eager(E, s1), _eager(E, gen)
    assert n1 >= 3
    _session_sighting(G, s1, w1, n1, "the session's script: sighted and captured", 0)
    _session_sighting(G, s1, w1, n1, "the script again: replays", 1)
    before = G.buffers()
    _mstep(G, gen, wg, "the generate", **_sighting(1, ng, 0))
    _moved(G, before, ("lints",), "generate behind a session of (3, 96, 8)", lkv_gen=1)
    _session_sighting(G, s1, w1, n1, "the session reopened behind the move: a first sighting", 0)
    _session_sighting(G, s1, w1, n1, "and again: replays", 1)
    _mstep(G, gen, wg, "the generate again", replays=ng)
    _report(G, since, f"session reopened behind a move of lints, head_dim {dims.head_dim}")


def _pair_script(prompts, eos, pad, n_slots=2, max_len=64, cap=6):
    """a session of two slots: both prompts admitted at once, run and read until it is empty -> the whole log"""
    def call(eng):
        log = []
        with eng.session(n_slots, max_len, cap, eos, pad) as s:
            s.admit([prompts[0], prompts[1]], [0, 1], [6, 3])
            while s.busy:
                fin, steps = s.run()
                log.append(np.asarray([steps] + fin, dtype=np.int32))
                if steps:
                    log.append(eng.debug_read("llama_last", n_slots * eng.dims.hidden))
                for slot in fin:
                    log.append(np.asarray([slot] + [int(t) for t in s.read(slot)], dtype=np.int32))
        return log
    return call


def test_llama_session_reopened_with_another_size_and_no_move(llama):
    """Behind a captured session of (3, 96, 8) a smaller one, (2, 64, 6), fits every buffer: nothing moves, its key is a new one.
    (3, 96, 8) opened again - other prompts, an eos id, another pad id - then replays the old graph from its first step."""
    dims, G, E = llama
    since, v = G.graph_stats(), dims.vocab
    _pregrow_amax(G, E, v)
    p2 = _tokens((7, 41, 1), v, 2141)
    eos2 = int(E.generate([p2[1]], 3, [], 0)[0][0, 1])
    assert eos2 not in E.generate([p2[0]], 8, [], 0)[0], "slot 0 must outlast the late admit: the inputs need changing"
    s1, s2 = _session_script(_tokens((30, 12, 5), v, 2140), [], 0), _session_script(p2, [eos2], 7)
    small = _pair_script(_tokens((22, 9), v, 2142), [], 0)
    (w1, n1), (w2, n2), (ws, ns) = _eager(E, s1), _eager(E, s2), _eager(E, small)
    assert n1 >= 3 and ns >= 2 and (len(w1) != len(w2) or _differ(w1, w2))
    _session_sighting(G, s1, w1, n1, "session (3, 96, 8): sighted and captured", 0)
    _session_sighting(G, s1, w1, n1, "again: replays", 1)
    before = G.buffers()
    _session_sighting(G, small, ws, ns, "session (2, 64, 6): a new key", 0)
    _moved(G, before, (), "a smaller session")
    _mstep(G, s2, w2, "session (3, 96, 8) again, other prompts: a replay from its first step", replays=n2)
    _mstep(G, small, ws, "session (2, 64, 6) again", replays=ns)
    _mstep(G, s1, w1, "the first script again", replays=n1)
    _report(G, since, f"sessions of two sizes, no move, head_dim {dims.head_dim}")


def test_llama_amax_move_under_both_keys(llama):
    """amax_gen stands in GK_LLAMA_STEP's and GK_LLAMA_SESSION_STEP's key.  The buffers are sized for a generate with 2 prompts and
    a session of (3, 96, 8) first, both are primed (nothing moves meanwhile), then greedy1 with 8 prompts reallocates the arg-max
    pair and nothing else: the generate and the session are first sightings again."""
    dims, G, E = llama
    since, v = G.graph_stats(), dims.vocab
    gen = _llama_generate(_tokens((40, 23), v, 2150), 8, [], 0)
    s1 = _session_script(_tokens((30, 12, 5), v, 2151), [], 0)
    wide = _tokens((5, 9, 3, 12, 7, 4, 8, 6), v, 2152)
    (wg, ng), (w1, n1) = _eager(E, gen), _eager(E, s1)
    assert n1 >= 3 and ng >= 3
    G.session(3, 96, 8, [], 0).close()
    G.generate(_tokens((41, 23), v, 2153), 8, [], 0)                    # (lints grows here, under another key: P 49)
    sized, before = G.buffers(), G.graph_stats()
    _session_sighting(G, s1, w1, n1, "the session: sighted and captured", 0)
    _session_sighting(G, s1, w1, n1, "the session again", 1)
    _mprime(G, gen, wg, ng, 1, "the generate")
    _moved(G, sized, (), "priming behind the sizing calls")
    np.testing.assert_array_equal(G.greedy1(wide), E.greedy1(wide))
    _moved(G, sized, AMAX, "greedy1 with 8 prompts", amax_gen=2)
    assert {k: G.graph_stats()[k] - before[k] for k in ("n_keys", "failed")} == dict(n_keys=2, failed=0)
    _again(G, gen, wg, ng, 1, "the generate")
    _session_sighting(G, s1, w1, n1, "the session behind the move: a first sighting", 0)
    _session_sighting(G, s1, w1, n1, "the session again: replays", 1)
    _report(G, since, f"amax move under GK_LLAMA_STEP and GK_LLAMA_SESSION_STEP, head_dim {dims.head_dim}")


# ---------------------------------------------------------------- launches in flight -----------------------------------------------

def _launch(eng, seqs, prefix, ids, slot):
    eng.stage(seqs, slot=slot)
    eng.score_staged(prefix, ids, slot=slot)


def _staged(seqs, prefix, ids, slot):
    """stage, launch and read on one slot -> (scores,)"""
    def call(eng):
        _launch(eng, seqs, prefix, ids, slot)
        return (eng.read_scores(slot),)
    return call


def _long_pair(v, seed):
    """K0 on slot 0 and K0' on slot 1: 5 sequences of about 120 tokens at 17 decoder positions (a long decoder chain)"""
    return ((_tokens(LONG5, v, seed), DEC17, [21, 22, 23, 24]), (_tokens(LONG5B, v, seed + 1), DEC17, [33, 22, 50, 24]))


@pytest.mark.parametrize("passing_slot", [0, 1])
def test_eviction_with_both_slots_queued(t5, passing_slot):
    """evict_graphs destroys every instantiated graph but the passing key's after draining both decoder streams and slot 0's
    encoder stream.  K0 (slot 0) and K0' (slot 1) are primed, the table is filled to its bound with cheap first sightings, both are
    launched as replays and NOT read, and the key that passes the bound is launched behind them on `passing_slot`: the eviction
    destroys both graphs while their launches are queued or running.  The other slot's scores - a slot keeps its scores until its
    next launch - read afterwards must be E's; so must the passing key's; and K0 on slot 0 comes back eager, captured, replayed."""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    bound = G.graph_stats()["max_keys"]
    k = _long_pair(v, 2200)
    want = [_eager(E, _staged(*k[s], s))[0] for s in (0, 1)]
    assert _differ(want[0], want[1])
    for s in (0, 1):
        _mprime(G, _staged(*k[s], s), want[s], 1, 1, f"K0 on slot {s}")
    short = _tokens((9, 17, 5, 33, 12), v, 2202)
    others = [(n_seq, n_out) for n_out in range(1, 65) for n_seq in range(1, 6)]
    need = bound - G.graph_stats()["n_keys"]
    assert 0 < need < len(others)
    for n_seq, n_out in others[:need]:
        G.score(short[:n_seq], [0], list(range(40, 40 + n_out)))
    full = G.graph_stats()
    assert full["n_keys"] == bound and full["evictions"] == since["evictions"] and full["failed"] == 0, full
    n_seq, n_out = others[need]
    passing = (short[:n_seq], [0], list(range(40, 40 + n_out)))
    want_p = _eager(E, _staged(*passing, passing_slot))[0]
    for s in (0, 1):
        _launch(G, *k[s], s)
    queued = G.graph_stats()
    assert {c: queued[c] - full[c] for c in COUNTERS} == dict(dict.fromkeys(COUNTERS, 0), replays=2), "both launches are replays"
    _launch(G, *passing, passing_slot)
    now = G.graph_stats()
    assert now["evictions"] - queued["evictions"] == queued["n_ready"] and now["n_keys"] == 1 and now["n_keys"] <= bound, now
    assert now["eager"] - queued["eager"] == 1 and now["replays"] == queued["replays"] and now["failed"] == 0, now
    other = 1 - passing_slot
    _same((G.read_scores(other),), want[other], f"slot {other}'s queued replay, read across the eviction")
    _same((G.read_scores(passing_slot),), want_p, "the passing key's scores")
    k0 = _staged(*k[0], 0)
    _mstep(G, k0, want[0], "K0 after the eviction: a first sighting", eager=1, n_keys=1)
    _mstep(G, k0, want[0], "K0 captured again", captures=1, n_ready=1)
    _mstep(G, k0, want[0], "K0 replayed", replays=1)
    _report(G, since, f"eviction with both slots queued, the passing key on slot {passing_slot}")


@pytest.mark.parametrize("mover", ["greedy", "first_generate"])
def test_buffer_move_with_the_other_slot_queued(t5, mover):
    """Grown::reserve waits for every stream of both slots before it frees.  A long score is launched on slot 1 and not read; a
    blocking call on slot 0 then reallocates the arg-max pair (greedy with 6 sequences behind one with 2) or allocates the
    generate buffers for the first time (K / V cache, gen_buf, the decode ring); slot 1's scores, read afterwards, and the blocking
    call's result are E's, and slot 1's key still replays."""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    k1 = _long_pair(v, 2300)[1]
    s1 = _staged(*k1, 1)
    want1 = _eager(E, s1)[0]
    _mprime(G, s1, want1, 1, 1, "the long score on slot 1")
    small = _greedy3(E, _tokens((40, 77), v, 2302), [0], 3, v)
    _mstep(G, small, _eager(E, small)[0], "greedy, 2 sequences", eager=3, n_keys=3)
    if mover == "greedy":
        call, keys, names, gens = _greedy3(E, _tokens(LEN_B + (90,), v, 2303), [9], 3, v), 3, AMAX, dict(amax_gen=2)
    else:
        b = _tokens((70, 33), v, 2304)
        eos = _unused_id([E.generate(b, [0], 4, eos_id=v - 1)[0]], v)
        call, keys, names, gens = _generate(b, [0], 4, eos, 0), 1, ("kv_cache", "gen_buf"), dict(kv_gen=1)
    want, n = _eager(E, call)
    before, stats = G.buffers(), G.graph_stats()
    _launch(G, *k1, 1)
    got = call(G)
    _moved(G, before, names, f"{mover} with slot 1 queued", **gens)
    _same((G.read_scores(1),), want1, "slot 1's scores, read behind the move")
    _same(got, want, f"the blocking {mover}")
    exp = dict(dict.fromkeys(COUNTERS, 0), **_sighting(keys, n, 0))
    exp["replays"] += 1                                                 # slot 1's launch
    d = {c: G.graph_stats()[c] - stats[c] for c in COUNTERS}
    assert d == exp, f"counters moved by {d}, expected {exp}"
    _mstep(G, s1, want1, "slot 1 again", replays=1)
    _report(G, since, f"{mover} moves buffers with slot 1 queued")


def test_options_change_with_a_launch_queued(t5):
    """rk_engine_set_option starts a new epoch at once.  A primed key is launched on slot 1 (a replay), dec_gemv is set to 0 before the
    scores are read: they are the bits of the options the launch was made under; the next launch on slot 1 is a first sighting
    and gives the other family's bits.  (Two sequences at two positions: four decoder rows, the few-row GEMV
    family; the families differ in a few bits of the hidden rows, so the inputs are the first of eight seeds whose 64 scores differ on E.)"""
    dims, G, E = t5
    since, v = G.graph_stats(), dims.vocab
    try:
        for seed in range(2400, 2408):                                  # inputs whose SCORES differ between the two families on E
            k = (_tokens((90, 120), v, seed), [0, 7], list(range(21, 85)))
            call = _staged(*k, 1)
            E.set_option("dec_gemv", 1)
            on = _eager(E, call)[0]
            E.set_option("dec_gemv", 0)
            off = _eager(E, call)[0]
            if _differ(on, off):
                break
        assert _differ(on, off), "dec_gemv 1 and 0 give the same scores on the eager engine for every seed: the inputs need changing"
        _mprime(G, call, on, 1, 1, "dec_gemv = 1")
        stats = G.graph_stats()
        _launch(G, *k, 1)
        G.set_option("dec_gemv", 0)
        _same((G.read_scores(1),), on, "launched under dec_gemv = 1, read behind set_option")
        assert {c: G.graph_stats()[c] - stats[c] for c in COUNTERS} == dict(dict.fromkeys(COUNTERS, 0), replays=1)
        _mstep(G, call, off, "dec_gemv = 0: a first sighting", eager=1, n_keys=1)
        _mstep(G, call, off, "dec_gemv = 0: captured", captures=1, n_ready=1)
        _mstep(G, call, off, "dec_gemv = 0: replayed", replays=1)
    finally:
        G.set_option("dec_gemv", 1)
        E.set_option("dec_gemv", 1)
    _mstep(G, call, on, "dec_gemv = 1 again: a third epoch", eager=1, n_keys=1)
    _report(G, since, "options change with a launch queued on slot 1")
