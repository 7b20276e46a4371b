"""The sampling head on the GPU: sample_rows_kernel alone (rk_debug_sample) against the fp64 reference of tests/_sampling_ref.py -
kept sets, the draw's place in the reference CDF, frequencies - and end to end through rk_llama_generate_sampled and sampled
decoding sessions on the toy Llama / Qwen2 / Qwen3 models at both head widths: a row's tokens follow from its logits, (T, k, p),
its seed and its token index alone."""
import numpy as np
import pytest

import _sampling_ref as ref

pytestmark = pytest.mark.gpu

# (T, k, p): top-k only, top-p only, both, k = 1, k >= V with top-p, T = 0.01, T = 100 (with top-k alone and with top-p over a few ids:
# at T = 100 the whole vocabulary is nearly flat and no top-p boundary over it could keep the clearance below)
CONFIGS = [(1.0, 50, 1.0), (1.0, 0, 0.9), (0.6, 50, 0.9), (1.0, 1, 1.0), (1.0, 1 << 20, 0.6), (0.01, 0, 0.9), (100.0, 50, 1.0), (100.0, 5, 0.9)]
VOCABS = [8, 1000, 32000, 151936]
ROW_SEED = {8: 1, 1000: 3, 32000: 1, 151936: 2}           # make_rows seeds at which every row keeps the two clearances (asserted below)
N_DRAWS = 4096


@pytest.fixture(scope="module")
def eng():
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    dims = _synth.TOY_LLAMA
    e = RkLlamaEngine(dims, device=0, max_tokens=1024, max_seqs=8).load_state(_synth.synth_state_dict(dims, seed=929).items())
    yield e
    e.close()


_CACHE = {}


def _rows(V):
    """16 logit rows of V ids and their filtered references per configuration, computed once per vocabulary"""
    if V not in _CACHE:
        x = ref.make_rows(V, 16, ROW_SEED[V])
        _CACHE[V] = (x, {c: [ref.filter_row(x[r], *c) for r in range(16)] for c in CONFIGS})
    return _CACHE[V]


def _clear(row):
    """The conditions on the INPUTS (not tolerances on the kernel): the k-th and (k + 1)-th largest logit are more than 1e-3 apart -
    or bit-equal, a tie both sides keep by rule (the all-equal row) -, and the cumulative mass on either side of the top-p boundary
    is more than 1e-4 away from 1 - p."""
    return (row.k_gap > 1e-3 or row.k_gap == 0) and row.p_clear > 1e-4


@pytest.mark.parametrize("V", VOCABS)
def test_kept_sets_equal_the_reference(eng, V):
    x, refs = _rows(V)
    for c in CONFIGS:
        assert all(_clear(r) for r in refs[c]), (V, c, [(r.k_gap, r.p_clear) for r in refs[c]])
    for c in CONFIGS:
        for n in (1, 3, 16):
            tok, kk, kp = eng.debug_sample(x[:n], *c, seeds=np.arange(n) + 77, index=np.arange(n))
            want_k = [int(r.kept_k.sum()) for r in refs[c][:n]]
            want_p = [int(r.kept.sum()) for r in refs[c][:n]]
            assert list(kk) == want_k and list(kp) == want_p, (V, c, n, list(kk), want_k, list(kp), want_p)
            assert all(refs[c][r].kept[tok[r]] for r in range(n)), (V, c, n, list(tok))
    # what the rows are there for
    one = refs[(1.0, 0, 0.9)]
    assert one[2].kept.all() and one[3].kept.sum() == 1 and refs[(1.0, 1, 1.0)][2].kept.all()
    assert np.isinf(x[4]).any() and (x[1] < 0).all() and (x[0] > 0).any() and (x[0] < 0).any()


@pytest.mark.parametrize("V", VOCABS)
def test_draw_lies_in_the_reference_cdf_interval(eng, V):
    """4 096 (seed, index) pairs per configuration in one call, 256 per logit row.  The device's token must be kept in the reference
    and u Z_ref must lie in the token's fp64 CDF interval widened by eps Z_ref.  eps follows from the kernel (DESIGN.md section 3,
    "Sampling head"): every sum is an exact integer sum of 2^-40 fixed-point weights, so the error is the weights' own -
    (1 + |a_i|) 2^-23 relative for w_i = expf(a_i), a_i = (x_i - max) / T (one rounding each in the subtraction and the division,
    1 ulp in expf), and 2^-40 of truncation per id - in the running sum and in Z alike: eps = 2 ((1 + S) 2^-23 + V 2^-40) with
    S = sum w_i |a_i| / Z of the row.  It is below the order-free bound (V + 100) 2^-24 at every size here."""
    x, refs = _rows(V)
    rng = np.random.default_rng(V)
    seeds = rng.integers(0, 2 ** 63, N_DRAWS, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, N_DRAWS, dtype=np.uint64)
    index = rng.integers(0, 1 << 20, N_DRAWS).astype(np.int32)
    index[:8] = [0, 1, 2, 3, 2 ** 31 - 1, 4095, 4096, 65535]
    u = ref.uniform(seeds, index)
    for c in CONFIGS:
        tok, _, _ = eng.debug_sample(x, *c, seeds=seeds, index=index)
        outside = 0
        for lr in range(16):
            row, sel = refs[c][lr], np.arange(lr, N_DRAWS, 16)
            t = tok[sel]
            assert ((t >= 0) & (t < V)).all() and row.kept[t].all(), (V, c, lr)
            lo, hi = row.interval(t)
            target = u[sel] * row.Z
            eps = 2 * ((1 + row.spread) * 2.0 ** -23 + V * 2.0 ** -40)
            assert eps <= (V + 100) * 2.0 ** -24
            assert ((target >= lo - eps * row.Z) & (target <= hi + eps * row.Z)).all(), (V, c, lr)
            outside += int(((target < lo) | (target >= hi)).sum())
        print(f"V {V} {c}: {outside} of {N_DRAWS} draws outside the un-widened interval")
        assert outside <= N_DRAWS // 100, (V, c, outside)


def test_frequencies_follow_the_kept_distribution(eng):
    """V = 64, 8 ids kept, 16 384 fixed seeds in one call: every kept id's count within 6 binomial standard deviations of N q_i -
    for the reference sampler on the CPU first, then for the device."""
    N = 16384
    rng = np.random.default_rng(64)
    x = rng.normal(0.0, 1.5, (1, 64)).astype(np.float32)
    row = ref.filter_row(x[0], 0.8, 8, 1.0)
    assert row.kept.sum() == 8 and row.k_gap > 1e-3
    q = row.w / row.Z
    seeds = np.arange(N, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)
    index = (np.arange(N) % 97).astype(np.int32)
    sd = np.sqrt(N * q * (1 - q))

    def check(tokens, who):
        counts = np.bincount(tokens, minlength=64)
        assert counts[~row.kept].sum() == 0, who
        dev = np.abs(counts - N * q)[row.kept] / sd[row.kept]
        print(f"{who}: largest deviation {dev.max():.2f} sd")
        assert (dev < 6).all(), (who, dev)

    check(row.draw(ref.uniform(seeds, index)), "reference")
    tok, kk, kp = eng.debug_sample(x, 0.8, 8, 1.0, seeds=seeds, index=index)
    assert (kk == 8).all() and (kp == 8).all()
    check(tok, "device")


def test_debug_sample_refuses_bad_arguments(eng):
    x = np.zeros((1, 8), np.float32)
    for T, k, p in ((0.0, 0, 1.0), (-1.0, 0, 1.0), (float("nan"), 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5)):
        assert eng.debug_sample(x, T, k, p, seeds=[1], index=[0], check=False) == -1
    assert eng.debug_sample(x, 1.0, 0, 1.0, seeds=[1], index=[-1], check=False) == -1


# ---- end to end ------------------------------------------------------------------------------------------------------------
SAMPLING = (2.0, 20, 0.95)            # (a temperature at which the toy models' rows leave the greedy path)
LENS, MAX_NEW, PAD = (5, 64, 129, 33), 12, 0
SEEDS = [0x0123456789ABCDEF, 2 ** 64 - 1, 7, 0xDEADBEEF00000000]


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 1024)
    kw.setdefault("max_seqs", 8)
    return RkLlamaEngine(dims, device=0, **kw).load_state(state.items())


@pytest.fixture(scope="module", params=["toy-llama", "toy-qwen2", "toy-qwen3", "toy-llama-hd64", "toy-qwen2-hd64"])
def model(request):
    """dims, state, four prompts and - computed once - every prompt's sampled tokens alone (the reference of the tests below)"""
    from llmrankers import _synth
    dims = _synth.NAMED_DIMS[request.param]
    state = _synth.synth_state_dict(dims, seed=929)
    base = _synth.synth_token_batch(1, 200, 200, dims.vocab, seed=17)[0]
    prompts = [list(base[:n]) for n in LENS]
    eng = _engine(dims, state)
    eng.set_sampling(*SAMPLING)
    alone = [eng.generate([p], MAX_NEW, [], PAD, seeds=[s])[0][0].tolist() for p, s in zip(prompts, SEEDS)]
    yield request.param, dims, state, prompts, alone, eng
    eng.close()


def test_determinism_and_batch_independence(model):
    _, dims, state, prompts, alone, eng = model
    eng.set_sampling(*SAMPLING)
    a, steps = eng.generate(prompts, MAX_NEW, [], PAD, seeds=SEEDS)
    b, _ = eng.generate(prompts, MAX_NEW, [], PAD, seeds=SEEDS)
    assert steps == MAX_NEW and np.array_equal(a, b)
    assert a.tolist() == alone                                          # alone == in a batch of 4, per seed
    perm = [2, 0, 3, 1]                                                 # ... and in any row of it
    c, _ = eng.generate([prompts[i] for i in perm], MAX_NEW, [], PAD, seeds=[SEEDS[i] for i in perm])
    assert c.tolist() == [alone[i] for i in perm]
    assert ((a >= 0) & (a < dims.vocab)).all()


def test_session_equals_generate_sampled(model):
    """a sampled session with 1 slot (every prompt re-uses it) and with 4: a prompt's tokens == rk_llama_generate_sampled's alone"""
    _, dims, state, prompts, alone, eng = model
    eng.set_sampling(*SAMPLING)
    new = [MAX_NEW, 3, MAX_NEW, 7]
    for n_slots in (1, 4):
        got = {}
        with eng.session(n_slots, 256, MAX_NEW, [], PAD) as s:
            nxt, owner = 0, {}
            while nxt < len(prompts) or s.busy:
                free = s.free_slots()
                take = list(range(nxt, min(nxt + len(free), len(prompts))))
                if take:
                    s.admit([prompts[r] for r in take], free[:len(take)], [new[r] for r in take], seeds=[SEEDS[r] for r in take])
                    owner.update(zip(free, take))
                    nxt += len(take)
                finished, _ = s.run()
                for slot in finished:
                    got[owner.pop(slot)] = s.read(slot).tolist()
        for r in range(len(prompts)):
            assert got[r] == alone[r][:new[r]], (n_slots, r, got[r], alone[r])
    # a slot that held a long row, then another prompt with another seed: nothing of the first row or its seed is left
    with eng.session(1, 256, MAX_NEW, [], PAD) as s:
        s.admit([prompts[2]], [0], [MAX_NEW], seeds=[SEEDS[0]])
        s.run()
        s.read(0)
        s.admit([prompts[0]], [0], [MAX_NEW], seeds=[SEEDS[0]])
        s.run()
        assert s.read(0).tolist() == alone[0]


def test_graph_replay_equals_eager(model):
    """dec_graph 0 against 1 on separate engines: the step's token index comes from the device positions, so a replayed graph
    moves along the Philox stream without a host write"""
    _, dims, state, prompts, alone, _ = model
    out = {}
    for graph in (0, 1):
        eng = _engine(dims, state)
        eng.set_option("dec_graph", graph)
        eng.set_sampling(*SAMPLING)
        for _ in range(3):                                              # eager, captured, replayed
            out[graph] = eng.generate(prompts, MAX_NEW, [], PAD, seeds=SEEDS)[0].tolist()
            assert out[graph] == alone
        st = eng.graph_stats()
        assert (st["replays"] > 0 and st["failed"] == 0) if graph else (st["captures"] == 0 and st["replays"] == 0), st
        eng.close()
    assert out[0] == out[1]


def test_greedy_equivalence(model):
    _, dims, state, prompts, alone, eng = model
    eng.set_sampling(0, 0, 1)
    greedy, gsteps = eng.generate(prompts, MAX_NEW, [], PAD)
    off, osteps = eng.generate(prompts, MAX_NEW, [], PAD, seeds=SEEDS)            # sampling off: the greedy form, seeds ignored
    assert np.array_equal(greedy, off) and gsteps == osteps
    eng.set_sampling(1.0, 1, 1.0)                                                 # k = 1 keeps the arg-max alone
    k1, _ = eng.generate(prompts, MAX_NEW, [], PAD, seeds=SEEDS)
    assert np.array_equal(greedy, k1)
    assert np.array_equal(eng.generate(prompts, MAX_NEW, [], PAD)[0], greedy)     # the plain form stays greedy whatever is set
    eos = [int(greedy[1, 4])]                                                     # ... and the stop rules are the greedy call's
    a, sa = eng.generate(prompts, MAX_NEW, eos, PAD)
    b, sb = eng.generate(prompts, MAX_NEW, eos, PAD, seeds=SEEDS)
    assert np.array_equal(a, b) and sa == sb
    eng.set_sampling(*SAMPLING)


def test_seeds_matter_on_flat_logits():
    from llmrankers import _synth
    dims = _synth.TOY_LLAMA
    eng = _engine(dims, _synth.synth_state_dict(dims, seed=929, gain=0.1))
    eng.set_sampling(1.0, 0, 1.0)
    p = list(_synth.synth_token_batch(1, 40, 40, dims.vocab, seed=17)[0])
    a = eng.generate([p, p], 16, [], PAD, seeds=[1, 2])[0]
    assert not np.array_equal(a[0], a[1])
    b = eng.generate([p, p], 16, [], PAD, seeds=[2, 1])[0]
    assert np.array_equal(a[0], b[1]) and np.array_equal(a[1], b[0])
    eng.close()


def test_sampled_ids_are_plausible_for_the_oracle(model):
    """the sampled sequence teacher-forced through the numpy oracle: every sampled id's oracle logit is at least the min(k, V)-th
    largest oracle logit - 2 delta, delta = the step-logit bound of DESIGN.md section 4 (4e-3 x scale).  No id is exempt."""
    name, dims, state, prompts, alone, _ = model
    from oracle.llama_numpy import LlamaOracle
    if dims.qk_norm:
        from _qwen3_ref import Qwen3Oracle as Oracle
    elif dims.qkv_bias:
        from _qwen2_ref import Qwen2Oracle as Oracle
    else:
        Oracle = LlamaOracle
    orc = Oracle(dims, state)
    k = min(SAMPLING[1], dims.vocab)
    for p, row in zip(prompts, alone):
        lg = orc.last_logits([list(p) + row[:j] for j in range(MAX_NEW)])
        for j, t in enumerate(row):
            delta = 4e-3 * float(np.abs(lg[j]).max())
            assert lg[j, t] >= np.sort(lg[j])[-k] - 2 * delta, (name, len(p), j, t)


def test_refusals_leave_everything_as_it_was(model):
    from llmrankers import _synth
    from llmrankers._engine import RkEngine, RkError
    _, dims, state, prompts, alone, eng = model

    def code(fn, *a, **kw):
        """the refusal's code; no grown buffer moved or grew under it"""
        before = eng.buffers()
        with pytest.raises(RkError) as ei:
            fn(*a, **kw)
        assert eng.buffers() == before
        return ei.value.code

    eng.set_sampling(0, 0, 1)
    greedy0 = eng.generate(prompts[:1], MAX_NEW, [], PAD)[0][0].tolist()
    eng.set_sampling(*SAMPLING)
    for bad in ((-0.5, 0, 1.0), (float("nan"), 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.01)):
        assert code(eng.set_sampling, *bad) == -1
    assert eng.generate(prompts[:1], MAX_NEW, [], PAD, seeds=SEEDS[:1])[0][0].tolist() == alone[0]       # the old setting still holds
    import ctypes as C
    from llmrankers._engine import _i32p, pack_ragged
    tok, off = pack_ragged(prompts[:1])
    out, steps = np.full((1, MAX_NEW), -7, np.int32), C.c_int32(-7)
    rc = eng.lib.rk_llama_generate_sampled(eng.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), 1, MAX_NEW, 0, None, 0, PAD,
                                           out.ctypes.data_as(_i32p), C.byref(steps), None)
    assert rc == -1 and (out == -7).all() and steps.value == -7                                          # null seeds
    with eng.session(2, 256, MAX_NEW, [], PAD) as s:                                                     # a sampled session
        assert code(eng.set_sampling, 1.0, 0, 1.0) == -4
        assert code(s.admit, prompts[:1], [0], [MAX_NEW]) == -4 and not s.busy                           # plain admit
        sl, mn = np.array([0], np.int32), np.array([MAX_NEW], np.int32)
        assert eng.lib.rk_llama_session_admit_sampled(eng.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p),
                                                      mn.ctypes.data_as(_i32p), 1, None) == -1
        assert s.run() == ([], 0)                                                                        # nothing was admitted
        s.admit(prompts[:1], [1], [MAX_NEW], seeds=SEEDS[:1])
        s.run()
        assert s.read(1).tolist() == alone[0]
    eng.set_sampling(0, 0, 1)
    with eng.session(2, 256, MAX_NEW, [], PAD) as s:                                                     # a greedy session
        assert code(s.admit, prompts[:1], [0], [MAX_NEW], seeds=SEEDS[:1]) == -4 and not s.busy
        assert s.run() == ([], 0)
        s.admit(prompts[:1], [0], [MAX_NEW])
        s.run()
        assert s.read(0).tolist() == greedy0
    eng.set_sampling(*SAMPLING)
    t5 = RkEngine(_synth.TOY_GATED_UNTIED, device=0, max_tokens=256, max_seqs=4, max_dec_len=4)
    assert code(RkLlamaEngineView(t5).set_sampling, 1.0, 0, 1.0) == -4
    t5.close()


class RkLlamaEngineView:
    """set_sampling on an engine of the other family (the Python T5 wrapper has no such method: the C call is what refuses)"""

    def __init__(self, eng):
        self.eng = eng

    def set_sampling(self, T, k, p):
        self.eng._chk(self.eng.lib.rk_llama_set_sampling(self.eng.h, float(T), int(k), float(p)))
