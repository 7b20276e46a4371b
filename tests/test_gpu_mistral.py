"""Sliding-window attention (Mistral family) on the HIP engine, end to end and at kernel level: the windowed entries of the prefill
kernels (attn_causal_dma_kernel<., 1>, attn_causal_tile_kernel<64, 1>) and of the decode step (attn_dec_cached_win_kernel,
attn_dec_combine_win_kernel) behind rk_llama_set_sliding_window.  Two toys - TOY_LLAMA's shape (128-wide heads) and TOY_LLAMA_HD64's
(64-wide) - at windows W = 1, 5, 33, 64, 100, 128, 129, 200: below a wave's 32 queries, off every 32 / 64 / 128 boundary, exactly one
decode chunk, one key into the next chunk, spanning two chunks.

Against the fp32 oracle with the window mask (tests/_mistral_ref.py) under the bounds the window-less kernels are held to
(tests/test_gpu_llama_listwise.py, tests/test_gpu_llama_hd64.py); against the window-less engine on the same weights, byte for byte,
wherever no sequence is longer than the window - also for the short sequences of a call that a longer one flips to the windowed
kernels; against the fp64 references of tests/_attn_ref*.py through rk_debug_attn kinds 4 and 5 (tests/_attn_ref_win.py).

The module stops at the first device error: nothing more is started on a device that has faulted."""
import dataclasses

import numpy as np
import pytest

from llmrankers import _synth
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu
FLOOR = 5e-3              # fp16 noise floor of the toy scale (test_gpu_rerank.py)
BOUND = 4e-3              # x logit scale: what the window-less prefill and step are held to
CHUNK = 128               # attn_dec_cached_kernel: keys per workgroup (csrc/llama_kernels.h: LDC_CHUNK)
ERR_INVALID, ERR_HIP, ERR_STATE = -1, -3, -4
TOYS = ["toy-mistral", "toy-mistral-hd64"]
WINDOWS = [1, 5, 33, 64, 100, 128, 129, 200]
SEED = 929
TOKEN_SEED = 940          # the token test's weights: see test_tokens_vs_oracle_greedy1_and_the_reprefill_loop


def _guard(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{getattr(fn, '__name__', fn)}: {err}", returncode=3)
        raise


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 32768)
    kw.setdefault("max_seqs", 128)
    return _guard(RkLlamaEngine(dims, device=0, **kw).load_state, state.items())


def _oracle(dims, state):
    from _mistral_ref import MistralOracle
    return MistralOracle(dims, state)


def _all_logits(eng, seqs, vocab):
    return np.concatenate([_guard(eng.last_logits, seqs, list(range(v0, v0 + 64))) for v0 in range(0, vocab, 64)], axis=1)


def _last(eng, n, hidden):
    return eng.debug_read("llama_last", n * hidden).reshape(n, hidden).copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module", params=TOYS)
def toy(request):
    """base dims (the tests put their own window), state, head, one 700-token sequence - computed once, never modified"""
    dims = _synth.NAMED_DIMS[request.param]
    state = _synth.synth_state_dict(dims, seed=SEED)
    base = _synth.synth_token_batch(1, 700, 700, dims.vocab, seed=17)[0]
    return dims, state, np.asarray(state["lm_head.weight"], dtype=np.float32), base


def test_dims():
    a, b = (_synth.NAMED_DIMS[n] for n in TOYS)
    assert dataclasses.replace(a, sliding_window=0, mistral=False) == _synth.TOY_LLAMA
    assert dataclasses.replace(b, sliding_window=0, mistral=False) == _synth.TOY_LLAMA_HD64
    assert a.mistral and b.mistral and a.sliding_window > 0 and b.sliding_window > 0


@pytest.mark.parametrize("W", WINDOWS)
def test_prefill_last_logits_vs_oracle(toy, W):
    """prefixes of one 700-token sequence in ONE call: 1, W - 1 .. W + 1, W + 31 .. W + 33, 2 W, 700 and both sides of every multiple
    of 128; every vocabulary row of the last position against the oracle with the window mask"""
    base_dims, state, _, base = toy
    dims = dataclasses.replace(base_dims, sliding_window=W)
    lens = sorted(n for n in set([1, W - 1, W, W + 1, W + 31, W + 32, W + 33, 2 * W, 700] + [e + d for e in (128, 256, 384, 512, 640) for d in (-1, 0, 1)])
                  if 1 <= n <= 700)
    seqs = [base[:n] for n in lens]
    eng = _engine(dims, state)
    got = _all_logits(eng, seqs, dims.vocab)
    eng.close()
    want = _oracle(dims, state).last_logits(seqs)
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"W = {W}: max |logit - oracle| = {err:.3e} at scale {scale:.2f} (bound {BOUND * scale:.3e})")
    assert got.shape == want.shape
    assert err < BOUND * scale, (W, err, scale)


@pytest.mark.parametrize("W", WINDOWS)
def test_step_kernel_vs_oracle_on_both_sides_of_the_window_and_of_every_chunk(toy, W):
    """the loop of test_step_kernel_vs_oracle_at_every_chunk_count: max_new 1 .. 6, no EOS; the final-normed rows the LAST step's head
    read, times head^T, against the oracle's logits of prompt + generated tokens.  Prompt lengths put pos on both sides of W and of
    every multiple of 128 up to 640"""
    base_dims, state, head, base = toy
    dims = dataclasses.replace(base_dims, sliding_window=W)
    lens = sorted(n for n in set([1, 2, W - 6, W - 5, W - 2, W - 1, W, W + 1, 2 * W] + [k * CHUNK + d for k in range(1, 6) for d in (-6, -5, -2, -1, 0, 1)]
                                 + [694]) if 1 <= n <= 694)
    seqs = [base[:n] for n in lens]
    eng = _engine(dims, state)
    orc = _oracle(dims, state)
    for max_new in range(1, 7):
        toks, steps = _guard(eng.generate, seqs, max_new, [], 0)
        assert steps == max_new and toks.shape == (len(seqs), max_new)
        got = _last(eng, len(seqs), dims.hidden) @ head.T
        want = orc.last_logits([list(s) + [int(t) for t in toks[b, :max_new - 1]] for b, s in enumerate(seqs)])
        scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
        print(f"W = {W}, max_new {max_new}: max |logit - oracle| = {err:.3e} at scale {scale:.2f}")
        assert err < BOUND * scale, (W, max_new, err, scale)
    eng.close()


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("name", TOYS)
def test_tokens_vs_oracle_greedy1_and_the_reprefill_loop(name, W):
    """5 prompts of W - 10, W - 1, W, W + 1, W + 15 tokens (at least 1), 20 new tokens: generated tokens == the oracle's up to the first
    step whose ORACLE margin is under the floor; column 0 == greedy1; == a greedy1 re-prefill loop over the checked steps.  At least 75
    of the 100 steps must be checked, at every window.  Synth seed 929 does not give that from the oracle alone (toy-mistral 100 / 81 /
    73 / 82 / 100 / 100 / 100 / 100 at W = 1 .. 200, toy-mistral-hd64 100 / 77 / 100 / 100 / 80 / 67 / 58 / 100), nor do 930 .. 939; seed
    940 is the next that does: 100 / 100 / 96 / 100 / 86 / 93 / 100 / 98 and 100 / 93 / 79 / 75 / 83 / 100 / 98 / 84."""
    from _llama_gen_stub import oracle_greedy
    dims = dataclasses.replace(_synth.NAMED_DIMS[name], sliding_window=W)
    state = _synth.synth_state_dict(dims, seed=TOKEN_SEED)
    orc = _oracle(dims, state)
    seqs = [_synth.synth_token_batch(1, n, n, dims.vocab, seed=7 + i)[0] for i, n in enumerate(max(1, W + d) for d in (-10, -1, 0, 1, 15))]
    eng = _engine(dims, state, max_tokens=4096, max_seqs=16)
    gen, steps = _guard(eng.generate, seqs, 20, [], 0)
    assert steps == 20
    np.testing.assert_array_equal(gen[:, 0], _guard(eng.greedy1, seqs))
    checked = 0
    for b, s in enumerate(seqs):
        toks, margins = oracle_greedy(orc, s, 20)
        low = next((i for i, m in enumerate(margins) if m < FLOOR), len(margins))
        assert list(gen[b, :low]) == toks[:low], (W, b, low)
        cur = list(s)
        for t in range(low):
            assert int(_guard(eng.greedy1, [cur])[0]) == int(gen[b, t]), (W, b, t)
            cur.append(int(gen[b, t]))
        checked += low
    eng.close()
    print(f"W = {W}: {checked} of 100 steps checked")
    assert checked >= 75, (W, checked)


def test_a_window_no_shorter_than_every_sequence_changes_no_byte(toy):
    """W = 700 >= every length + new token: last logits, generated tokens and llama_last == the window-less engine's, bytes"""
    base_dims, state, _, base = toy
    seqs = [base[:n] for n in (1, 31, 64, 129, 300, 513, 690)]
    ids = list(range(0, base_dims.vocab, base_dims.vocab // 64))
    res = []
    for W in (0, 700):
        eng = _engine(dataclasses.replace(base_dims, sliding_window=W), state, max_tokens=4096, max_seqs=16)
        lg = _guard(eng.last_logits, seqs, ids)
        gen, _ = _guard(eng.generate, seqs, 6, [], 0)
        res.append((lg, gen, _last(eng, len(seqs), base_dims.hidden)))
        eng.close()
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0]))
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert np.array_equal(_bits(res[0][2]), _bits(res[1][2]))


def _shorts(W):
    """sequences that stay inside the window while `new` tokens are generated: lengths, new"""
    lens = sorted({1, max(1, W // 2), max(1, W - 6)})
    return lens, min(5, W - max(lens) + 1)


@pytest.mark.parametrize("W", WINDOWS)
def test_short_sequences_of_a_windowed_call_equal_the_windowless_engine(toy, W):
    """one sequence longer than W (it flips the call to the windowed prefill kernel) with sequences that never leave the window: theirs
    are the window-less engine's bytes - last logits, generated tokens, llama_last - and a session's tokens; and each sequence alone
    on the windowed engine equals itself in the mixed call (bytes), a DecodePool run equals generate (tokens)"""
    from llmrankers._runtime import LlamaRuntime
    base_dims, state, _, base = toy
    lens, new = _shorts(W)
    short = [base[100:100 + n] for n in lens]
    mixed = short[:1] + [base[:W + 70]] + short[1:]                 # the long one in the middle of the call
    where = [0] + list(range(2, len(mixed)))
    ids = list(range(0, base_dims.vocab, base_dims.vocab // 64))
    plain = _engine(dataclasses.replace(base_dims, sliding_window=0), state, max_tokens=4096, max_seqs=16)
    want_lg = _guard(plain.last_logits, short, ids)
    want_gen, _ = _guard(plain.generate, short, new, [], 0)
    want_last = _last(plain, len(short), base_dims.hidden)
    plain.close()
    eng = _engine(dataclasses.replace(base_dims, sliding_window=W), state, max_tokens=4096, max_seqs=16)
    lg = _guard(eng.last_logits, mixed, ids)
    gen, _ = _guard(eng.generate, mixed, new, [], 0)
    last = _last(eng, len(mixed), base_dims.hidden)
    assert np.array_equal(_bits(lg[where]), _bits(want_lg)), W
    np.testing.assert_array_equal(gen[where], want_gen)
    assert np.array_equal(_bits(last[where]), _bits(want_last)), W
    for b, s in enumerate(mixed):                                      # batch independence on the windowed engine, the long one included
        assert np.array_equal(_bits(_guard(eng.last_logits, [s], ids)), _bits(lg[b:b + 1])), (W, b)
        solo, _ = _guard(eng.generate, [s], new, [], 0)
        np.testing.assert_array_equal(solo[0], gen[b])
        assert np.array_equal(_bits(_last(eng, 1, base_dims.hidden)), _bits(last[b:b + 1])), (W, b)
    with eng.session(len(mixed), 1024, 8, [], 0) as s:
        _guard(s.admit, [list(x) for x in mixed], list(range(len(mixed))), [new] * len(mixed))
        got = {}
        while s.busy:
            for slot in _guard(s.run)[0]:
                got[slot] = [int(t) for t in s.read(slot)]
    for b in range(len(mixed)):
        assert got[b] == [int(t) for t in gen[b]], (W, b)
    long_new = 12                                                      # a pool: the long request decodes beyond the window
    alone, _ = _guard(eng.generate, [mixed[1]], long_new, [], 0)
    with LlamaRuntime.from_engine(eng).open_pool(16, [], 0, n_slots=2) as pool:
        for b, x in enumerate(mixed):
            pool.submit(b, x, long_new if b == 1 else new)
        done = {}
        while pool.pending():
            done.update({k: [int(t) for t in v] for k, v in _guard(pool.wait)})
    eng.close()
    assert done[1] == [int(t) for t in alone[0]], W
    for b in where:
        assert done[b] == [int(t) for t in gen[b]], (W, b)


# ---- kernel level: rk_debug_attn kinds 4 and 5 on windowed engines against fp64 -------------------------------------------------
def _ref(dims):
    import _attn_ref as A
    import _attn_ref_hd64 as D
    return A if dims.head_dim == 128 else D


def _sentinel(a):
    from _attn_ref import SENTINEL
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all())


def _pargs(p):
    return dict(n_seq=p.n_seq, H=p.H, n_kv=p.n_kv, q=p.q, out=p.out, band_rows=p.band, ldq=p.ldq, ldctx=p.ldctx, seq_off=p.seq_off)


def _sargs(p):
    return dict(n_seq=p.n_seq, H=p.H, n_kv=p.n_kv, q=p.q, out=p.out, band_rows=p.band, P=p.P, ldq=p.ldq, ldctx=p.ldctx, pos=p.pos, cos=p.cos,
                sin=p.sin, qkv_bias=p.qkv_bias, cache=p.cache)


@pytest.mark.parametrize("W", [1, 33, 64, 100, 129])
def test_prefill_kernels_vs_fp64(toy, W):
    """kind 4 on a windowed engine, tier R: calls whose longest sequence exceeds W are planned windowed (out_kind + 4) and held to the
    fp64 reference with the window; calls that fit are planned plain; guard bands untouched; each sequence alone the same bytes"""
    import _attn_ref_win as X
    base_dims, state, _, _ = toy
    M = _ref(base_dims)
    plain_kind = 1 if base_dims.head_dim == 128 else 2
    eng = _engine(dataclasses.replace(base_dims, sliding_window=W), state, max_tokens=4096, max_seqs=16)
    for n, (heads, lens) in enumerate([((4, 2), [W + 1]), ((7, 1), [W, 3 * W + 5, 1]), ((4, 2), [31, W + 200, 64, W + 63]), ((3, 3), [513])]):
        p = M.build_llama(700 + n, heads[0], heads[1], lens, "R", band=8)
        what = f"windowed prefill W = {W} {heads} {lens}"
        plan = eng.debug_attn(M.LLAMA, plan_only=True, **_pargs(p))
        assert plan["kind"] == plain_kind + (4 if max(lens) > W else 0), (what, plan)
        out = _guard(eng.debug_attn, M.LLAMA, **_pargs(p))["out"]
        assert _sentinel(out[:p.band]) and _sentinel(out[-p.band:]), f"{what}: a guard band of the output was written"
        inner = out[p.band:-p.band]
        print(f"{what}: ratio {X.judge(M, p, W, inner, what):.2f}")
        for b in range(p.n_seq):
            s = X.alone(p, b)
            solo = _guard(eng.debug_attn, M.LLAMA, **_pargs(s))["out"][s.band:-s.band]
            assert solo.tobytes() == inner[int(p.seq_off[b]):int(p.seq_off[b + 1])].tobytes(), f"{what}: sequence {b} alone gives other bytes"
    p = M.build_llama(750, 4, 2, [1, max(1, W - 1), W], "R", band=8)      # fits the window: the plain kernel
    assert eng.debug_attn(M.LLAMA, plan_only=True, **_pargs(p))["kind"] == plain_kind
    eng.close()


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("W", [1, 33, 100, 128, 129, 200])
def test_step_kernels_vs_fp64(toy, W, bias):
    """kind 5 on a windowed engine, tier R, every R of the rule (8 / 4 / 2 / 1 heads per kv head; 7 through llama_dec_r = 2 at 128):
    planned windowed (out_kind 1), the context within the fp64 reference's tolerance over the last W keys, the cache afterwards holds
    the new key and value at pos and is otherwise untouched - nothing below the window is disturbed -, guard bands intact"""
    import _attn_ref_win as X
    base_dims, state, _, _ = toy
    M = _ref(base_dims)
    hd, P = base_dims.head_dim, 400
    pos = sorted({0, 1, W - 1, W, W + 1, 127, 128, 129, 255, 256, 383, 398} - {-1})
    pos = [t for t in pos if 0 <= t < P]
    eng = _engine(dataclasses.replace(base_dims, sliding_window=W), state, max_tokens=4096, max_seqs=16)
    for n, (H, n_kv, r_opt) in enumerate([(8, 1, 0), (4, 1, 0), (4, 2, 0), (3, 3, 0), (7, 1, 0), (7, 1, 2), (4, 2, 1)]):
        p = M.build_step(800 + 10 * n + bias, H, n_kv, pos, P, "R", bias=bias, band=8)
        what = f"windowed step W = {W} {H}/{n_kv} bias={bias} llama_dec_r={r_opt}"
        eng.set_option("llama_dec_r", r_opt)
        try:
            plan = eng.debug_attn(M.STEP, plan_only=True, **_sargs(p))
            assert plan["kind"] == 1, (what, plan)
            if r_opt == 2:
                assert plan["R"] == (7 if hd == 128 else 1), (what, plan)
            r = _guard(eng.debug_attn, M.STEP, **_sargs(p))
        finally:
            eng.set_option("llama_dec_r", 0)
        out, cache, cb = r["out"], r["cache"], p.band * hd
        assert _sentinel(out[:p.band]) and _sentinel(out[-p.band:]), f"{what}: a guard band of the output was written"
        assert _sentinel(cache[:cb]) and _sentinel(cache[-cb:]), f"{what}: a guard band of the cache was written"
        print(f"{what}: ratio {X.judge(M, p, W, out[p.band:-p.band], what):.2f}")
        M.judge_cache(p, cache[cb:-cb], what)
    eng.close()


def test_plain_engine_plans_are_unchanged(toy):
    base_dims, state, _, _ = toy
    M = _ref(base_dims)
    eng = _engine(dataclasses.replace(base_dims, sliding_window=0), state, max_tokens=4096, max_seqs=16)
    p = M.build_llama(760, 4, 2, [300, 5], "R", band=8)
    assert eng.debug_attn(M.LLAMA, plan_only=True, **_pargs(p))["kind"] == (1 if base_dims.head_dim == 128 else 2)
    s = M.build_step(761, 4, 2, [0, 200], 256, "R", band=8)
    assert eng.debug_attn(M.STEP, plan_only=True, **_sargs(s))["kind"] == 0
    eng.close()


# ---- refusals: nothing is launched, the sentinels are intact --------------------------------------------------------------------
def _raw_prefill_call(eng, p):
    """rk_debug_attn kind 4 with an output allocation the test keeps (filled with the sentinel) -> (status, that allocation)"""
    import ctypes as C
    from _attn_ref import SENTINEL
    from llmrankers._engine import RkDebugAttnCall
    c = RkDebugAttnCall()
    q, out, off = np.ascontiguousarray(p.q, np.float16), np.ascontiguousarray(p.out, np.float16), np.ascontiguousarray(p.seq_off, np.int32)
    out_all = np.full((out.shape[0] + 2 * p.band, p.ldctx), SENTINEL, np.uint8).repeat(2, axis=1)
    c.kind, c.n_seq, c.H, c.n_kv, c.ldq, c.ldctx, c.band_rows = 4, p.n_seq, p.H, p.n_kv, p.ldq, p.ldctx, p.band
    c.q, c.q_rows, c.seq_off = q.ctypes.data, q.shape[0] - 2 * p.band, off.ctypes.data
    c.out, c.out_rows, c.out_all = out.ctypes.data, out.shape[0], out_all.ctypes.data
    return eng.lib.rk_debug_attn(eng.h, C.byref(c)), out_all


def test_register_staged_prefill_kernel_refuses_a_call_longer_than_the_window():
    """llama_attn_dma = 0 selects attn_causal_tile_kernel<128>, which has no windowed form: RK_ERR_STATE naming the option and the window, the
    debug call's output all sentinel; a call that fits the window runs; the 64-wide engine has one kernel and ignores the option"""
    import _attn_ref as A
    dims = dataclasses.replace(_synth.TOY_MISTRAL, sliding_window=48)
    state = _synth.synth_state_dict(dims, seed=SEED)
    eng = _engine(dims, state, max_tokens=4096, max_seqs=16)
    eng.set_option("llama_attn_dma", 0)
    long, fits = A.build_llama(770, 4, 2, [10, 49], "R", band=8), A.build_llama(771, 4, 2, [10, 48], "R", band=8)
    with pytest.raises(RkError) as ei:
        eng.debug_attn(A.LLAMA, **_pargs(long))
    assert ei.value.code == ERR_STATE and "llama_attn_dma" in str(ei.value) and "48" in str(ei.value)
    rc, out_all = _raw_prefill_call(eng, long)                         # the same call with the caller's output allocation kept
    assert rc == ERR_STATE and _sentinel(out_all), "a refused call wrote its output"
    seqs = _synth.synth_token_batch(2, 49, 60, dims.vocab, seed=3)
    for call in (lambda: eng.last_logits(seqs, [1, 2]), lambda: eng.greedy1(seqs), lambda: eng.generate(seqs, 2, [], 0)):
        with pytest.raises(RkError) as ei:
            call()
        assert ei.value.code == ERR_STATE and "llama_attn_dma" in str(ei.value)
    plan = eng.debug_attn(A.LLAMA, plan_only=True, **_pargs(fits))
    assert plan["kind"] == 0
    _guard(eng.debug_attn, A.LLAMA, **_pargs(fits))
    short = [s[:40] for s in seqs]
    want = _guard(eng.last_logits, short, [1, 2])
    eng.set_option("llama_attn_dma", 1)
    assert _guard(eng.last_logits, seqs, [1, 2]).shape == (2, 2) and want.shape == (2, 2)
    eng.close()
    d64 = dataclasses.replace(_synth.TOY_MISTRAL_HD64, sliding_window=48)
    e64 = _engine(d64, _synth.synth_state_dict(d64, seed=SEED), max_tokens=4096, max_seqs=16)
    a = _guard(e64.last_logits, seqs, [1, 2])
    e64.set_option("llama_attn_dma", 0)
    assert np.array_equal(_bits(_guard(e64.last_logits, seqs, [1, 2])), _bits(a))
    e64.close()


def test_setter_refusals():
    """after finalize, on a T5 engine, a negative window: refused, and the engine goes on as it was"""
    from llmrankers._engine import RkEngine, RkLlamaEngine
    dims = dataclasses.replace(_synth.TOY_MISTRAL, sliding_window=0)
    state = _synth.synth_state_dict(dims, seed=SEED)
    eng = RkLlamaEngine(dims, device=0, max_tokens=1024, max_seqs=4)
    assert eng.lib.rk_llama_set_sliding_window(eng.h, -1) == ERR_INVALID
    assert eng.lib.rk_llama_set_sliding_window(eng.h, 0) == 0
    eng.load_state(state.items())
    assert eng.lib.rk_llama_set_sliding_window(eng.h, 8) == ERR_STATE
    seqs = _synth.synth_token_batch(2, 20, 30, dims.vocab, seed=5)
    a = _guard(eng.last_logits, seqs, [1, 2])
    eng.close()
    ref = _engine(dims, state, max_tokens=1024, max_seqs=4)       # the refused call left no window behind
    assert np.array_equal(_bits(_guard(ref.last_logits, seqs, [1, 2])), _bits(a))
    ref.close()
    t5 = RkEngine(_synth.TOY_GATED_UNTIED, device=0, max_tokens=512, max_seqs=4, max_dec_len=4)
    assert t5.lib.rk_llama_set_sliding_window(t5.h, 8) == ERR_STATE
    t5.close()


# ---- the reference's recorded R1 listwise cases (tools/make_r1_listwise_golden.py) on the engine -----------------------------------
def test_r1_listwise_reference_cases_on_the_engine(tmp_path):
    """R1ListwiseLlmRanker end to end on the toy Mistral checkpoint (its small window in the config, the LoRA adapter merged by the
    loader): prompt sha256s, new ids, completions, returned strings, final ranking, scores and counters of every recorded case - no
    step is excluded: every recorded margin clears the floor on the fp32 and on the fp16-rounded weights -, through the public
    constructor and through from_runtime; rerank_many == one by one"""
    import contextlib
    import io
    import json
    import os
    from conftest import GOLD
    from transformers import AutoTokenizer
    from llmrankers.listwise import R1ListwiseLlmRanker
    from llmrankers.rankers import SearchResult
    from _r1_listwise_gold import check_r1_case, run_r1_case
    with open(os.path.join(GOLD, "r1_listwise_cases.json")) as f:
        gold = json.load(f)
    ckpt, adir, tokdir = str(tmp_path / "ckpt"), str(tmp_path / "adapter"), os.path.join(GOLD, gold["tokenizer"])
    _synth.write_checkpoint(ckpt, gold["ckpt"], tokdir)
    assert _synth.checkpoint_sha256(ckpt) == gold["ckpt"]["sha256"]
    assert _synth.write_lora_adapter(adir, _synth.NAMED_DIMS[gold["ckpt"]["dims"]], gold["adapter"]) == gold["adapter"]["sha256"]
    first = gold["cases"][0]
    pub = R1ListwiseLlmRanker(ckpt, tokdir, gold["prompt"], first["window_size"], first["step_size"], lora_path=adir, num_repeat=first["num_repeat"],
                              max_new_tokens=first["max_new_tokens"])
    rt, tok = pub.llm, AutoTokenizer.from_pretrained(tokdir)
    assert rt.model_type == "mistral" and rt.dims.sliding_window == gold["sliding_window"] and rt.generation["eos_token_ids"] == [gold["model_eos"]]
    assert all(min(c["margin"]) > FLOOR for case in gold["cases"] for c in case["compares"])
    res, log = run_r1_case(pub, rt, first, _guard)
    check_r1_case(pub, res, log, first)
    make = lambda case: R1ListwiseLlmRanker.from_runtime(rt, tok, gold["prompt"], window_size=case["window_size"], step_size=case["step_size"],
                                                         num_repeat=case["num_repeat"], max_new_tokens=case["max_new_tokens"])
    for case in gold["cases"][1:]:
        rk = make(case)
        res, log = run_r1_case(rk, rt, case, _guard)
        check_r1_case(rk, res, log, case)
    rk = make(first)                                                           # two queries in lock step: ONE generate call per step
    items = [(first["query"], [SearchResult(docid=d, score=None, text=t) for d, t in first["docs"]]) for _ in range(2)]
    with contextlib.redirect_stdout(io.StringIO()):
        results, counters = rk.rerank_many(items)
    for r, n in zip(results, counters):
        assert [d.docid for d in r] == first["docids"] and list(n) == first["counters"]
    rt.engine.close()
