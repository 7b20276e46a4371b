"""The Qwen3 family on the HIP engine: the q / k head RMSNorm in the prefill's rotary kernel (rope128_qkn_kernel, rk_debug_rows op 11)
and in the cached decode step (attn_dec_cached_qkn_kernel, rk_debug_attn kind 5 with qk_norm) against fp64, the step's cached key
bit for bit the prefill's, the toy model against the fp32 oracle, session and graph replay, outlier norm weights against HF's own
fp16 error, Qwen3-4B widths, the contract, and RankR1SetwiseLlmRanker end to end on the recorded cases."""
import dataclasses
import json
import os
import random

import numpy as np
import pytest

import _attn_ref as A
import _qwen3_ref as Q
from conftest import GOLD
from llmrankers import _synth

pytestmark = pytest.mark.gpu
FLOOR = 5e-3              # fp16 noise floor of the toy scale (tests/test_gpu_rankr1.py)
BOUND = 4e-3              # x logit scale: what the Llama and Qwen2 prefill and step are held to (tests/test_gpu_rankr1.py)
BAND = 256
f16, i32 = np.float16, np.int32


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "qwen3_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def toy(gold):
    """toy-qwen3 at the recorded seed and gain: dims, state, oracle, head - computed once, never modified"""
    rec = gold["greedy"]
    dims = _synth.NAMED_DIMS[rec["dims"]]
    state = _synth.synth_state_dict(dims, seed=rec["seed"], gain=rec["gain"])
    return dims, state, Q.Qwen3Oracle(dims, state), np.asarray(state["model.embed_tokens.weight"], dtype=np.float32)


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 4096)
    kw.setdefault("max_seqs", 16)
    return RkLlamaEngine(dims, device=0, **kw).load_state(state.items())


@pytest.fixture(scope="module")
def eng(toy):
    """the toy engine the two debug entries run on (they take every shape from the call; the engine gives head_dim 128, no window)"""
    e = _engine(toy[0], toy[1], max_tokens=1024, max_seqs=8)
    yield e
    e.close()


def _all_logits(eng, seqs, vocab):
    return np.concatenate([eng.last_logits(seqs, list(range(v0, v0 + 64))) for v0 in range(0, vocab, 64)], axis=1)


# ---- the prefill kernel ----------------------------------------------------------------------------------------------------------------
def _rope_qkn(eng, p, qkv=None, pos=None):
    """op 11 on the problem (or on other rows of its shape) -> the rows afterwards; bands, plan and a second run are checked here"""
    qkv = p.qkv if qkv is None else qkv
    pos = p.pos if pos is None else np.asarray(pos, i32)
    T = qkv.shape[0]
    params = dict(rows=T, H=p.H, n_kv=p.n_kv, hd=128, ld=p.ld, max_pos=p.max_pos, eps=p.eps)
    ins = [pos, p.cos, p.sin, p.w]
    pl = eng.debug_rows(Q.OP_ROPE_QKN, ins=ins, outs=[qkv], band=BAND, plan_only=True, **params)
    assert (pl["grid"], pl["tparam"], pl["variant"]) == ((T, 1, 1), 128, 2), pl
    a = eng.debug_rows(Q.OP_ROPE_QKN, ins=ins, outs=[qkv], band=BAND, **params)["all"][0]
    b = eng.debug_rows(Q.OP_ROPE_QKN, ins=ins, outs=[qkv], band=BAND, **params)["all"][0]
    assert np.array_equal(a, b), "a second run gives other bytes"
    assert (a[:, :BAND] == A.SENTINEL).all() and (a[:, -BAND:] == A.SENTINEL).all(), "a band was written"
    return np.ascontiguousarray(a[0, BAND:-BAND]).view(f16).reshape(T, p.ld)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("H,n_kv", [(4, 2), (7, 1), (3, 3), (40, 8)])
def test_prefill_kernel_vs_fp64(eng, H, n_kv, T):
    """(3, 3): 48 items, a partly filled wave; (40, 8): 384 items, a second trip of the loop.  Positions restart at 0 and reach the
    table's last row; one head is all zero.  Value heads and pad columns byte for byte what they were."""
    p = Q.build_qkn(1100 + H + T, T, H, n_kv, zero_head=(T // 2, 1))
    assert int(p.pos[-1]) == p.max_pos - 1 and (T == 1 or int(p.pos[0]) == 0)
    out = _rope_qkn(eng, p)
    want, touched = Q.qkn_expected(p)
    assert np.array_equal(out[~touched].view(np.uint16), p.qkv[~touched].view(np.uint16)), "value heads or pad columns were touched"
    assert not touched[:, (H + n_kv) * 128:].any()
    assert not (out[T // 2, 128:256] != 0).any(), "the all-zero head: zeros (of either sign), not NaN"
    Q.qkn_judge(p, out, f"rope_qkn H={H} n_kv={n_kv} T={T}")


def test_debug_entries_refuse_what_the_kernels_do_not_take(eng):
    """op 11 without weights, at width 64 or with eps = 0; op 8 and op 3 as they were"""
    p = Q.build_qkn(7, 2, 4, 2)
    base = dict(rows=2, H=4, n_kv=2, hd=128, ld=p.ld, max_pos=p.max_pos, eps=p.eps)
    for ins, params in (([p.pos, p.cos, p.sin, None], base), ([p.pos, p.cos, p.sin, p.w], {**base, "hd": 64}),
                        ([p.pos, p.cos, p.sin, p.w], {**base, "eps": 0.0}), ([p.pos, p.cos, p.sin, p.w[:128]], base)):
        res = eng.debug_rows(Q.OP_ROPE_QKN, ins=ins, outs=[p.qkv], band=BAND, check=False, **params)
        assert res["rc"] == -1 and (res["all"][0] == A.SENTINEL).all(), params
    assert eng.debug_rows(12, ins=[p.pos], outs=[p.qkv], band=BAND, check=False, rows=2)["rc"] == -1
    pl = eng.debug_rows(8, ins=[p.pos, p.cos, p.sin, None], outs=[p.qkv], band=BAND, plan_only=True, **{k: v for k, v in base.items() if k != "eps"})
    assert (pl["tparam"], pl["variant"]) == (128, 0)
    x = np.zeros((1, 4100), np.float32)
    assert eng.debug_rows(3, ins=[x, np.ones(4100, np.float32), None], outs=[np.zeros(4100, f16)], band=BAND, check=False, rows=1, d=4100, src_rows=1, eps=1e-6,
                          out_scale=1.0)["rc"] == -1                                  # rmsnorm's d <= 4096 stays


# ---- the step kernel ---------------------------------------------------------------------------------------------------------------------
STEP_POS, STEP_P = [0, 1, 127, 128, 129, 300], 512


def _step(eng, p, **kw):
    return eng.debug_attn(A.STEP, n_seq=p.n_seq, H=p.H, q=p.q, out=p.out, band_rows=p.band, n_kv=p.n_kv, P=p.P, ldq=p.ldq, ldctx=p.ldctx, pos=p.pos,
                          cos=p.cos, sin=p.sin, cache=p.cache, qk_norm=p.qk_w, qk_eps=p.qk_eps, **kw)


def _prefill_cache(eng, p):
    """What the prefill writes for the step's rows: sequence b = pos[b] filler tokens and then the step's row, through the prefill
    kernel (op 11) and kv_cache_fill (op 9) into an empty cache of P positions -> K, V [n_seq][n_kv][P][128]"""
    rs = np.random.RandomState(3)
    lens = [int(t) + 1 for t in p.pos]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(i32)
    rows = rs.standard_normal((int(off[-1]), p.ldq)).astype(f16)
    pos = np.concatenate([np.arange(n) for n in lens]).astype(i32)
    for b in range(p.n_seq):
        rows[off[b + 1] - 1] = p.q[p.band + b]
    rp = Q.SimpleNamespace(H=p.H, n_kv=p.n_kv, ld=p.ldq, max_pos=p.P, eps=p.qk_eps, cos=p.cos, sin=p.sin, w=p.qk_w)
    rotated = _rope_qkn(eng, rp, qkv=rows, pos=pos)
    cache = A.sentinel16((2 * p.n_seq * p.n_kv * p.P * 128,))
    res = eng.debug_rows(9, ins=[rotated, off, None], outs=[cache], band=BAND, rows=p.n_seq, H=p.H, n_kv=p.n_kv, hd=128, ld=p.ldq, P=p.P)
    filled = np.ascontiguousarray(res["all"][0][0, BAND:-BAND]).view(f16)
    return A.step_cache_views(p, filled)


@pytest.mark.parametrize("H,n_kv", [(2, 2), (4, 2), (4, 1), (8, 1), (7, 1)])
def test_step_kernel_vs_fp64_and_its_cached_key_is_the_prefills(eng, H, n_kv):
    """G = 1, 2, 4, 8 by the plan's rule (R = G) and 7 with llama_dec_r 0 (R = 1) and 2 (R = 7): positions on both sides of the 128-key
    chunk edges in a cache of 512.  The context against fp64; the cache untouched but for the appended rows; the appended key and
    value bit for bit what the prefill kernel + kv_cache_fill write for the same row; R = 1 and R = 7 the same bytes."""
    G = H // n_kv
    p = Q.build_qkn_step(300 + H + n_kv, H, n_kv, STEP_POS, STEP_P)
    kpre, vpre = _prefill_cache(eng, p)
    runs = {}
    for opt in ((0, 2) if G == 7 else (0,)):
        eng.set_option("llama_dec_r", opt)
        try:
            plan = _step(eng, p, plan_only=True)
            want_R = 7 if (G == 7 and opt == 2) else (1 if G == 7 else G)
            assert (plan["kind"], plan["R"], plan["tparam"], plan["nch"]) == (2, want_R, want_R, STEP_P // 128), plan
            assert plan["grid"] == (STEP_P // 128, H // want_R, p.n_seq) and plan["grid2"] == (H, p.n_seq, 1)
            r1, r2 = _step(eng, p), _step(eng, p)
        finally:
            eng.set_option("llama_dec_r", 0)
        b, cb = p.band, p.band * 128
        assert r1["out"].tobytes() == r2["out"].tobytes() and r1["cache"].tobytes() == r2["cache"].tobytes(), "a second run gives other bytes"
        for a in (r1["out"][:b], r1["out"][-b:], r1["cache"][:cb], r1["cache"][-cb:]):
            assert (np.ascontiguousarray(a).view(np.uint8) == A.SENTINEL).all(), "a band was written"
        Q.qkn_step_judge(p, r1["out"][b:-b], f"qkn step H={H} n_kv={n_kv} llama_dec_r={opt}")
        kc, vc = A.step_cache_views(p, r1["cache"][cb:-cb])
        k0, v0 = A.step_cache_views(p, p.cache)
        for s in range(p.n_seq):
            t = int(p.pos[s])
            keep = np.arange(STEP_P) != t
            assert np.array_equal(kc[s][:, keep].view(np.uint16), k0[s][:, keep].view(np.uint16)), "the cache beside the appended key changed"
            assert np.array_equal(vc[s][:, keep].view(np.uint16), v0[s][:, keep].view(np.uint16)), "the cache beside the appended value changed"
            assert np.array_equal(kc[s, :, t].view(np.uint16), kpre[s, :, t].view(np.uint16)), f"row {s} at {t}: the step's key is not the prefill's"
            assert np.array_equal(vc[s, :, t].view(np.uint16), vpre[s, :, t].view(np.uint16)), f"row {s} at {t}: the step's value is not the prefill's"
        runs[opt] = (r1["out"].tobytes(), r1["cache"].tobytes())
    if G == 7:
        assert runs[0] == runs[2], "llama_dec_r 0 and 2 give other bytes"
    # null weights: the entry every earlier caller gets, untouched (kind 0)
    plain = eng.debug_attn(A.STEP, n_seq=p.n_seq, H=p.H, q=p.q, out=p.out, band_rows=p.band, n_kv=p.n_kv, P=p.P, ldq=p.ldq, ldctx=p.ldctx, pos=p.pos,
                           cos=p.cos, sin=p.sin, cache=p.cache)
    assert plain["kind"] == 0
    A.judge(p, plain["out"][p.band:-p.band], what="the plain step beside it")


# ---- the toy model against the oracle ---------------------------------------------------------------------------------------------------
def test_prefill_vs_oracle(toy):
    """6 ragged prompts (1, 2, 63, 64, 65, 300 tokens), every vocabulary row, against the fp32 oracle.  What the bound is worth:
    tests/test_qwen3_host.py::test_what_the_gpu_bound_is_worth (either norm left out: > 5 bounds away, on these prompts)."""
    dims, state, orc, _ = toy
    seqs = [_synth.synth_token_batch(1, n, n, dims.vocab, seed=40 + n)[0] for n in (1, 2, 63, 64, 65, 300)]
    eng = _engine(dims, state)
    got = _all_logits(eng, seqs, dims.vocab)
    eng.close()
    want = orc.last_logits(seqs)
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"max |logit - oracle| = {err:.3e} at scale {scale:.2f} (bound {BOUND * scale:.3e})")
    assert got.shape == want.shape == (6, dims.vocab)
    assert err < BOUND * scale, (err, scale)


def test_decode_step_at_chunk_boundaries(gold, toy):
    """prefixes of one 300-token sequence around the step kernel's 128-key chunks, max_new 1 .. 4, no EOS: the rows the last step's
    head read against the oracle; tokens == the oracle's (and HF's recorded ones) and == a greedy1 re-prefill loop wherever the
    oracle margin clears the floor (a step's cached key equals a prefill's); at least 20 tokens compared"""
    from _llama_gen_stub import oracle_greedy
    dims, state, orc, head = toy
    rec = gold["greedy"]
    base = _synth.synth_token_batch(1, 300, 300, dims.vocab, seed=rec["base_seed"])[0]
    assert rec["prefix_lens"] == [1, 2, 3, 126, 127, 128, 129, 255, 256, 257] and rec["max_new"] == 4
    seqs = [base[:n] for n in rec["prefix_lens"]]
    eng = _engine(dims, state)
    gen = None
    for max_new in range(1, 5):
        gen, steps = eng.generate(seqs, max_new, [], 0)
        assert steps == max_new and gen.shape == (len(seqs), max_new)
        last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), dims.hidden)
        want = orc.last_logits([list(s) + [int(t) for t in gen[b, :max_new - 1]] for b, s in enumerate(seqs)])
        scale, err = float(np.abs(want).max()), float(np.abs(last @ head.T - want).max())
        print(f"max_new {max_new}: max |logit - oracle| = {err:.3e} at scale {scale:.2f}")
        assert err < BOUND * scale, (max_new, err, scale)
    checked = 0
    for b, s in enumerate(seqs):
        toks, margins = oracle_greedy(orc, s, 4)
        low = next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
        assert list(gen[b, :low]) == toks[:low] == rec["tokens"][b][:low], (b, low)
        cur = list(s)
        for t in range(low):
            assert int(eng.greedy1([cur])[0]) == int(gen[b, t]), (b, t)
            cur.append(int(gen[b, t]))
        checked += low
    eng.close()
    assert checked >= 20, checked


def test_batch_independence(toy):
    """a row alone, in a batch of 7 and in the reversed batch: equal tokens where the oracle margins clear the floor, bit-equal final
    rows between the batch and the reversed batch"""
    from _llama_gen_stub import oracle_greedy
    dims, state, orc, _ = toy
    rs = np.random.RandomState(23)
    seqs = [rs.randint(3, dims.vocab - 28, size=n).astype(np.int32) for n in (3, 300, 129, 47, 256, 64, 190)]
    eng = _engine(dims, state)
    batch, _ = eng.generate(seqs, 6, [], 0)
    last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), -1).copy()
    rev, _ = eng.generate(seqs[::-1], 6, [], 0)
    last_rev = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), -1)
    np.testing.assert_array_equal(rev[::-1], batch)
    assert np.array_equal(last_rev[::-1].view(np.uint32), last.view(np.uint32))
    for b, s in enumerate(seqs):
        alone, _ = eng.generate([s], 6, [], 0)
        toks, margins = oracle_greedy(orc, s, 6)
        low = next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
        assert list(alone[0, :low]) == list(batch[b, :low]) == toks[:low], (b, low)
    eng.close()


# ---- session and graph ---------------------------------------------------------------------------------------------------------------------
def test_session_with_staggered_admits_and_the_eager_step(toy):
    """ten prompts through a session of 4 slots, free slots refilled while the others decode: every prompt's tokens are the tokens
    rk_llama_generate gives it alone; and generate on an engine created for dec_graph = 0 (eager launches) gives the default
    engine's tokens and final rows bit for bit"""
    dims, state, _, _ = toy
    lens = (1, 2, 63, 64, 65, 127, 128, 129, 255, 300)
    max_new = tuple((40, 5, 2, 1)[i % 4] for i in range(len(lens)))
    base = _synth.synth_token_batch(1, 300, 300, dims.vocab, seed=17)[0]
    prompts = [list(base[:n]) for n in lens]
    eng = _engine(dims, state)
    want = []
    for p, m in zip(prompts, max_new):
        toks, steps = eng.generate([p], m, [], 0)
        want.append([int(t) for t in toks[0, :steps]])
    got, refills, nxt = {}, 0, 0
    with eng.session(4, 384, 40, [], 0) as s:
        owner = {}
        while nxt < len(prompts) or s.busy:
            free = s.free_slots()
            take = list(range(nxt, min(nxt + len(free), len(prompts))))
            if take:
                refills += bool(s.busy)
                slots = free[:len(take)]
                s.admit([prompts[r] for r in take], slots, [max_new[r] for r in take])
                owner.update(zip(slots, take))
                nxt += len(take)
            finished, _ = s.run()
            assert finished, "a run with busy slots must end with a finish"
            for slot in finished:
                got[owner.pop(slot)] = [int(t) for t in s.read(slot)]
    assert refills >= 2, refills
    for r, w in enumerate(want):
        assert got[r] == w, (r, lens[r], got[r], w)
    batch = prompts[2:9]
    gen, steps = eng.generate(batch, 6, [], 0)
    rows = eng.debug_read("llama_last", len(batch) * dims.hidden).copy()
    eng.close()
    eager = _engine(dims, state)
    eager.set_option("dec_graph", 0)
    gen0, steps0 = eager.generate(batch, 6, [], 0)
    rows0 = eager.debug_read("llama_last", len(batch) * dims.hidden)
    eager.close()
    assert steps0 == steps
    np.testing.assert_array_equal(gen0, gen)
    assert np.array_equal(rows0.view(np.uint32), rows.view(np.uint32))


# ---- outlier norm weights -------------------------------------------------------------------------------------------------------------
def test_outlier_norm_weights_vs_hf_fp16_error(gold, toy):
    """4 channels of every q_norm and k_norm weight x 20: the engine's max logit error against fp32 on 4 prompts of 40 - 120 tokens
    must not exceed HF's own fp16 error there (Qwen3ForCausalLM.half() on the CPU against fp32, tools/make_qwen3_golden.py)"""
    dims, state, _, _ = toy
    rec = gold["outlier"]
    assert (rec["dims"], rec["seed"], rec["gain"]) == (gold["greedy"]["dims"], gold["greedy"]["seed"], gold["greedy"]["gain"])
    out = Q.with_norm_outliers(state)
    seqs = _synth.synth_token_batch(4, 40, 120, dims.vocab, seed=rec["prompt_seed"])
    assert [len(s) for s in seqs] == rec["prompt_lens"]
    eng = _engine(dims, out)
    got = _all_logits(eng, seqs, dims.vocab)
    eng.close()
    want = Q.Qwen3Oracle(dims, out).last_logits(seqs)
    errs = np.abs(got - want).max(axis=1)
    print(f"engine max |logit - fp32| per prompt {[f'{e:.4f}' for e in errs]}; HF fp16: {[f'{e:.4f}' for e in rec['hf_fp16_err_per_prompt']]} "
          f"(scale {float(np.abs(want).max()):.2f})")
    assert float(errs.max()) <= rec["hf_fp16_max_err"], (float(errs.max()), rec["hf_fp16_max_err"])


# ---- real widths ---------------------------------------------------------------------------------------------------------------------------
def test_qwen3_4b_widths_vs_oracle():
    """Qwen3-4B widths (32 query heads on 8 kv heads of 128: q width 4096 against hidden 2560, tied head) with two layers and a
    vocabulary of 4096: one 600-token and one 45-token prompt, every vocabulary row within the bound"""
    dims = dataclasses.replace(_synth.QWEN3_4B, n_layers=2, vocab=4096)
    assert dims.qk_norm and dims.tied_head and dims.n_heads * dims.head_dim == 4096 != dims.hidden
    state = _synth.synth_state_dict(dims, seed=929, threads=16)
    seqs = [s for n in (600, 45) for s in _synth.synth_token_batch(1, n, n, dims.vocab, seed=700 + n)]
    eng = _engine(dims, state, max_tokens=2048, max_seqs=4)
    got = _all_logits(eng, seqs, dims.vocab)
    eng.close()
    want = Q.Qwen3Oracle(dims, state).last_logits(seqs)
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"max |logit - oracle| = {err:.3e} at scale {scale:.2f} (bound {BOUND * scale:.3e})")
    assert err < BOUND * scale, (err, scale)


# ---- the contract ------------------------------------------------------------------------------------------------------------------------
def test_contract(toy, ckpt_dirs):
    """rk_llama_set_qk_norm on a T5 engine and after finalize: RK_ERR_STATE; finalize with the switch on and a norm weight missing:
    RK_ERR_MISSING naming it; with 64-wide heads, a window or q / k / v biases beside it: RK_ERR_STATE with a message; the switch off:
    the norm weights are ignored and the engine computes the plain Llama model"""
    from conftest import load_state
    from llmrankers._engine import RkEngine, RkError, RkLlamaEngine
    from oracle.llama_numpy import LlamaOracle
    dims, state, _, _ = toy
    t5dims, t5state = load_state(ckpt_dirs["ckpt_gated_untied"])
    t5 = RkEngine(t5dims, device=0, max_tokens=512, max_seqs=4, max_dec_len=4)
    assert t5.lib.rk_llama_set_qk_norm(t5.h, 1) == -4
    t5.close()
    eng = _engine(dims, state, max_tokens=512, max_seqs=4)
    assert eng.lib.rk_llama_set_qk_norm(eng.h, 0) == -4
    assert b"finalize" in eng.lib.rk_last_error(eng.h)
    eng.close()
    missing = "model.layers.1.self_attn.k_norm.weight"
    eng = RkLlamaEngine(dims, device=0, max_tokens=512, max_seqs=4)
    with pytest.raises(RkError) as ex:
        eng.load_state((k, v) for k, v in state.items() if k != missing)
    assert ex.value.code == -5 and missing in str(ex.value)
    eng.close()
    for bad in (dataclasses.replace(_synth.TOY_LLAMA_HD64, qk_norm=True), dataclasses.replace(dims, sliding_window=64, mistral=True),
                dataclasses.replace(dims, qkv_bias=True)):
        eng = RkLlamaEngine(bad, device=0, max_tokens=512, max_seqs=4)
        with pytest.raises(RkError) as ex:
            eng.load_state(_synth.synth_state_dict(bad, seed=3).items())
        assert ex.value.code == -4 and "head norm" in str(ex.value) and "head_dim 128" in str(ex.value), str(ex.value)
        eng.close()
    eng = _engine(dataclasses.replace(dims, qk_norm=False), state, max_tokens=512, max_seqs=4)
    seqs = [[5, 9, 200, 31, 77]]
    got = eng.last_logits(seqs, list(range(64)))
    eng.close()
    want = LlamaOracle(dims, state).last_logits(seqs)[:, :64]
    assert float(np.abs(got - want).max()) < BOUND * float(np.abs(want).max())


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_rankr1_recorded_cases_on_the_engine(gold, tmp_path):
    """the recorded cases (HF's fp32 greedy tokens under RankR1SetwiseLlmRanker, every step's margin above the floor) through the
    ranker on the real engine, the checkpoint written from its recipe (sha256 asserted): every compare's label, rankings, counters;
    then the reference's constructor, by path"""
    from transformers import AutoTokenizer
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    assert gold["min_margin"] > FLOOR
    path = str(tmp_path / "toy-qwen3")
    tokdir, prompt = os.path.join(GOLD, gold["tokenizer"]), os.path.join(GOLD, gold["prompt_file"])
    _synth.write_checkpoint(path, gold["ckpt"], tokdir)
    assert _synth.checkpoint_sha256(path) == gold["ckpt"]["sha256"]
    with pytest.raises(NotImplementedError):
        LlamaRuntime(path, "cuda")                                  # the default still serves Llama only
    rt = LlamaRuntime(path, "cuda", max_tokens=4096, max_seqs=16, accept_model_types=("qwen3",))
    assert rt.model_type == "qwen3" and rt.dims.qk_norm and rt.generation["eos_token_ids"] == [gold["model_eos"]]
    tok = AutoTokenizer.from_pretrained(tokdir)                     # (its own directory: see tests/test_rankr1_host.py)
    for case in gold["cases"]:
        rk = RankR1SetwiseLlmRanker.from_runtime(rt, tok, prompt, num_child=case["num_child"], k=case["k"], method=case["method"],
                                                 num_permutation=case["num_permutation"], max_new_tokens=case["max_new_tokens"])
        outs, real = [], rk.compare
        rk.compare = lambda q, docs: outs.append(real(q, docs)) or outs[-1]
        random.seed(case["random_seed"])
        res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
        tag = case["qid"]
        assert outs == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
    rt.engine.close()
    case = gold["cases"][0]
    rk = RankR1SetwiseLlmRanker(path, prompt, tokenizer_name_or_path=tokdir, num_child=case["num_child"], k=case["k"], method=case["method"],
                                num_permutation=case["num_permutation"], max_new_tokens=case["max_new_tokens"])
    assert rk.llm.model_type == "qwen3" and rk.llm.dims.qk_norm
    random.seed(case["random_seed"])
    res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
    assert [d.docid for d in res] == case["docids"]
    assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"]
    rk.llm.engine.close()
