"""FP8 K / V cache of the Llama decoding step (rk_llama_set_kv_fp8; DESIGN.md section 3 "FP8 K/V cache").

Like FP8 step weights the design needs no tolerance of its own: a dequantised cache element is an fp16 number, so the byte kernels
are, bit for bit, the fp16 kernels on the dequantised cache.  Held here:
  1. the quantiser every cache writer calls equals tests/_kv8_ref.py byte for byte on adversarial vectors;
  2. the step's attention on host data (rk_debug_kv8_step): the byte form equals the rounded-fp16 form bit for bit in context and
     partials, the cache it leaves is numpy's quantisation of what the fp16 kind-5 entry writes, both lie within _attn_ref's kind-5
     rule of fp64 on the dequantised operands, the KEYS form equals the unchanged fp16 KEYS kernel, guard bands intact;
  3. the fill (prefill and session admit) against numpy's quantisation of an fp16 engine's cache;
  4. the model three ways on every toy family: byte form = rounded-fp16 form in tokens and last rows - generate, a session with
     refill, a drafting session, graph replay - and the prefill-only entries equal an fp16 engine's;
  5. the last step's logits against the independent reference (Kv8Oracle) within 4e-3 x logit scale + D_ref;
  6. the contract; 7. the size."""
import numpy as np
import pytest

import _attn_ref as A
import _kv8_ref as K
from llmrankers import _synth
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_HIP, ERR_STATE = -1, -3, -4
PAD = 0
BAND = 256                # bytes of every guard band of rk_debug_kv8_step's outputs
f16, f32, f64 = np.float16, np.float32, np.float64


def _guard(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{getattr(fn, '__name__', fn)}: {err}", returncode=3)
        raise


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 2048)
    kw.setdefault("max_seqs", 16)
    return _guard(RkLlamaEngine(dims, device=0, **kw).load_state, state.items())


def _state(name):
    dims = K.families()[name][0]
    return dims, _synth.synth_state_dict(dims, seed=K.SYNTH_SEED)


def _last(eng, n, hidden):
    return _guard(eng.debug_read, "llama_last", n * hidden).reshape(n, hidden).copy()


def _lkv_bytes(eng):
    cap = eng.buffers()["lkv"]["cap"]            # halfs
    return _guard(eng.debug_read, "lkv", cap // 2).view(np.uint8).copy()


@pytest.fixture(scope="module")
def eng8():
    """a toy Llama engine with an FP8 cache: the two debug entries take every shape from the call"""
    dims, state = _state("toy-llama")
    e = _engine(dims, state, max_tokens=1024, max_seqs=8, kv_fp8=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng8_win():
    """the same with a sliding window of 100: the step entries take the window from the engine"""
    import dataclasses
    dims, state = _state("toy-mistral")
    e = _engine(dataclasses.replace(dims, sliding_window=100), state, max_tokens=1024, max_seqs=8, kv_fp8=True)
    yield e
    e.close()


# ---- 1. the quantiser ------------------------------------------------------------------------------------------------------------------
def test_quantiser_equals_the_reference_byte_for_byte(eng8):
    x = K.adversarial_vectors()
    q_ref, e_ref, d_ref = K.quantize_vectors(x)
    assert e_ref.min() == -15 and e_ref.max() == 7
    q, e, d = _guard(eng8.debug_kv8_quant, x)
    np.testing.assert_array_equal(e, e_ref, err_msg="exponents")
    bad = np.argwhere(q != q_ref)
    assert bad.size == 0, f"{len(bad)} bytes differ, first at {bad[0]}: engine {q[tuple(bad[0])]:#x} reference {q_ref[tuple(bad[0])]:#x} for x = {float(x[tuple(bad[0])])!r}"
    np.testing.assert_array_equal(d.view(np.uint16), d_ref.view(np.uint16), err_msg="dequantised fp16")
    q3, e3, d3 = _guard(eng8.debug_kv8_quant, d)                  # a fixed point in value
    assert d3.tobytes() == d.tobytes()
    q1, e1, d1 = _guard(eng8.debug_kv8_quant, x[17:18])           # one vector alone: a workgroup with 16 live threads
    assert q1.tobytes() == q[17:18].tobytes() and e1[0] == e[17] and d1.tobytes() == d[17:18].tobytes()


# ---- 2. the step's attention on host data -------------------------------------------------------------------------------------------------
STEP_POS = [0, 1, 31, 32, 127, 128, 129, 255, 256, 300]          # both sides of every wave (32 keys) and chunk (128 keys) edge
P_STEP = 304
HEADS = [(4, 4), (4, 2), (8, 2), (8, 1), (7, 1)]                  # G = 1, 2, 4, 8, 7


def _split(buf, band, dtype):
    """a read-back allocation [band | interior | band] -> the interior as dtype; the bands must hold the sentinel"""
    buf = np.asarray(buf, dtype=np.uint8)
    assert (buf[:band] == A.SENTINEL).all() and (buf[-band:] == A.SENTINEL).all(), "a guard band was written"
    return buf[band:-band].view(dtype)


def _fp16_step(eng, p, qk=None, g1=0, live=None):
    """the unchanged fp16 kind-5 entry on the problem -> (context [n_seq, H 128], the cache it leaves: K plane, V plane)"""
    kw = dict(n_seq=p.n_seq, H=p.H, q=p.q, out=p.out, band_rows=p.band, n_kv=p.n_kv, P=p.P, ldq=p.ldq, ldctx=p.ldctx, pos=p.pos,
              cos=p.cos, sin=p.sin, qkv_bias=p.qkv_bias, cache=p.cache, g1=g1, live=live)
    if qk is not None:
        kw.update(qk_norm=p.qk_w, qk_eps=p.qk_eps)
    r = _guard(eng.debug_attn, A.STEP, **kw)
    cache = r["cache"][p.band * 128:-p.band * 128]
    rows = p.n_seq // max(g1, 1)
    half = rows * p.n_kv * p.P * 128
    return r["out"][p.band:-p.band], cache[:half].reshape(rows, p.n_kv, p.P, 128), cache[half:].reshape(rows, p.n_kv, p.P, 128)


def _kv8_step(eng, p, mode, qk=None, g1=0, live=None, cache=None):
    kw = dict(mode=mode, qkv=p.q[p.band:p.band + p.n_seq], pos=p.pos, cos=p.cos, sin=p.sin, cache=p.cache if cache is None else cache,
              H=p.H, n_kv=p.n_kv, P=p.P, qkv_bias=p.qkv_bias, g1=g1, live=live, band=BAND, fill=float(f16(-3.0)))
    if qk is not None:
        kw.update(qk_norm=p.qk_w, qk_eps=p.qk_eps)
    r = _guard(eng.debug_kv8_step, **kw)
    return (_split(r["ctx"], BAND, f16).reshape(p.n_seq, p.H * 128), _split(r["part"], BAND, f32), _split(r["cache"], BAND, np.uint8), r)


def _check_step(eng, p, what, window=0, qk=None):
    rows = p.n_seq
    ctx16, k16, v16 = _fp16_step(eng, p, qk)
    c0, part0, cache0, r0 = _kv8_step(eng, p, 0, qk)
    c1, part1, cache1, _ = _kv8_step(eng, p, 1, qk)
    G = p.H // p.n_kv
    assert r0["R"] == (8 if G % 8 == 0 else 4 if G % 4 == 0 else 2 if G % 2 == 0 else 1) and r0["pe"] == K.pad32(p.P), (what, r0["R"], r0["pe"])
    # the byte form and the rounded-fp16 form: the same bits in context and partials
    assert c0.tobytes() == c1.tobytes(), f"{what}: context, bytes vs rounded fp16"
    assert part0.tobytes() == part1.tobytes(), f"{what}: partials, bytes vs rounded fp16"
    # the cache after the step: numpy's quantisation of what the fp16 entry writes for the same operands
    Kq, Vq = K.quantize_cache(k16, v16)
    kq, vq, ke, ve = K.layout_views(cache0, rows, p.n_kv, p.P)
    for got, want, name in ((kq, Kq[0], "K bytes"), (vq, Vq[0], "V bytes"), (ke, Kq[1], "K exponents"), (ve, Vq[1], "V exponents")):
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: {name} of the cache: {len(bad)} differ, first at {bad[0]}"
    want1 = np.concatenate([Kq[2].reshape(-1), Vq[2].reshape(-1)])
    assert cache1.view(np.uint16).tobytes() == want1.view(np.uint16).tobytes(), f"{what}: the rounded-fp16 cache is not the dequantised cache"
    # both within _attn_ref's kind-5 rule of fp64 on the dequantised operands (the own key as the fp16 entry forms it, rounded)
    new16 = (np.stack([k16[b, :, int(p.pos[b])] for b in range(rows)]), np.stack([v16[b, :, int(p.pos[b])] for b in range(rows)]))
    ref, em, _ = K.step_reference(p, new16, window=window, qk=qk is not None)
    worst = K.step_judge(ref, em, c0, what)
    merged = K.merge_partials(part0, rows, p.H, r0["nch"], p.pos, window)           # the partials say the same as the context they merge into
    assert np.abs(merged - c0.astype(f64)).max() <= 2 * A.half_ulp16(merged).max() + 1e-6, f"{what}: partials vs context"
    return worst


ROWS3 = [[0, 129, 300], [1, 32, 256], [31, 127, 255], [128, 99, 100]]      # three rows with different positions: every position again
FORMS = ["plain", "bias", "window", "window+bias", "qknorm"]
WINDOWED = ("window", "window+bias")


def _problem(form, seed, H, n_kv, pos):
    import _qwen3_ref as Q3
    if form == "qknorm":
        return Q3.build_qkn_step(seed, H, n_kv, pos, P_STEP)
    return A.build_step(seed, H, n_kv, pos, P_STEP, "R", bias=form in ("bias", "window+bias"))


@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"H{h[0]}kv{h[1]}")
@pytest.mark.parametrize("form", FORMS)
def test_step_attention_bytes_equal_rounded_fp16_and_fp64(eng8, eng8_win, form, heads):
    """every kernel (form x R x mode is an instantiation of its own) at every position of STEP_POS as a one-row call, and in four
    three-row calls with different positions; the window forms (W = 100, without and with the bias) so see positions on both sides of W,
    99 and 100 included"""
    eng, window = (eng8_win, 100) if form in WINDOWED else (eng8, 0)
    H, n_kv = heads
    worst = 0.0
    for n, pos in enumerate([[t] for t in STEP_POS] + ROWS3):
        p = _problem(form, 900 + 31 * H + n_kv + n, H, n_kv, pos)
        # exponents that differ between kv heads, K and V, and positions: what a wrong exponent plane would show
        c = p.cache.reshape(2, len(pos), n_kv, P_STEP, 128).astype(f32)
        c *= (2.0 ** np.random.RandomState(n).randint(-3, 3, size=(2, len(pos), n_kv, P_STEP, 1))).astype(f32)
        p.cache = c.astype(f16).reshape(-1)
        worst = max(worst, _check_step(eng, p, f"{form} H={H} n_kv={n_kv} pos={pos}", window, p if form == "qknorm" else None))
    print(f"{form} H={H} n_kv={n_kv}: worst (error - half ulp) / E = {worst:.3f} (C {A.C})")


@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"H{h[0]}kv{h[1]}")
@pytest.mark.parametrize("form", FORMS)
def test_keys_form_equals_the_fp16_keys_kernel(eng8, eng8_win, form, heads):
    """g1 = 3: three step rows per cache row at pos, pos + 1, pos + 2, for every pos of STEP_POS (one cache row) and in three calls
    with two cache rows.  With every row dead (live = 0) nothing is appended: the FP8 KEYS kernel over the quantised cache against
    the unchanged fp16 KEYS kernel over the dequantised cache, bit for bit.  With every row live: the rounding append leaves numpy's
    quantisation of what the fp16 append writes, and the two forms agree."""
    eng = eng8_win if form in WINDOWED else eng8
    H, n_kv = heads
    for n, base in enumerate([[t] for t in STEP_POS] + [[0, 129], [31, 255], [127, 300]]):
        pos = [min(b + j, P_STEP - 1) for b in base for j in range(3)]
        what = f"keys {form} H={H} n_kv={n_kv} pos={pos}"
        p = _problem(form, 950 + 31 * H + n_kv + n, H, n_kv, pos)
        qk = p if form == "qknorm" else None
        rows = len(base)
        kc, vc = A.step_cache_views(p, p.cache)
        kd, vd = K.quantize_vectors(kc[:rows])[2], K.quantize_vectors(vc[:rows])[2]
        p.cache = np.concatenate([kd.reshape(-1), vd.reshape(-1)])           # a dequantised cache of `rows` cache rows
        dead, live = np.zeros(len(pos), np.int32), np.ones(len(pos), np.int32)
        ctx16, k16, v16 = _fp16_step(eng, p, qk, g1=3, live=dead)
        assert k16.tobytes() == kd.tobytes() and v16.tobytes() == vd.tobytes(), f"{what}: dead rows wrote the fp16 cache"
        c0, part0, cache0, _ = _kv8_step(eng, p, 0, qk, g1=3, live=dead)
        assert c0.tobytes() == np.ascontiguousarray(ctx16).tobytes(), f"{what}: FP8 KEYS kernel vs the fp16 KEYS kernel on the dequantised cache"
        kq, vq, ke, ve = K.layout_views(cache0, rows, n_kv, P_STEP)
        Kq, Vq = K.quantize_cache(kd, vd)
        assert (kq == Kq[0]).all() and (vq == Vq[0]).all() and (ke == Kq[1]).all() and (ve == Vq[1]).all(), f"{what}: dead rows wrote the FP8 cache"
        # live rows: the append
        _, k16, v16 = _fp16_step(eng, p, qk, g1=3, live=live)
        c0, part0, cache0, _ = _kv8_step(eng, p, 0, qk, g1=3, live=live)
        c1, part1, cache1, _ = _kv8_step(eng, p, 1, qk, g1=3, live=live)
        assert c0.tobytes() == c1.tobytes() and part0.tobytes() == part1.tobytes(), f"{what}: bytes vs rounded fp16"
        Kq, Vq = K.quantize_cache(k16, v16)
        kq, vq, ke, ve = K.layout_views(cache0, rows, n_kv, P_STEP)
        assert (kq == Kq[0]).all() and (vq == Vq[0]).all() and (ke == Kq[1]).all() and (ve == Vq[1]).all(), f"{what}: the append's bytes"
        want1 = np.concatenate([Kq[2].reshape(-1), Vq[2].reshape(-1)])
        assert cache1.view(np.uint16).tobytes() == want1.view(np.uint16).tobytes(), f"{what}: the rounding append's fp16 cache"


# ---- 3. the fill -------------------------------------------------------------------------------------------------------------------------
FILL_LENS = [1, 5, 127, 128, 129, 300]


def _prompts(dims, lens, seed=60):
    return [[int(t) for t in _synth.synth_token_batch(1, n, n, dims.vocab, seed=seed + n)[0]] for n in lens]


def _fp16_planes(raw, n_layers, rows, n_kv, P):
    c = raw.view(f16)[:n_layers * 2 * rows * n_kv * P * 128].reshape(n_layers, 2, rows, n_kv, P, 128)
    return c[:, 0], c[:, 1]


def _written(plane, lens):
    """a copy of one layer's fp16 plane [rows, n_kv, P, 128] with everything no prompt wrote set to 0 (never-written device memory
    holds anything, NaN patterns included: nothing the reference's quantiser should see); lens: {cache row: prompt length}"""
    out = np.zeros_like(plane)
    for b, n in lens.items():
        out[b, :, :n] = plane[b, :, :n]
    return out


def _kv8_planes(raw, n_layers, rows, n_kv, P):
    lb = K.layer_bytes(rows, n_kv, P)
    return [K.layout_views(raw[l * lb:(l + 1) * lb], rows, n_kv, P) for l in range(n_layers)]


@pytest.mark.parametrize("name", ["toy-llama", "toy-qwen2", "toy-qwen3"])
def test_fill_equals_numpys_quantisation_of_the_fp16_cache(name):
    dims, state = _state(name)
    seqs = _prompts(dims, FILL_LENS)
    P, rows, n_kv, L = max(FILL_LENS) + 1, len(seqs), dims.n_kv_heads, dims.n_layers
    e16, e8 = _engine(dims, state), _engine(dims, state, kv_fp8=True)
    t16, _ = _guard(e16.generate, seqs, 1, [], PAD)
    t8, _ = _guard(e8.generate, seqs, 1, [], PAD)
    np.testing.assert_array_equal(t8, t16)                           # column 0 is the prefill's: un-quantised
    k16, v16 = _fp16_planes(_lkv_bytes(e16), L, rows, n_kv, P)
    got = _kv8_planes(_lkv_bytes(e8), L, rows, n_kv, P)
    e8.set_option("llama_kv_fp8", 0)
    _guard(e8.generate, seqs, 1, [], PAD)
    kr, vr = _fp16_planes(_lkv_bytes(e8), L, rows, n_kv, P)
    lens = dict(enumerate(FILL_LENS))
    for l in range(L):
        Kq, Vq = K.quantize_cache(_written(k16[l], lens), _written(v16[l], lens))
        kq, vq, ke, ve = got[l]
        for b, n in enumerate(FILL_LENS):                            # the prompt's positions (what lies behind them was never written)
            what = f"{name} layer {l} prompt of {n}"
            assert (kq[b, :, :n] == Kq[0][b, :, :n]).all() and (vq[b, :, :n] == Vq[0][b, :, :n]).all(), f"{what}: bytes"
            assert (ke[b, :, :n] == Kq[1][b, :, :n]).all() and (ve[b, :, :n] == Vq[1][b, :, :n]).all(), f"{what}: exponents"
            assert kr[l][b, :, :n].tobytes() == Kq[2][b, :, :n].tobytes() and vr[l][b, :, :n].tobytes() == Vq[2][b, :, :n].tobytes(), f"{what}: rounded fp16"
    e16.close(); e8.close()


def test_session_admit_fills_its_slots_and_no_others():
    """every length of FILL_LENS through an admit into slots {2, 0} of 4 (three sessions of two prompts each), in the byte form and
    in the rounded-fp16 form: the admitted positions hold numpy's quantisation (its dequantised values) of what an fp16 engine's
    admit writes; every other byte of the cache is what it was before the admit"""
    dims, state = _state("toy-llama")
    slots, n_slots, P, n_kv, L = [2, 0], 4, 304, dims.n_kv_heads, dims.n_layers
    e16, e8 = _engine(dims, state), _engine(dims, state, kv_fp8=True)

    def admit(e, seqs):
        with e.session(n_slots, P, 2, [], PAD) as s:
            before = _lkv_bytes(e)
            _guard(s.admit, seqs, slots, [1, 1])
            return before, _lkv_bytes(e)

    for pair in ((1, 5), (127, 128), (129, 300)):
        seqs = _prompts(dims, list(pair))
        lens = dict(zip(slots, pair))
        k16, v16 = _fp16_planes(admit(e16, seqs)[1], L, n_slots, n_kv, P)
        for mode in (1, 0):
            e8.set_option("llama_kv_fp8", mode)
            before, after = admit(e8, seqs)
            if mode:
                got, was = _kv8_planes(after, L, n_slots, n_kv, P), _kv8_planes(before, L, n_slots, n_kv, P)
            else:                                                     # fp16 planes, compared as bit patterns
                got = [tuple(x[l].view(np.uint16) for x in _fp16_planes(after, L, n_slots, n_kv, P)) for l in range(L)]
                was = [tuple(x[l].view(np.uint16) for x in _fp16_planes(before, L, n_slots, n_kv, P)) for l in range(L)]
            for l in range(L):
                Kq, Vq = K.quantize_cache(_written(k16[l], lens), _written(v16[l], lens))
                want = (Kq[0], Vq[0], Kq[1], Vq[1]) if mode else (Kq[2].view(np.uint16), Vq[2].view(np.uint16))
                what = f"prompts {pair} llama_kv_fp8 {mode} layer {l}"
                for slot, n in lens.items():
                    for g, w in zip(got[l], want):
                        assert (g[slot, :, :n] == w[slot, :, :n]).all(), f"{what} slot {slot}"
                    for g, o in zip(got[l], was[l]):                  # behind the prompt: as it was
                        assert (g[slot, :, n:] == o[slot, :, n:]).all(), f"{what} slot {slot}: positions behind the prompt changed"
                for slot in (1, 3):
                    for g, o in zip(got[l], was[l]):
                        assert (g[slot] == o[slot]).all(), f"{what}: slot {slot} is not the admit's to write"
    e16.close(); e8.close()


# ---- 4. the model three ways ------------------------------------------------------------------------------------------------------------
NEW = 6


def _session(eng, prompts, max_new, n_slots, draft=0):
    """the requests in order through a session of n_slots (free slots refilled whenever there are any) -> {request: tokens}, refills"""
    got, nxt, refills = {}, 0, 0
    with eng.session(n_slots, 256, 32, [], PAD, draft=draft) as s:
        owner = {}
        while nxt < len(prompts) or s.busy:
            free = s.free_slots()
            take = list(range(nxt, min(nxt + len(free), len(prompts))))
            if take:
                refills += bool(s.busy)
                sl = free[:len(take)]
                _guard(s.admit, [prompts[r] for r in take], sl, [max_new[r] for r in take])
                owner.update(zip(sl, take))
                nxt += len(take)
            finished, _ = _guard(s.run)
            assert finished
            for slot in finished:
                got[owner.pop(slot)] = [int(t) for t in _guard(s.read, slot)]
    return got, refills


@pytest.mark.parametrize("name", ["toy-llama", "toy-qwen2", "toy-qwen3", "toy-mistral"])
def test_model_bytes_equal_rounded_fp16(name):
    dims, state = _state(name)
    five = _prompts(dims, [120, 123, 126, 128, 130], seed=300)        # 6 new tokens: the rows cross the 128-key chunk edge
    ses = _prompts(dims, [4, 33, 70, 129, 9, 64, 17], seed=200)
    ses_new = [5, 12, 18, 8, 9, 4, 6]
    ids = list(range(0, dims.vocab, 7))[:64]
    e8 = _engine(dims, state, kv_fp8=True)
    out = {}
    for kv in (1, 0):
        for graph in (1, 0):
            e8.set_option("llama_kv_fp8", kv)
            e8.set_option("dec_graph", graph)
            r = {}
            for tag, seqs in (("one", five[3:4]), ("five", five)):
                toks, steps = _guard(e8.generate, seqs, NEW, [], PAD)
                assert steps == NEW
                r[tag] = (toks.copy(), _last(e8, len(seqs), dims.hidden))
            r["session"], refills = _session(e8, ses, ses_new, 4)      # (the session's and the drafting session's step graphs, or eager)
            assert refills >= 2, "no slot was re-used while others were decoding"
            r["draft"], _ = _session(e8, ses, ses_new, 4, draft=3)
            out[kv, graph] = r
    g1 = _guard(e8.greedy1, five)
    lg = _guard(e8.last_logits, five, ids)
    e8.close()
    ref = out[1, 1]
    for key, r in out.items():
        for tag in ("one", "five"):
            np.testing.assert_array_equal(ref[tag][0], r[tag][0], err_msg=f"{name} {tag}: tokens (llama_kv_fp8, dec_graph) (1, 1) vs {key}")
            assert ref[tag][1].tobytes() == r[tag][1].tobytes(), f"{name} {tag}: last rows (1, 1) vs {key}"
        assert r["session"] == ref["session"], f"{name}: session tokens (1, 1) vs {key}"
        assert r["draft"] == r["session"], f"{name}: the drafting session's tokens are not the plain session's, {key}"
    np.testing.assert_array_equal(ref["five"][0][3], ref["one"][0][0], err_msg=f"{name}: a row's tokens depend on its batch")
    # the prefill-only entries: an fp16 engine's, bit for bit
    e16 = _engine(dims, state)
    np.testing.assert_array_equal(g1, _guard(e16.greedy1, five))
    assert lg.tobytes() == _guard(e16.last_logits, five, ids).tobytes(), f"{name}: last_logits on an FP8-cache engine"
    t16, _ = _guard(e16.generate, five, NEW, [], PAD)
    np.testing.assert_array_equal(t16[:, 0], ref["five"][0][:, 0])    # column 0 is the prefill's
    moved = _last(e16, len(five), dims.hidden).tobytes() != ref["five"][1].tobytes()
    e16.close()
    assert moved, f"{name}: the FP8 cache must change the steps' rows for this test to mean anything"


# ---- 5. against the independent reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy-llama", "toy-qwen2", "toy-qwen3", "toy-mistral"])
def test_last_step_logits_against_the_kv8_oracle(name):
    dims, state = _state(name)
    base = K.families()[name][1]
    prompt = K.check5_prompt(dims)
    head = np.asarray(state["model.embed_tokens.weight"] if dims.tied_head else state["lm_head.weight"], dtype=f32)
    e8 = _engine(dims, state, kv_fp8=True)
    toks, steps = _guard(e8.generate, [prompt], K.CHECK5["max_new"], [], PAD)
    assert steps == K.CHECK5["max_new"]
    got = _last(e8, 1, dims.hidden)[0] @ head.T
    e8.close()
    fed = [int(t) for t in toks[0, :-1]]
    want, plain, scale, d_ref, bound = K.check5_reference(base, dims, state, prompt, fed)
    err = float(np.abs(got - want).max())
    print(f"{name}: max |logit - Kv8Oracle| = {err:.4e}; logit scale {scale:.3f}, 4e-3 x scale = {K.LOGIT_BOUND * scale:.4e}, D_ref = {d_ref:.4e}, bound {bound:.4e}; "
          f"against the plain oracle {float(np.abs(got - plain).max()):.4e}")
    assert err <= bound, (name, err, bound)


# ---- 6. the contract -----------------------------------------------------------------------------------------------------------------------
def test_refusals(eng8):
    from llmrankers._engine import RkEngine, RkLlamaEngine
    t5 = RkEngine(_synth.TOY_GATED_UNTIED, device=0, max_tokens=512, max_seqs=4, max_dec_len=2)
    try:
        assert t5.lib.rk_llama_set_kv_fp8(t5.h, 1) == ERR_STATE and b"Llama" in t5.lib.rk_last_error(t5.h)
    finally:
        t5.close()
    assert eng8.lib.rk_llama_set_kv_fp8(eng8.h, 0) == ERR_STATE and b"finalize" in eng8.lib.rk_last_error(eng8.h)
    dims64 = _synth.TOY_LLAMA_HD64
    e64 = RkLlamaEngine(dims64, device=0, max_tokens=512, max_seqs=4, kv_fp8=True)
    with pytest.raises(RkError, match="64-wide") as ei:
        e64.load_state(_synth.synth_state_dict(dims64, seed=K.SYNTH_SEED).items())
    assert ei.value.code == ERR_STATE
    e64.close()
    with pytest.raises(RkError):
        eng8.set_option("llama_kv_fp8", 2)
    with eng8.session(2, 64, 4, [], PAD):
        with pytest.raises(RkError, match="session") as ei:
            eng8.set_option("llama_kv_fp8", 0)
        assert ei.value.code == ERR_STATE
    eng8.set_option("llama_kv_fp8", 0)
    eng8.set_option("llama_kv_fp8", 1)
    # the debug entries: another engine, a bad mode, a position outside the cache
    dims, state = _state("toy-llama")
    plain = _engine(dims, state, max_tokens=256, max_seqs=4)
    p = A.build_step(3, 4, 2, [5], 16, "R")
    with pytest.raises(RkError) as ei:
        _kv8_step(plain, p, 0)
    assert ei.value.code == ERR_STATE
    plain.close()
    with pytest.raises(RkError) as ei:
        _kv8_step(eng8, p, 2)
    assert ei.value.code == ERR_INVALID
    p.pos = np.array([16], np.int32)
    with pytest.raises(RkError) as ei:
        _kv8_step(eng8, p, 0)
    assert ei.value.code == ERR_INVALID


def test_dec_r_2_falls_back_to_the_rule():
    """Qwen2's seven heads per kv head: llama_dec_r = 2 selects the R = 7 kernel on an fp16-cache engine and the rule's R = 1 on an
    FP8-cache engine (no R = 7 instantiation there), with the same tokens as llama_dec_r = 0"""
    dims, state = _state("toy-qwen2")
    seqs = _prompts(dims, [126, 9], seed=400)
    e8 = _engine(dims, state, kv_fp8=True)
    assert e8.debug_kv8_step(mode=0, qkv=np.zeros((1, 9 * 128), f16), pos=[0], cos=np.ones((4, 64), f32), sin=np.zeros((4, 64), f32),
                             cache=np.zeros(2 * 4 * 128, f16), H=7, n_kv=1, P=4, plan_only=True)["R"] == 1
    a, _ = _guard(e8.generate, seqs, NEW, [], PAD)
    la = _last(e8, 2, dims.hidden)
    e8.set_option("llama_dec_r", 2)
    assert e8.debug_kv8_step(mode=0, qkv=np.zeros((1, 9 * 128), f16), pos=[0], cos=np.ones((4, 64), f32), sin=np.zeros((4, 64), f32),
                             cache=np.zeros(2 * 4 * 128, f16), H=7, n_kv=1, P=4, plan_only=True)["R"] == 1
    b, _ = _guard(e8.generate, seqs, NEW, [], PAD)
    assert (a == b).all() and la.tobytes() == _last(e8, 2, dims.hidden).tobytes()
    e8.close()
    e16 = _engine(dims, state)
    e16.set_option("llama_dec_r", 2)
    assert e16.debug_attn(A.STEP, n_seq=1, H=7, n_kv=1, P=4, ldctx=7 * 128, plan_only=True)["R"] == 7
    e16.close()


def test_setter_off_is_the_engine_that_never_called_it():
    dims, state = _state("toy-llama")
    seqs = _prompts(dims, [126, 9, 130], seed=500)
    from llmrankers._engine import RkLlamaEngine
    never = _engine(dims, state)
    off = RkLlamaEngine(dims, device=0, max_tokens=2048, max_seqs=16)
    assert off.lib.rk_llama_set_kv_fp8(off.h, 0) == 0
    _guard(off.load_state, state.items())
    res = []
    for e in (never, off):
        toks, _ = _guard(e.generate, seqs, NEW, [], PAD)
        res.append((toks.tobytes(), _last(e, 3, dims.hidden).tobytes(), e.buffers()["lkv"]["cap"]))
        e.set_option("llama_kv_fp8", 0)                               # no effect on an engine without an FP8 cache
        again, _ = _guard(e.generate, seqs, NEW, [], PAD)
        assert again.tobytes() == toks.tobytes()
        e.close()
    assert res[0] == res[1]


# ---- 7. the size ---------------------------------------------------------------------------------------------------------------------------
def test_cache_is_at_most_052_of_the_fp16_cache():
    dims, state = _state("toy-llama")
    e16, e8 = _engine(dims, state), _engine(dims, state, kv_fp8=True)
    for lens, new in (([15], 1), ([120, 130, 7], 6), ([300] * 5, 20)):
        seqs = _prompts(dims, lens, seed=600)
        caps = []
        for e in (e16, e8):
            _guard(e.generate, seqs, new, [], PAD)
            caps.append(2 * e.buffers()["lkv"]["cap"])
        rows, P = len(lens), max(lens) + new
        assert caps[0] == dims.n_layers * 4 * rows * dims.n_kv_heads * P * 128, "the fp16 engine's cache"
        assert caps[1] == dims.n_layers * K.layer_bytes(rows, dims.n_kv_heads, P), "the layout's size"
        print(f"rows {rows} P {P}: {caps[1]} / {caps[0]} bytes = {caps[1] / caps[0]:.4f}")
        assert caps[1] <= 0.52 * caps[0], (rows, P, caps)
    e16.close(); e8.close()
