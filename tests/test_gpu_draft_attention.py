"""The attention of a drafting step alone on an MI355X: kv_cache_append_kernel and the attn_dec_keys_* entries through
rk_debug_attn kind 5 with g1 / live - plan_llama_dec_attn over the step rows and launch_llama_dec_attn with g1 / live, as llama_step_rows
calls them - against the fp64 reference of tests/_attn_ref_draft.py (tests/test_attn_ref_draft_host.py shows that it tells wrong
kernels apart on these very problems).

Per problem: the plan is the Python mirror's with n_seq = step rows; the guard bands of the output and of the cache are intact; a second
run gives the same bytes (dead rows included); the live rows' contexts are the reference's (tier S bit for bit, tier R within the
step references' half ulp + C x E - no tolerance of this file's); the cache afterwards holds the live rows' keys and values and is
otherwise the caller's bit for bit, the NaN poison above every slot's highest live position and a dead row's would-be position
included; llama_dec_r 0 / 1 (/ 2 where a kv head has 7 query heads) give the same bytes; and g1 PLAIN kind-5 calls, call j feeding
row (s, j) on the cache call j - 1 left, give every live row's context and the final cache byte for byte.

Head shapes G = 8, 4, 2, 1, 7 (R = 8, 4, 2, 1 and 1 / 7: the production R = 4 and R = 8 entries no whole-session toy launches), g1 =
2, 4, 8, P = 304 (three key chunks), the slots of _attn_ref_draft.slot_sets.  Engines: 128- and 64-wide Llama with and without the
q / k / v bias, toy-mistral at both widths (window 64, tier R: the selector designs know no window) and toy-qwen3 (head norm)."""
import numpy as np
import pytest

import _attn_ref as A
import _attn_ref_draft as X
from llmrankers import _synth
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_HIP, ERR_STATE = -1, -3, -4
LDC_CHUNK = 128
FORMS = {"llama128": ("toy-llama", "SR"), "llama64": ("toy-llama-hd64", "SR"), "mistral128": ("toy-mistral", "R"),
         "mistral64": ("toy-mistral-hd64", "R"), "qwen3": ("toy-qwen3", "R")}
RATIOS = {}
_ENGINES = {}


@pytest.fixture(scope="module")
def engines():
    """an engine per form, created when a test first asks for it, closed with the module"""
    from llmrankers._engine import RkLlamaEngine

    def get(form):
        if form not in _ENGINES:
            dims = _synth.NAMED_DIMS[FORMS[form][0]]
            _ENGINES[form] = (RkLlamaEngine(dims, device=0, max_tokens=256, max_seqs=4).load_state(_synth.synth_state_dict(dims, seed=929).items()), dims)
        return _ENGINES[form]

    yield get
    for e, _ in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def call_args(p, draft=True):
    kw = dict(n_seq=p.n_seq, H=p.H, n_kv=p.n_kv, q=p.q, out=p.out, band_rows=p.band, P=p.P, ldq=p.ldq, ldctx=p.ldctx, pos=p.pos, cos=p.cos, sin=p.sin,
              qkv_bias=p.qkv_bias, cache=p.cache, qk_norm=p.qk_w, qk_eps=p.qk_eps)
    if draft:
        kw.update(g1=p.g1, live=p.live)
    return kw


def mirror_step(dec_r, p, dims):
    G = p.H // p.n_kv
    R = 8 if G % 8 == 0 else 4 if G % 4 == 0 else 2 if G % 2 == 0 else 1
    if dec_r == 1:
        R = 1
    if dec_r == 2 and G == 7 and p.hd == 128:
        R = 7
    nch = -(-p.P // LDC_CHUNK)
    return dict(kind=1 if dims.sliding_window else (2 if p.qk_w is not None else 0), R=R, nch=nch, tparam=R, grid=(nch, p.H // R, p.n_seq), grid2=(p.H, p.n_seq, 1))


def _all_sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == A.SENTINEL).all())


def guarded(eng, what, **kw):
    try:
        return eng.debug_attn(A.STEP, **kw)
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{what}: {err}", returncode=3)
        raise


def run_problem(eng, dims, p, what):
    b, cb = p.band, p.band * p.hd
    bits = {}
    for dec_r in (0, 1, 2) if p.H // p.n_kv == 7 else (0, 1):
        eng.set_option("llama_dec_r", dec_r)
        try:
            plan = eng.debug_attn(A.STEP, plan_only=True, **call_args(p))
            for k, v in mirror_step(dec_r, p, dims).items():
                assert plan[k] == v, f"{what} llama_dec_r={dec_r}: plan field {k} = {plan[k]}, the shape should take {v} (plan {plan})"
            r = guarded(eng, what, **call_args(p))
            if dec_r == 0:
                again = guarded(eng, what, **call_args(p))
                assert r["out"].tobytes() == again["out"].tobytes() and r["cache"].tobytes() == again["cache"].tobytes(), f"{what}: a second run gives other bytes"
        finally:
            eng.set_option("llama_dec_r", 0)
        out, cache = r["out"], r["cache"]
        assert _all_sentinel(out[:b]) and _all_sentinel(out[-b:]), f"{what}: a guard band of the output was written"
        assert _all_sentinel(cache[:cb]) and _all_sentinel(cache[-cb:]), f"{what}: a guard band of the cache was written"
        bits[dec_r] = out[b:-b].tobytes() + cache[cb:-cb].tobytes()
        if dec_r == 0:
            ratio = X.judge(p, out[b:-b], what)
            X.judge_cache(p, cache[cb:-cb], what)
            ctx, left = out[b:-b], cache[cb:-cb]
    for k, v in bits.items():
        assert v == bits[0], f"{what}: llama_dec_r 0 and {k} are documented as the same bits and differ"
    # the sequential plain equivalent: byte for byte
    now = p.cache
    for j, (src, c) in enumerate(X.sequential(p)):
        c.cache = now
        r = guarded(eng, what, **call_args(c, draft=False))
        for s in np.flatnonzero(src == np.arange(p.n_slots) * p.g1 + j):
            assert r["out"][b + s].tobytes() == ctx[src[s]].tobytes(), f"{what}: step row {src[s]} differs from plain call {j} of the sequence"
        now = np.ascontiguousarray(r["cache"][cb:-cb])
    diff = np.flatnonzero(now.view(np.uint16) != left.view(np.uint16))
    if diff.size:
        half, (slot, g, t, d) = now.size // 2, np.unravel_index(diff[0] % (now.size // 2), (p.n_slots, p.n_kv, p.P, p.hd))
        raise AssertionError(f"{what}: the cache differs from the one the sequence of plain calls leaves in {diff.size} elements, first the "
                             f"{'key' if diff[0] < half else 'value'} of slot {slot}, kv head {g}, position {t}, dim {d}: {left[diff[0]]} against {now[diff[0]]}")
    return ratio


def run_cases(engines, form, heads, g1, bias):
    eng, dims = engines(form)
    name = f"attn_dec_keys{'_win' if dims.sliding_window else '_qkn' if dims.qk_norm else ''}<{dims.head_dim}>" + ("+bias" if bias else "")
    for tier in FORMS[form][1]:
        for call in range(3):
            p = X.problem(dims.head_dim, heads, g1, call, tier, bias=bias, W=dims.sliding_window, qkn=dims.qk_norm)
            what = f"draft step {form} {heads} g1={g1} bias={bias} call {call} tier {tier}"
            r = run_problem(eng, dims, p, what)
            if tier == "R":
                RATIOS[name] = max(RATIOS.get(name, 0.0), r)
                print(f"{what}: ratio {r:.2f}; max ratio so far: {name} {RATIOS[name]:.3f}")


@pytest.mark.parametrize("g1", X.G1S)
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("heads", X.HEADS, ids=lambda h: f"{h[0]}on{h[1]}")
@pytest.mark.parametrize("form", ["llama128", "llama64"])
def test_llama(engines, form, heads, bias, g1):
    run_cases(engines, form, heads, g1, bias)


@pytest.mark.parametrize("g1", X.G1S)
@pytest.mark.parametrize("heads,bias", [((8, 2), False), ((4, 4), True), ((28, 4), False), ((8, 1), True)], ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("form", ["mistral128", "mistral64"])
def test_windowed(engines, form, heads, bias, g1):
    """window 64: the slots at 190 .. 197 have their first visible key cross 127 / 128 - whole workgroups of chunk 0 return without a
    partial and the merge starts at chunk 1 - and the keys below lo inside a visible wave are finite and masked"""
    run_cases(engines, form, heads, g1, bias)


@pytest.mark.parametrize("g1", X.G1S)
@pytest.mark.parametrize("heads", [(8, 1), (8, 2), (4, 2), (28, 4)], ids=lambda h: f"{h[0]}on{h[1]}")
def test_head_norm(engines, heads, g1):
    run_cases(engines, "qwen3", heads, g1, False)


def test_refusals(engines):
    """n_seq no multiple of g1, g1 > 8, no live: RK_ERR_INVALID; the head norm with a bias, at width 64 or under a window:
    RK_ERR_STATE - before anything is launched; g1 = 0 and 1 are the plain call"""
    eng, dims = engines("llama128")
    p = X.problem(128, (4, 2), 4, 0, "R")

    def refused(e, code, **change):
        if "g1" in change:                                                   # (a cache of the size the binding expects of that g1)
            change["cache"] = np.zeros(2 * (p.n_seq // max(change["g1"], 1)) * p.n_kv * p.P * p.hd, np.float16)
        with pytest.raises(RkError) as ei:
            e.debug_attn(A.STEP, **dict(call_args(p), **change))
        assert ei.value.code == code, f"{sorted(change)}: status {ei.value.code}, expected {code}"

    refused(eng, ERR_INVALID, g1=5)                                          # 12 rows
    refused(eng, ERR_INVALID, g1=9)
    refused(eng, ERR_INVALID, g1=-1)
    refused(eng, ERR_INVALID, live=None)
    import _qwen3_ref as Q3
    w = Q3.head_weights(np.random.RandomState(1))
    refused(eng, ERR_STATE, qk_norm=w, qk_eps=1e-6, qkv_bias=np.zeros(p.ldq, np.float32))
    refused(engines("mistral128")[0], ERR_STATE, qk_norm=w, qk_eps=1e-6)
    p64 = X.problem(64, (4, 2), 4, 0, "R")
    with pytest.raises(RkError) as ei:
        engines("llama64")[0].debug_attn(A.STEP, **dict(call_args(p64), qk_norm=w[:128], qk_eps=1e-6))
    assert ei.value.code == ERR_STATE
    plain = X.sequential(p)[0][1]                                            # g1 = 0 and 1: the plain call, the same bytes
    plain.cache = p.cache
    res = [eng.debug_attn(A.STEP, **dict(call_args(plain, draft=False), **extra)) for extra in ({}, {"g1": 1}, {"g1": 1, "live": np.zeros(plain.n_seq, np.int32)})]
    assert all(r["out"].tobytes() == res[0]["out"].tobytes() and r["cache"].tobytes() == res[0]["cache"].tobytes() for r in res)
