"""The rotary kernels where roundings part, on an MI355X: the rope op (rk_debug_rows op 8 / 11) and the cached step with its drafting
form (rk_debug_attn kind 5, g1 / live) on the aimed cases of tests/_rope_exact.py - rows, tables and biases on which the fused,
the unfused and the "other product" form of the rotation give different fp16 bytes in hundreds of elements per case
(tests/test_rope_exact_host.py counts them), where random data parts them in about 1.3e-4 of elements.

Form, exactly: the rope op's rows are the documented form's exact emulation byte for byte (width 128: fused on pair index % 8 == 0,
unfused elsewhere; width 64: fused everywhere; the bias sum in front, one fp16 rounding behind).
Equalities, byte for byte: for every rotated row the key heads and the (biased) value heads the rope op gives at position p are what
the cached step leaves in the cache at p, what the append of a drafting step (g1 = 2 and 8, dead rows writing nothing) leaves there,
and - bias = all zeros - what the bias-free kernels give, from the rope op and from the step.  At width 128 the last holds except the
sign of a zero (the bias-free kernels add nothing, -0 + 0.0f = +0): the rows hold signed-zero pairs and the test asserts that the
bytes differ exactly where the emulation says they do, zeros on both sides.  The bias-free 128-wide kernels are compiled per
instantiation, so every R the plan can choose has its case, on the plain and on the windowed engine.
Every call: the guard bands of the output, the cache and the rows intact, every cache byte no live row owns as it was, a second run
the same bytes, the plan's R the one the case is there for.  T = 32 rows, P = 40, every row at its own position."""
import numpy as np
import pytest

import _attn_ref as A
import _rope_exact as X
from llmrankers import _synth
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu

f16, f32, u16 = np.float16, np.float32, np.uint16
BAND, BAND_ROWS, ERR_HIP, EPS = 256, 8, -3, 1e-6
ENGINES = {"llama128": "toy-llama", "llama64": "toy-llama-hd64", "mistral128": "toy-mistral", "qwen3": "toy-qwen3"}
_ENG = {}


@pytest.fixture(scope="module")
def engines():
    """an engine per name, created when a test first asks for it, closed with the module (the debug entries take every shape from
    the call; the engine gives the head width, the window and the head norm)"""
    from llmrankers._engine import RkLlamaEngine

    def get(name):
        if name not in _ENG:
            dims = _synth.NAMED_DIMS[ENGINES[name]]
            _ENG[name] = RkLlamaEngine(dims, device=0, max_tokens=256, max_seqs=4).load_state(_synth.synth_state_dict(dims, seed=929).items())
        return _ENG[name]

    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _is_sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == A.SENTINEL).all())


def where_differs(c, got, want):
    """a sentence on where two sets of rows [T, ld] differ: how many elements, in which half of a pair, at which pair index % 8"""
    d = np.argwhere(got.view(u16) != want.view(u16))
    if not d.size:
        return ""
    nr, half = (c.H + c.n_kv) * c.hd, c.hd // 2
    rot = d[d[:, 1] < nr]
    col = rot[:, 1] % c.hd
    up, j = col >= half, (col % half) % 8
    t, k = d[0]
    return (f"{len(d)} elements differ ({len(rot)} rotated: {int((~up).sum())} lo / {int(up.sum())} up, {int((j == 0).sum())} at pair index % 8 == 0); first row {t}, "
            f"column {k} (head {k // c.hd}): {got[t, k]!r} against {want[t, k]!r}")


def rope_op(eng, c, bias=None, qkn=None):
    """op 8 (op 11 with the head-norm weights) in place on the case's rows -> the rows afterwards"""
    params = dict(rows=c.T, H=c.H, n_kv=c.n_kv, hd=c.hd, ld=c.ld, max_pos=c.max_pos)
    if qkn is None:
        op, ins, want = 8, [c.pos, c.cos, c.sin, bias], ((c.T, 1, 1), c.hd, int(bias is not None))
    else:
        op, ins, want = 11, [c.pos, c.cos, c.sin, qkn], ((c.T, 1, 1), 128, 2)
        params["eps"] = EPS
    pl = eng.debug_rows(op, ins=ins, outs=[c.rows], band=BAND, plan_only=True, **params)
    assert (pl["grid"], pl["tparam"], pl["variant"]) == want, pl
    a = eng.debug_rows(op, ins=ins, outs=[c.rows], band=BAND, **params)["all"][0]
    b = eng.debug_rows(op, ins=ins, outs=[c.rows], band=BAND, **params)["all"][0]
    assert np.array_equal(a, b), "rope op: a second run gives other bytes"
    assert (a[:, :BAND] == A.SENTINEL).all() and (a[:, -BAND:] == A.SENTINEL).all(), "rope op: a band was written"
    return np.ascontiguousarray(a[0, BAND:-BAND]).view(f16).reshape(c.T, c.ld)


def step(eng, c, what, bias=None, qkn=None, g1=0, live=None, want_R=None):
    """kind 5 on the case's rows over a cache of random finite values -> (cache before, cache after), each [2][cache rows][n_kv][P][hd]"""
    hd, n_rows = c.hd, c.T // max(g1, 1)
    q = A.sentinel16((c.T + 2 * BAND_ROWS, c.ld))
    q[BAND_ROWS:BAND_ROWS + c.T] = c.rows
    cache = np.random.RandomState(7).standard_normal(2 * n_rows * c.n_kv * c.P * hd).astype(f16)
    kw = dict(n_seq=c.T, H=c.H, n_kv=c.n_kv, q=q, out=A.sentinel16((c.T, c.H * hd)), band_rows=BAND_ROWS, P=c.P, ldq=c.ld, ldctx=c.H * hd, pos=c.pos,
              cos=c.cos, sin=c.sin, qkv_bias=bias, cache=cache, qk_norm=qkn, qk_eps=EPS if qkn is not None else 0.0)
    if g1:
        kw.update(g1=g1, live=live)
    plan = eng.debug_attn(A.STEP, plan_only=True, **kw)
    assert want_R is None or plan["R"] == want_R, f"{what}: the plan takes R = {plan['R']}, the case is there for R = {want_R}"
    res = []
    for _ in range(2):
        try:
            res.append(eng.debug_attn(A.STEP, **kw))
        except RkError as err:
            if err.code == ERR_HIP:              # a fault on the device: nothing more is started on it from this module
                pytest.exit(f"{what}: {err}", returncode=3)
            raise
    r, again = res
    assert r["out"].tobytes() == again["out"].tobytes() and r["cache"].tobytes() == again["cache"].tobytes(), f"{what}: a second run gives other bytes"
    cb = BAND_ROWS * hd
    assert _is_sentinel(r["out"][:BAND_ROWS]) and _is_sentinel(r["out"][-BAND_ROWS:]), f"{what}: a guard band of the output was written"
    assert _is_sentinel(r["cache"][:cb]) and _is_sentinel(r["cache"][-cb:]), f"{what}: a guard band of the cache was written"
    shape = (2, n_rows, c.n_kv, c.P, hd)
    return cache.reshape(shape), np.ascontiguousarray(r["cache"][cb:-cb]).reshape(shape)


def cache_problem(c, before, after, rotated, g1, live, what):
    """"" if `after` is `before` with the keys and values of the rotated rows at (cache row b / g1, the row's position) of every live
    row and nothing else changed; else a sentence"""
    keys, vals = X.key_value_heads(c, rotated)
    want = before.copy()
    for b in range(c.T):
        if live is None or live[b]:
            want[0, b // max(g1, 1), :, c.pos[b]] = keys[b]
            want[1, b // max(g1, 1), :, c.pos[b]] = vals[b]
    d = np.argwhere(after.view(u16) != want.view(u16))
    if not d.size:
        return ""
    owned = np.zeros(want.shape, bool)
    for b in range(c.T):
        if live is None or live[b]:
            owned[:, b // max(g1, 1), :, c.pos[b]] = True
    foreign = int((~owned[tuple(d.T)]).sum())
    dim = d[:, 4]
    up, j = dim >= c.hd // 2, (dim % (c.hd // 2)) % 8
    kv, row, g, p, e = d[0]
    return (f"{what}: {len(d)} cache elements differ from the rope op's rows ({int((d[:, 0] == 0).sum())} key / {int((d[:, 0] == 1).sum())} value elements; keys: "
            f"{int((~up & (d[:, 0] == 0)).sum())} lo / {int((up & (d[:, 0] == 0)).sum())} up, {int(((j == 0) & (d[:, 0] == 0)).sum())} at pair index % 8 == 0; {foreign} in rows no "
            f"live row owns); first {'key' if kv == 0 else 'value'} of cache row {row}, kv head {g}, position {p}, dim {e}: {after[kv, row, g, p, e]!r} against {want[kv, row, g, p, e]!r}")


def live_rows(T):
    live = np.ones(T, np.int32)
    live[3::5] = 0
    return live


def equalities(eng, c, what, bias=None, qkn=None, want_R=None):
    """rope op == plain step's cache == the drafting append's cache (g1 = 2, 8) -> (the rope op's rows, the sentences of what failed)"""
    rotated = rope_op(eng, c, bias=bias, qkn=qkn)
    bad = []
    for g1 in (0, 2, 8):
        live = live_rows(c.T) if g1 else None
        w = f"{what} {'plain step' if not g1 else f'drafting step g1={g1}'}"
        before, after = step(eng, c, w, bias=bias, qkn=qkn, g1=g1, live=live, want_R=want_R)
        bad.append(cache_problem(c, before, after, rotated, g1, live, w))
    return rotated, [b for b in bad if b]


# ---- form, exactly -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", X.FORM_CASES, ids=lambda k: f"hd{k[0]}-{k[1]}on{k[2]}-{'bias' if k[3] else 'nobias'}")
def test_rope_op_is_the_documented_form(engines, key):
    """(32, 8): 320 items, the kernel's loop makes its second trip"""
    c = X.case(*key)
    got = rope_op(engines("llama128" if c.hd == 128 else "llama64"), c, bias=c.bias)
    msg = where_differs(c, got, X.rotate(c))
    assert not msg, f"rope op {c.name} against the documented form: {msg}"


# ---- equalities: the bias-free 128-wide kernels, every instantiation ----------------------------------------------------------------------
R_OF = {(8, 8): (1, 0), (4, 2): (2, 0), (8, 2): (4, 0), (8, 1): (8, 0), (28, 4): (7, 2)}      # (H, n_kv) -> (R, llama_dec_r)


@pytest.mark.parametrize("name", ["llama128", "mistral128"])
@pytest.mark.parametrize("heads", X.EQUAL_HEADS_128, ids=lambda h: f"{h[0]}on{h[1]}")
def test_bias_free_128(engines, heads, name):
    eng, c = engines(name), X.case(128, heads[0], heads[1], False)
    R, dec_r = R_OF[heads]
    what = f"{name} {c.name} R={R}"
    zb = np.zeros((c.H + 2 * c.n_kv) * c.hd, f32)
    eng.set_option("llama_dec_r", dec_r)
    try:
        free, bad = equalities(eng, c, what, want_R=R)
        zero, bad_z = equalities(eng, c, what + " zero bias", bias=zb, want_R=R)
    finally:
        eng.set_option("llama_dec_r", 0)
    bad += bad_z
    # an all-zero bias gives the bias-free bits except the sign of a zero: the bytes differ exactly where the emulation's do
    d = free.view(u16) != zero.view(u16)
    want_d = X.rotate(c, bias=None).view(u16) != X.rotate(c, bias=zb).view(u16)
    if not ((free == 0) & (zero == 0))[d].all():
        bad.append(f"{what}: the rope op with an all-zero bias differs from the bias-free one beyond the sign of a zero: {where_differs(c, zero, free)}")
    elif not np.array_equal(d, want_d):
        bad.append(f"{what}: zeros change sign in {int(d.sum())} elements, the emulation says {int(want_d.sum())}")
    assert want_d.any(), "the case holds no signed-zero pair"
    assert not bad, "\n".join(bad)


# ---- equalities: the forms fixed in source from the start ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["llama128-bias", "llama64-nobias", "llama64-bias", "qwen3"])
def test_fixed_forms(engines, form):
    """one head pair each, (H, n_kv) = (4, 2).  Width 64 adds 0.0f without a bias: an all-zero bias gives the same bytes, zeros
    included.  Qwen3: the hardware rsqrt stands in front of the rotation, nothing is aimed - the same rows, equalities only."""
    if form == "qwen3":
        eng, c, kw = engines("qwen3"), X.case(128, 4, 2, False), dict(qkn=X.qk_weights())
    else:
        name, b = form.split("-")
        eng, c = engines(name), X.case(128 if name == "llama128" else 64, 4, 2, b == "bias")
        kw = dict(bias=c.bias)
    rotated, bad = equalities(eng, c, form, want_R=2, **kw)
    if form == "llama64-nobias":
        zb = np.zeros((c.H + 2 * c.n_kv) * c.hd, f32)
        zero, bad_z = equalities(eng, c, form + " zero bias", bias=zb, want_R=2)
        bad += bad_z
        msg = where_differs(c, zero, rotated)
        if msg:
            bad.append(f"{form}: the rope op with an all-zero bias differs from the bias-free one: {msg}")
    assert not bad, "\n".join(bad)
