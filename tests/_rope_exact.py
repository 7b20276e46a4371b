"""The rotary kernels' arithmetic, exactly: every rounding form a compiler or an author can give the rotation of one pair, and rows
built so that the forms give different fp16 bytes.

The rotation of a pair (x1, x2) by a table entry (cos, sin) is lo = cos x1 - sin x2, up = cos x2 + sin x1 in fp32 and ONE fp16
rounding (common.h: f2h_sat).  The fp32 part has three forms per output:
    unfused     two rounded products and an add                      rope_rot(fused = false)
    fused       lo = fma(cos, x1, -(sin x2)), up = fma(cos, x2, sin x1)    rope_rot(fused = true)
    other       lo = fma(-sin, x2, cos x1),   up = fma(sin, x1, cos x2)    the other product rounded: what a compiler may pick
They differ by at most one fp32 ulp, which shows in the fp16 byte only where the exact value lies within an fp32 ulp or so of an
fp16 rounding midpoint: about 1.3e-4 of random elements.  In front stands the bias sum (bias_add8: the fp32 add of the widened fp16
value and the fp32 bias; at width 64 the bias-free kernels add 0.0f, at width 128 they add nothing), behind it f2h_sat.
The documented form per kernel (csrc/llama_kernels.h, llama_kernels_hd64.h):
    width 128   fused on pair index % 8 == 0 (element 0 of a thread's eight), unfused elsewhere
    width 64    fused everywhere

The emulation is exact.  A product of two fp32 values is exact in fp64 and rounds to fp32 once; the sum behind an fma's exact product
is formed in fp64 with its rounding error (TwoSum) and, where that error is not zero, settled with fractions.Fraction.  Signed zeros
come out as IEEE gives them (the fp64 operations carry the signs).  The second half of the file is the same arithmetic written with
Fraction on one pair at a time (tests/test_rope_exact_host.py holds the two against each other on every element).

aimed_case builds rows [T, ld], tables [max_pos][hd / 2] and a bias on which the forms part.  The debug entries read the tables as
data, so an entry is any (cos, sin) in [-1, 1]^2: per (row, pair index) the base pair (x1, x2) and cos are drawn and sin is solved
so that the exact lo (pairs aimed at lo) or up lies at an fp16 midpoint, then moved by a few fp32 ulps to the value at which the
wanted one of the three forms is the odd one out.  A table entry belongs to every head of the row, so head h holds the base pair
times +-2^k(h) (and the base bias times the same factor): fp32 and fp16 rounding commute with such a factor away from the
subnormals, so every head, query or key, parts where the base pair parts.  A handful of cells hold x1 = -0 with x2 = +-0."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

f16, f32, f64, i32 = np.float16, np.float32, np.float64, np.int32
F16_MAX = 65504.0
UNFUSED, FUSED, OTHER = 0, 1, 2
FORM_NAMES = {UNFUSED: "unfused", FUSED: "fused", OTHER: "other"}
MUTANTS = ("other_fused", "fused_everywhere", "fused_nowhere", "f16_before_add", "bias_behind", "bias_f16", "pos_plus_1", "partner")


# ---- exact fp32 building blocks, vectorised ------------------------------------------------------------------------------------------
def _round_frac(q, prec, emin):
    """q (a Fraction whose denominator is a power of two, as every sum and product of floats is) rounded to nearest even at `prec`
    significand bits, exponents >= emin (gradual underflow) -> float (exact: at most 24 bits)"""
    n, d = abs(q.numerator), q.denominator
    if n == 0:
        return 0.0
    k = d.bit_length() - 1
    assert d == 1 << k
    lsb = max(n.bit_length() - 1 - k, emin) - prec + 1           # the exponent of the result's last place
    sh = lsb + k                                                 # |q| = n 2^-k = (n 2^-sh) 2^lsb
    if sh <= 0:
        m = n << -sh
    else:
        m, rem, half = n >> sh, n & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and m & 1):
            m += 1
    r = math.ldexp(m, lsb)
    return r if q > 0 else -r


def mul32(a, b):
    """fl32(a b): the product is exact in fp64"""
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)).astype(f32)


def add32(a, b):
    return (np.asarray(a, f32) + np.asarray(b, f32)).astype(f32)


def fma32(a, b, c):
    """fl32(a b + c) with ONE rounding.  p = a b is exact in fp64; s = fl64(p + c) with its exact error (TwoSum); err == 0: s is the
    exact sum and rounds once; else the element is settled with rationals."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    p, c64 = a.astype(f64) * b.astype(f64), c.astype(f64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    out = np.array(s.astype(f32))
    for k in np.flatnonzero(err != 0):
        out.flat[k] = float(_round_frac(Fraction(float(p.flat[k])) + Fraction(float(c64.flat[k])), 24, -126))
    fma32.settled += int(np.count_nonzero(err))
    return out


fma32.settled = 0


def f2h_sat(x):
    """common.h: (half_t)fminf(fmaxf(x, -65504), 65504)"""
    return np.clip(np.asarray(x, f32), f32(-F16_MAX), f32(F16_MAX)).astype(f16)


def rot(x1, x2, co, si, form):
    """(lo, up) in fp32 of one form; every operand fp32, broadcast against each other"""
    if form == UNFUSED:
        return add32(mul32(co, x1), -mul32(si, x2)), add32(mul32(co, x2), mul32(si, x1))
    if form == FUSED:
        return fma32(co, x1, -mul32(si, x2)), fma32(co, x2, mul32(si, x1))
    assert form == OTHER
    return fma32(-np.asarray(si, f32), x2, mul32(co, x1)), fma32(si, x1, mul32(co, x2))


def rot_by(x1, x2, co, si, forms):
    """forms: int array (broadcast against the operands) of UNFUSED / FUSED / OTHER per element"""
    x1, x2, co, si, forms = np.broadcast_arrays(np.asarray(x1, f32), np.asarray(x2, f32), np.asarray(co, f32), np.asarray(si, f32), np.asarray(forms))
    lo, up = np.zeros(x1.shape, f32), np.zeros(x1.shape, f32)
    for form in (UNFUSED, FUSED, OTHER):
        m = forms == form
        if m.any():
            lo[m], up[m] = rot(x1[m], x2[m], co[m], si[m], form)
    return lo, up


def documented_forms(hd):
    """per pair index: width 128 fused on index % 8 == 0, width 64 fused everywhere"""
    i = np.arange(hd // 2)
    return np.where(i % 8 == 0, FUSED, UNFUSED) if hd == 128 else np.full(hd // 2, FUSED)


# ---- a case through the documented form (or a mutant of it) ----------------------------------------------------------------------------
def _operands(c, rows, bias, mut):
    T, hd, half, nr = rows.shape[0], c.hd, c.hd // 2, c.H + c.n_kv
    x = rows[:, :nr * hd].reshape(T, nr, 2, half)
    x1h, x2h = x[:, :, 0], x[:, :, 1]
    if mut == "partner":
        x2h = x2h[..., np.arange(half) ^ 1]
    pos = (c.pos + 1) % c.max_pos if mut == "pos_plus_1" else c.pos
    co, si = c.cos[pos][:, None, :], c.sin[pos][:, None, :]
    b = None if bias is None else np.asarray(bias, f32)[:nr * hd].reshape(nr, 2, half)
    return x1h, x2h, b, co, si


def rotate(c, rows=None, bias="case", forms=None, mut=None):
    """The rows after the rotary kernel of width c.hd: q and k heads rotated at the rows' positions, with a bias the value heads
    biased, everything else (bias-free value heads, pad columns) as it was.  bias: "case" = the case's own, None = the bias-free
    kernel, or an array.  forms: per pair index, default the documented ones.  mut: one of MUTANTS."""
    rows = c.rows if rows is None else rows
    bias = c.bias if isinstance(bias, str) else bias
    hd, half, nr, nv = c.hd, c.hd // 2, c.H + c.n_kv, c.n_kv
    forms = documented_forms(hd) if forms is None else np.asarray(forms)
    if mut == "other_fused":
        forms = np.where(forms == FUSED, OTHER, forms)
    elif mut == "fused_everywhere":
        forms = np.full(half, FUSED)
    elif mut == "fused_nowhere":
        forms = np.full(half, UNFUSED)
    x1h, x2h, b, co, si = _operands(c, rows, bias, mut)
    x1, x2 = x1h.astype(f32), x2h.astype(f32)
    front = b is not None and mut != "bias_behind"
    if front:
        x1, x2 = add32(x1, b[None, :, 0]), add32(x2, b[None, :, 1])
        if mut == "bias_f16":
            x1, x2 = f2h_sat(x1).astype(f32), f2h_sat(x2).astype(f32)
    elif b is None and hd == 64:
        x1, x2 = add32(x1, f32(0)), add32(x2, f32(0))            # rope64_pairs: + 0.0f, what an all-zero bias adds
    if mut == "f16_before_add":
        lo = add32(f2h_sat(mul32(co, x1)).astype(f32), -f2h_sat(mul32(si, x2)).astype(f32))
        up = add32(f2h_sat(mul32(co, x2)).astype(f32), f2h_sat(mul32(si, x1)).astype(f32))
    else:
        lo, up = rot_by(x1, x2, co, si, forms[None, None, :])
    if b is not None and not front:
        lo, up = add32(lo, b[None, :, 0]), add32(up, b[None, :, 1])
    out = np.array(rows)
    out[:, :nr * hd] = np.stack([f2h_sat(lo), f2h_sat(up)], axis=2).reshape(rows.shape[0], nr * hd)
    if bias is not None:                                             # bias_v8: one rounding
        v = add32(rows[:, nr * hd:(nr + nv) * hd].astype(f32), np.asarray(bias, f32)[None, nr * hd:])
        out[:, nr * hd:(nr + nv) * hd] = f2h_sat(v)
    return out


def touched(c, bias):
    m = np.zeros((c.T, c.ld), bool)
    m[:, :(c.H + c.n_kv + (c.n_kv if bias is not None else 0)) * c.hd] = True
    return m


def key_value_heads(c, rotated):
    """[T, n_kv, hd] keys and values of rotated rows: what a step leaves in the cache at the row's position"""
    k0, v0 = c.H * c.hd, (c.H + c.n_kv) * c.hd
    return rotated[:, k0:v0].reshape(-1, c.n_kv, c.hd), rotated[:, v0:v0 + c.n_kv * c.hd].reshape(-1, c.n_kv, c.hd)


def separations(c):
    """{(out, fused_slot, pair of forms): number of rotated elements whose fp16 bytes differ between the two forms}, out in
    "lo" / "up", fused_slot = pair index % 8 == 0, over every q and k element of the case; and the largest |fp32 result|."""
    x1h, x2h, b, co, si = _operands(c, c.rows, c.bias, None)
    x1, x2 = x1h.astype(f32), x2h.astype(f32)
    if b is not None:
        x1, x2 = add32(x1, b[None, :, 0]), add32(x2, b[None, :, 1])
    r = {form: rot(x1, x2, co, si, form) for form in (UNFUSED, FUSED, OTHER)}
    slot = (np.arange(c.hd // 2) % 8 == 0)[None, None, :]
    counts = {}
    for o, name in enumerate(("lo", "up")):
        h = {form: f2h_sat(r[form][o]).view(np.uint16) for form in r}
        for fa, fb in ((UNFUSED, FUSED), (UNFUSED, OTHER), (FUSED, OTHER)):
            d = h[fa] != h[fb]
            counts[(name, True, (fa, fb))] = int((d & slot).sum())
            counts[(name, False, (fa, fb))] = int((d & ~slot).sum())
    return counts, float(max(np.abs(v).max() for pair in r.values() for v in pair))


# ---- rows on which the forms part ---------------------------------------------------------------------------------------------------
def head_factor(h):
    """head h holds the base pair times this: a power of two in 2^-3 .. 2^3, every third head negated"""
    return (-1.0 if h % 3 == 2 else 1.0) * 2.0 ** ((3 * h + 1) % 7 - 3)


ZERO_CELLS = [(0, 0), (1, 1), (2, 8), (3, 9), (4, 16), (5, 63)]     # (row, pair index) of the signed-zero pairs (pair index mod hd / 2)


def aimed_case(hd, H, n_kv, bias=False, T=32, P=40, seed=1, search=12):
    rs = np.random.RandomState(1000 * hd + 10 * H + n_kv + (5 if bias else 0) + seed)
    half, nr, n_all = hd // 2, H + n_kv, (H + 2 * n_kv) * hd
    ld = n_all + 8
    pos = rs.permutation(P)[:T].astype(i32)
    pos[0], pos[1] = (pos[0], pos[1]) if {0, P - 1} <= set(pos.tolist()) else (0, P - 1)
    if len(set(pos.tolist())) != T:                                  # (0 or P - 1 was drawn elsewhere as well)
        rest = [v for v in rs.permutation(P) if v not in (0, P - 1)]
        pos = np.array([0, P - 1] + rest[:T - 2], i32)
    t_idx, i_idx = np.arange(T)[:, None], np.arange(half)[None, :]

    def mags(shape):
        return 2.0 ** rs.uniform(-1, 3, shape)

    # the base pair per (row, pair index): fp16 values of magnitude 0.5 .. 8, the bias (per pair index) of their sign
    b1 = b2 = np.zeros(half, f32)
    s1, s2 = rs.choice([-1.0, 1.0], (T, half)), rs.choice([-1.0, 1.0], (T, half))
    if bias:
        b1, b2 = (rs.standard_normal(half) * 2).astype(f32), (rs.standard_normal(half) * 2).astype(f32)
        s1, s2 = np.broadcast_to(np.where(b1 < 0, -1.0, 1.0), (T, half)), np.broadcast_to(np.where(b2 < 0, -1.0, 1.0), (T, half))
    x1h, x2h = (s1 * mags((T, half))).astype(f16), (s2 * mags((T, half))).astype(f16)
    x1, x2 = add32(x1h.astype(f32), b1[None, :]), add32(x2h.astype(f32), b2[None, :])      # what the rotation sees
    co = (rs.choice([-1.0, 1.0], (T, half)) * rs.uniform(0.05, 1.0, (T, half))).astype(f32)
    aim_up = (i_idx // 8 + i_idx % 8 + t_idx) % 2 == 1
    # up = co x2 + si x1 aims with (a, d) = (x2, x1); lo = co x1 - si x2 with (a, d) = (x1, -x2): value = co a + si d
    a = np.where(aim_up, x2, x1).astype(f64)
    d = np.where(aim_up, x1, -x2).astype(f64)
    ca = co.astype(f64) * a
    u = rs.uniform(0.1, 0.85, (T, half)) * np.sign(ca) * np.sign(d)  # si d has the sign of co a: no cancellation, |value| >= 0.05
    v = ca + u * d
    ulp = 2.0 ** (np.floor(np.log2(np.abs(v))) - 10)
    m = (np.floor(v / ulp) + 0.5) * ulp                              # the fp16 rounding midpoint next to the value
    s0 = ((m - ca) / d).astype(f32)
    # a few fp32 ulps around s0: the nearest candidate at which the wanted form is the odd one of the three
    ks = np.array(sorted(range(-search, search + 1), key=abs), np.int32)
    cand = (s0.view(np.int32)[..., None] + ks).view(f32)
    forms3 = {form: rot(x1[..., None], x2[..., None], co[..., None], cand, form) for form in (UNFUSED, FUSED, OTHER)}
    h = {form: np.where(aim_up[..., None], f2h_sat(forms3[form][1]).view(np.uint16), f2h_sat(forms3[form][0]).view(np.uint16)) for form in forms3}
    uf, uo, fo = h[UNFUSED] != h[FUSED], h[UNFUSED] != h[OTHER], h[FUSED] != h[OTHER]
    odd = np.stack([uf & uo, uf & fo, uo & fo])                      # unfused / fused / other is the odd one out
    want = np.take_along_axis(odd, ((t_idx + i_idx // 8 + i_idx) % 3)[None, ..., None] * np.ones((1, T, half, ks.size), int), axis=0)[0]
    ok = np.abs(cand) <= 1.0
    first = lambda mask: np.where(mask.any(-1), mask.argmax(-1), -1)
    pick = first(want & ok)
    pick = np.where(pick < 0, first((uf | uo | fo) & ok), pick)
    pick = np.where(pick < 0, 0, pick)
    si = np.take_along_axis(cand, pick[..., None], -1)[..., 0]
    assert (np.abs(si) <= 1.0).all() and (np.abs(co) <= 1.0).all()
    cos, sin = np.zeros((P, half), f32), np.zeros((P, half), f32)
    ang = rs.uniform(0, 6.28, (P, half))                             # rows of the tables no row of the case stands at
    cos[:], sin[:] = np.cos(ang), np.sin(ang)
    cos[pos], sin[pos] = co, si
    rows = (rs.standard_normal((T, ld)) * 4).astype(f16)             # value heads and pad columns: random
    bvec = (rs.standard_normal(n_all) * 2).astype(f32) if bias else None
    for hh in range(nr):
        fac = head_factor(hh)
        rows[:, hh * hd:hh * hd + half] = (x1h.astype(f64) * fac).astype(f16)
        rows[:, hh * hd + half:(hh + 1) * hd] = (x2h.astype(f64) * fac).astype(f16)
        if bias:
            bvec[hh * hd:hh * hd + half], bvec[hh * hd + half:(hh + 1) * hd] = b1 * f32(fac), b2 * f32(fac)
    zeros = []
    for hh in (0, H):                                                # a query head and a key head
        for t, i in ZERO_CELLS:
            i %= half
            rows[t, hh * hd + i] = f16(-0.0)
            rows[t, hh * hd + half + i] = f16(-0.0) if t % 2 else f16(0.0)
            zeros.append((t, hh, i))
    return SimpleNamespace(hd=hd, H=H, n_kv=n_kv, T=T, P=P, max_pos=P, ld=ld, pos=pos, cos=cos, sin=sin, rows=rows, bias=bvec, aim_up=aim_up,
                           zero_cells=zeros, name=f"hd{hd}-{H}on{n_kv}-{'bias' if bias else 'nobias'}")


def qk_weights(seed=5):
    """Qwen3's q | k head-norm weights [256] for the equality checks on the 128-wide rows"""
    return (1.0 + 0.2 * np.random.RandomState(seed).standard_normal(256)).astype(f32)


# the cases tests/test_gpu_rope_forms.py runs, by (hd, H, n_kv, bias); built once per process
FORM_CASES = [(64, 4, 2, False), (64, 4, 2, True), (128, 4, 2, True), (128, 4, 2, False), (128, 32, 8, False)]
EQUAL_HEADS_128 = [(8, 8), (4, 2), (8, 2), (8, 1), (28, 4)]          # R = 1, 2, 4, 8 and, with llama_dec_r = 2, 7
ALL_CASES = FORM_CASES + [(128,) + hn + (False,) for hn in EQUAL_HEADS_128 if hn != (4, 2)]
_CASES = {}


def case(hd, H, n_kv, bias):
    key = (hd, H, n_kv, bool(bias))
    if key not in _CASES:
        c = aimed_case(*key)
        for a in (c.rows, c.cos, c.sin, c.pos) + ((c.bias,) if bias else ()):
            a.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


# ---- the same arithmetic in rationals, one pair at a time -----------------------------------------------------------------------------
def _neg(x):
    return np.signbit(x)


def _zero(neg):
    return -0.0 if neg else 0.0


def q_mul32(a, b):
    if a == 0 or b == 0:
        return _zero(_neg(a) != _neg(b))
    r = float(_round_frac(Fraction(a) * Fraction(b), 24, -126))
    return r if r != 0 else _zero(_neg(a) != _neg(b))


def q_add32(a, b):
    if a == 0 and b == 0:
        return _zero(_neg(a) and _neg(b))
    q = Fraction(a) + Fraction(b)
    return 0.0 if q == 0 else float(_round_frac(q, 24, -126))        # an exact zero sum of non-zeros: +0 (round to nearest)


def q_fma32(a, b, c):
    if a == 0 or b == 0:
        return _zero(_neg(a) != _neg(b) and _neg(c)) if c == 0 else float(c)
    q = Fraction(a) * Fraction(b) + Fraction(c)
    return 0.0 if q == 0 else float(_round_frac(q, 24, -126))


def q_f2h(x):
    if x == 0:
        return float(x)
    r = float(_round_frac(Fraction(min(max(x, -F16_MAX), F16_MAX)), 11, -14))
    return r if r != 0 else _zero(x < 0)


def q_pair(x1h, x2h, b1, b2, co, si, form, plus0):
    """one pair through the documented arithmetic -> (lo, up) as fp16 values.  b1 / b2: the bias entries or None; plus0: the
    bias-free + 0.0f of width 64."""
    x1, x2, co, si = float(x1h), float(x2h), float(co), float(si)
    if b1 is not None:
        x1, x2 = q_add32(x1, float(b1)), q_add32(x2, float(b2))
    elif plus0:
        x1, x2 = q_add32(x1, 0.0), q_add32(x2, 0.0)
    if form == FUSED:
        lo, up = q_fma32(co, x1, -q_mul32(si, x2)), q_fma32(co, x2, q_mul32(si, x1))
    elif form == OTHER:
        lo, up = q_fma32(-si, x2, q_mul32(co, x1)), q_fma32(si, x1, q_mul32(co, x2))
    else:
        lo, up = q_add32(q_mul32(co, x1), -q_mul32(si, x2)), q_add32(q_mul32(co, x2), q_mul32(si, x1))
    return q_f2h(lo), q_f2h(up)


def rotate_rational(c, bias="case"):
    """rotate(c, bias=bias) in rationals, element by element"""
    bias = c.bias if isinstance(bias, str) else bias
    hd, half, nr, nv = c.hd, c.hd // 2, c.H + c.n_kv, c.n_kv
    forms = documented_forms(hd)
    out = np.array(c.rows)
    for t in range(c.T):
        co, si = c.cos[c.pos[t]], c.sin[c.pos[t]]
        for hh in range(nr):
            base = hh * hd
            for i in range(half):
                b1, b2 = (None, None) if bias is None else (bias[base + i], bias[base + half + i])
                out[t, base + i], out[t, base + half + i] = q_pair(c.rows[t, base + i], c.rows[t, base + half + i], b1, b2, co[i], si[i], forms[i], hd == 64)
        if bias is not None:
            for j in range(nr * hd, (nr + nv) * hd):
                out[t, j] = q_f2h(q_add32(float(c.rows[t, j]), float(bias[j])))
    return out
