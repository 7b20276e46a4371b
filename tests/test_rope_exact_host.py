"""tests/_rope_exact.py on the CPU: the vectorised emulation against fractions.Fraction on every element of every case
tests/test_gpu_rope_forms.py uses; the cases part the rounding forms where they are said to; every mutant of the documented form
changes bytes of every case it applies to."""
from fractions import Fraction

import numpy as np
import pytest

import _rope_exact as X

u16 = np.uint16
CASE_IDS = [f"hd{hd}-{H}on{n_kv}-{'bias' if bias else 'nobias'}" for hd, H, n_kv, bias in X.ALL_CASES]


def test_fp32_blocks_against_rationals():
    """mul32 / add32 / fma32 / f2h_sat on operands that force the rational path (an addend far above and far below the product),
    ties, signed zeros, subnormals and the saturation"""
    rs = np.random.RandomState(3)
    n = 4000
    a = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(np.float32)
    b = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(np.float32)
    c = (rs.standard_normal(n) * 2.0 ** rs.randint(-40, 40, n)).astype(np.float32)
    c[:400] = -(a[:400].astype(np.float64) * b[:400].astype(np.float64)).astype(np.float32)          # cancellation: the fma's point
    for v in (a, b, c):
        v[rs.randint(0, n, 200)] = rs.choice([0.0, -0.0], 200)
    before = X.fma32.settled
    got = X.fma32(a, b, c)
    assert X.fma32.settled - before > 100, "no element took the rational path"
    for k in range(n):
        assert np.float32(X.q_fma32(float(a[k]), float(b[k]), float(c[k]))).view(np.uint32) == got[k].view(np.uint32), (a[k], b[k], c[k])
        assert np.float32(X.q_mul32(float(a[k]), float(b[k]))).view(np.uint32) == X.mul32(a[k], b[k]).view(np.uint32)
        assert np.float32(X.q_add32(float(a[k]), float(c[k]))).view(np.uint32) == X.add32(a[k], c[k]).view(np.uint32)
    # f2h_sat: every fp16 midpoint (a tie in fp32), its fp32 neighbours, the subnormals, the saturation, both zeros
    h = np.arange(0, 0x7C00, dtype=u16).view(np.float16).astype(np.float64)
    mid = ((h[:-1] + h[1:]) / 2).astype(np.float32)
    x = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1e9)), [65504.0, 65520.0, 7e4, 1e30, 0.0, 2.0 ** -25, 2.0 ** -26]]).astype(np.float32)
    x = np.concatenate([x, -x])
    got = X.f2h_sat(x)
    assert np.isfinite(got).all()
    for k in range(0, x.size, 7):
        assert np.float16(X.q_f2h(float(x[k]))).view(u16) == got[k].view(u16), x[k]
    assert X._round_frac(Fraction(3, 2) * Fraction(2) ** -24 + 1, 24, -126) == 1.0 + 2.0 ** -23       # 1 + 1.5 ulp/2 ... rounds up
    assert X._round_frac(Fraction(1) + Fraction(2) ** -24, 24, -126) == 1.0                           # a tie: to even


@pytest.mark.parametrize("key", X.ALL_CASES, ids=CASE_IDS)
def test_emulation_is_the_rational_arithmetic(key):
    c = X.case(*key)
    assert np.array_equal(X.rotate(c).view(u16), X.rotate_rational(c).view(u16))
    if not key[3] and (key[1], key[2]) == (4, 2):                    # the zero bias of the equality checks, where zeros change sign
        zb = np.zeros((c.H + 2 * c.n_kv) * c.hd, np.float32)
        assert np.array_equal(X.rotate(c, bias=zb).view(u16), X.rotate_rational(c, bias=zb).view(u16))


@pytest.mark.parametrize("key", X.ALL_CASES, ids=CASE_IDS)
def test_cases_part_the_forms(key):
    """in each of {lo, up} x {pair index % 8 == 0, other} at least 32 elements part each of the three pairs of forms; nothing near
    +-65504; tables in [-1, 1]; every row at its own position; aimed pairs of both kinds at fused and unfused indices; the
    signed-zero cells are there, in a query head and in a key head"""
    c = X.case(*key)
    counts, biggest = X.separations(c)
    assert len(counts) == 12
    for k, n in counts.items():
        assert n >= 32, f"{c.name}: only {n} elements part {X.FORM_NAMES[k[2][0]]} from {X.FORM_NAMES[k[2][1]]} in {k[0]}, pair index % 8 == 0: {k[1]}"
    assert biggest < 1024.0
    assert np.abs(c.cos).max() <= 1.0 and np.abs(c.sin).max() <= 1.0
    assert len(set(c.pos.tolist())) == c.T and c.pos.min() == 0 and c.pos.max() == c.P - 1
    slot = np.broadcast_to(np.arange(c.hd // 2) % 8 == 0, c.aim_up.shape)
    for up in (False, True):
        for s in (False, True):
            assert ((c.aim_up == up) & (slot == s)).sum() >= 32
    half = c.hd // 2
    assert {hh for _, hh, _ in c.zero_cells} == {0, c.H}
    for t, hh, i in c.zero_cells:
        x1, x2 = c.rows[t, hh * c.hd + i], c.rows[t, hh * c.hd + half + i]
        assert x1 == 0 and np.signbit(x1) and x2 == 0 and bool(np.signbit(x2)) == bool(t % 2)
    assert any(t % 2 for t, _, _ in c.zero_cells) and any(not t % 2 for t, _, _ in c.zero_cells)


def test_zero_bias_and_bias_free_differ_in_the_sign_of_zeros_only():
    """width 64 adds 0.0f in the bias-free kernels: the same bytes.  Width 128 adds nothing: the signed-zero cells, and only they,
    come out with another sign - the claim DESIGN.md makes, which the GPU file asserts of the kernels."""
    for hd in (64, 128):
        c = X.case(hd, 4, 2, False)
        zb = np.zeros((c.H + 2 * c.n_kv) * c.hd, np.float32)
        free, zero = X.rotate(c, bias=None), X.rotate(c, bias=zb)
        d = free.view(u16) != zero.view(u16)
        if hd == 64:
            assert not d.any()
        else:
            assert d.any() and ((free == 0) & (zero == 0))[d].all()
            rows = {t for t, _, _ in c.zero_cells}
            assert set(np.nonzero(d)[0].tolist()) <= rows


def applies(mut, key):
    hd, _, _, bias = key
    if mut == "fused_everywhere":
        return hd == 128                                             # width 64 IS fused everywhere
    if mut in ("bias_behind", "bias_f16"):
        return bias
    return True


@pytest.mark.parametrize("key", X.ALL_CASES, ids=CASE_IDS)
def test_every_mutant_changes_bytes(key):
    c = X.case(*key)
    base = X.rotate(c).view(u16)
    nr = (c.H + c.n_kv) * c.hd
    for mut in X.MUTANTS:
        if not applies(mut, key):
            assert np.array_equal(X.rotate(c, mut=mut).view(u16), base), f"{c.name}: {mut} should be the documented form here"
            continue
        got = X.rotate(c, mut=mut).view(u16)
        d = got != base
        assert d[:, :c.H * c.hd].any() and d[:, c.H * c.hd:nr].any(), f"{c.name}: mutant {mut} changes no byte of the query heads or of the key heads"
        assert not d[:, nr + (c.n_kv * c.hd if key[3] else 0):].any()
