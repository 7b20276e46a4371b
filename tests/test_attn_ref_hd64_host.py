"""tests/_attn_ref_hd64.py holds itself to its own rules on the CPU: the honest summation orders pass its tolerance with the figure
its docstring quotes, and a reference that breaks ONE rule of the 64-wide Llama calls fails - by orders of magnitude - on fixtures
of the shapes the GPU test runs."""
import numpy as np
import pytest

import _attn_ref_hd64 as D

A = D.A
FIXTURES = {}
STEP_POS = [0, 1, 63, 64, 127, 128, 129, 255, 256, 398]
ORDERS_OF_MAGNITUDE = 100.0          # a mutant's (error - half ulp) / E must exceed this: two orders of magnitude in the unit the honest
                                     # orders are measured in (they stay under 1.5, a kernel is allowed C = 3)


def prefill(tname):
    if ("p", tname) not in FIXTURES:
        kw = {"S": dict(tier="S"), "R": dict(tier="R"), "Rflat": dict(tier="R", flat=True)}[tname]
        FIXTURES[("p", tname)] = D.build_llama(640 + ("S", "R", "Rflat").index(tname), 4, 2, [31, 200, 1, 64], band=8, pad=(8, 64), **kw)
    return FIXTURES[("p", tname)]


def step(tname, bias):
    if ("s", tname, bias) not in FIXTURES:
        FIXTURES[("s", tname, bias)] = D.build_step(660 + 2 * ("S", "R").index(tname) + bias, 4, 2, STEP_POS, 400, tname, bias=bias, band=8)
    return FIXTURES[("s", tname, bias)]


def test_honest_orders_pass():
    """the chain, online softmax per 64-key tile, merge of 128-key chunks, four wave shares merged in order: the largest
    (error - half ulp) / E.  C = 3 (the project's) stands while this figure is at most 1.5."""
    worst = 0.0
    for tname in ("S", "R", "Rflat"):
        p = prefill(tname)
        for order, tile in (("chain", 64), ("online", 64), ("flash", 128)):
            worst = max(worst, D.judge(p, D.emulated(p, order, tile), what=f"prefill {tname} {order}/{tile}"))
    for tname in ("S", "R"):
        for bias in (False, True):
            p = step(tname, bias)
            for order, tile in (("chain", 64), ("online", 64), ("flash", 128), ("waves", 0)):
                worst = max(worst, D.judge(p, D.emulated(p, order, tile), what=f"step {tname} bias={bias} {order}/{tile}"))
            D.judge_cache(p, D.emulated_cache(p), what=f"step {tname} bias={bias} cache")
    print(f"honest orders at head width 64: largest (error - half ulp) / E = {worst:.2f} (C = {D.C})")
    assert worst <= 1.5 and D.C == 3.0


def test_selector_fixtures_have_their_traps_and_are_exact():
    p = prefill("S")
    assert p.n_traps >= 2 * p.n_seq * p.n_kv
    got, want = D.emulated(p), D.expected64(p)
    own = ~np.isnan(want)
    assert (got[own].view(np.uint16) == A.f16_sat(want[own]).view(np.uint16)).all()
    for bias in (False, True):
        s = step("S", bias)
        assert s.n_traps >= sum(1 for t in STEP_POS if t + 1 < 400)
        assert D.emulated(s).tobytes() == A.f16_sat(D.expected64(s)).tobytes()


@pytest.mark.parametrize("mut", D.MUTANTS_PREFILL)
def test_prefill_mutants_fail(mut):
    """scale 128**-0.5 (tier R: a selector's winner wins under any positive scale), the wrong kv head for a query head, key i + 1
    admitted"""
    for tname in (("R",) if mut == "scale128" else ("S", "R")):
        p = prefill(tname)
        got = D.emulated(p, mut=mut)
        with pytest.raises(AssertionError):
            D.judge(p, got, what=f"prefill {tname} mutant {mut}")
        if tname == "R":
            r = D.miss(p, got)
            print(f"prefill mutant {mut}: (error - half ulp) / E = {r:.0f}")
            assert r > ORDERS_OF_MAGNITUDE, (mut, r)


@pytest.mark.parametrize("mut", D.MUTANTS_STEP)
def test_step_mutants_fail(mut):
    """pairing i with i + 64, scale 128**-0.5, the wrong kv head, the cache row behind pos admitted, bias added after the rotation"""
    for tname in ("S", "R"):
        for bias in ((True,) if mut == "bias_after_rot" else (False, True)):
            if tname == "S" and mut in ("pair_i64", "bias_after_rot", "scale128"):
                continue                          # identity tables and a winner that wins under any scale: the tier has nothing to say
            p = step(tname, bias)
            got = D.emulated(p, mut=mut)
            with pytest.raises(AssertionError):
                D.judge(p, got, what=f"step {tname} bias={bias} mutant {mut}")
            if tname == "R":
                r = D.miss(p, got)
                print(f"step mutant {mut} bias={bias}: (error - half ulp) / E = {r:.0f}")
                assert r > ORDERS_OF_MAGNITUDE, (mut, bias, r)


def test_key_written_behind_pos_fails():
    """new key written at pos + 1: the cache check names the element"""
    for tname in ("S", "R"):
        p = step(tname, True)
        with pytest.raises(AssertionError):
            D.judge_cache(p, D.emulated_cache(p, mut="write_pos1"), what=f"step {tname} mutant write_pos1")


def test_rotation_mutants_fail_on_the_cache_too():
    p = step("R", True)
    for mut in ("pair_i64", "bias_after_rot"):
        kc = D.expected_cache(p, emul=True).astype(D.f16)
        for it in D.items(p, mut, emul=True):
            b, g, pos, knew, _ = it["new"]
            kc[((b * p.n_kv + g) * p.P + pos) * D.HD:((b * p.n_kv + g) * p.P + pos + 1) * D.HD] = knew
        with pytest.raises(AssertionError):
            D.judge_cache(p, kc, what=f"cache mutant {mut}")


def test_a_sequence_and_a_row_alone_are_the_same_problem():
    p = prefill("R")
    whole = D.emulated(p)
    for b in range(p.n_seq):
        s = D.alone(p, b)
        lo, hi = int(p.seq_off[b]), int(p.seq_off[b + 1])
        assert D.emulated(s).tobytes() == whole[lo:hi].tobytes()
    q = step("R", True)
    rows = D.emulated(q)
    for b in range(q.n_seq):
        assert D.emulated(D.row_alone(q, b)).tobytes() == rows[b:b + 1].tobytes()
