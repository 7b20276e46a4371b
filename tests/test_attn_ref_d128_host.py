"""tests/_attn_ref_d128.py holds itself to its own rules on the CPU: the honest summation orders pass its tolerance with the ratio
its docstring quotes, and a reference that breaks one addressing rule of the 128-wide call fails on the fixtures the GPU test runs."""
import numpy as np
import pytest

import _attn_ref_d128 as D

LENS = [31, 200, 1, 64]
FIXTURES = {}


def fixture(tname):
    if tname not in FIXTURES:
        kw = {"S": dict(tier="S"), "spike": dict(tier="S", spike=[5, -7, 128, -128, 1, -1]), "R": dict(tier="R"), "Rflat": dict(tier="R", flat=True)}[tname]
        FIXTURES[tname] = D.build_enc(340 + len(FIXTURES), 3, LENS, band=8, pad=(64, 8), **kw)
    return FIXTURES[tname]


def test_honest_orders_pass():
    """chain, online softmax per 32 / 64 / 128 keys, 64-key flash merge: the largest (error - half ulp) / E stays within C"""
    worst = 0.0
    for tname in ("S", "spike", "R", "Rflat"):
        p = fixture(tname)
        for order, tile in (("chain", 64), ("online", 32), ("online", 64), ("online", 128), ("flash", 64)):
            worst = max(worst, D.judge(p, D.emulated(p, order, tile), what=f"{tname} {order}/{tile}"))
    print(f"honest orders at head width 128: largest (error - half ulp) / E = {worst:.2f} (C = {D.C})")
    assert worst <= D.C


def test_selector_fixture_has_its_traps_and_edges():
    p = fixture("S")
    assert p.n_traps >= 2 * p.H                       # the row before and the row behind, per head
    got = D.emulated(p)
    want = D.expected64(p)
    assert (got[:, :128 * p.H].view(np.uint16) == D.A.f16_sat(want[:, :128 * p.H]).view(np.uint16)).all()


@pytest.mark.parametrize("mut,tiers", [("stride64", ("S", "R")), ("bias_head", ("spike", "R")), ("drop_last", ("S", "R")), ("next_seq", ("S", "R"))])
def test_mutants_fail(mut, tiers):
    for tname in tiers:
        p = fixture(tname)
        with pytest.raises(AssertionError):
            D.judge(p, D.emulated(p, mut=mut), what=f"{tname} mutant {mut}")


def test_a_sequence_alone_is_the_same_problem():
    p = fixture("R")
    whole = D.emulated(p)
    for b in range(p.n_seq):
        s = D.alone(p, b)
        lo, hi = int(p.seq_off[b]), int(p.seq_off[b + 1])
        assert D.emulated(s).tobytes() == whole[lo:hi].tobytes()
