"""tests/_plan_lines.py against planners whose lines are known: the interval finder, the choice of totals, the non-vacuity check and
the batch builder that tests/test_gpu_llama_plan_lines.py runs against the engine's own planner.  No GPU."""
import pytest

import _plan_lines as L

PROBES = (45, 129, 300)
STEPS = (768, 1536, 4096)                  # the step planner's lines: plan changes behind each


def step_plan(t):
    return (sum(t > s for s in STEPS),)


def pp2_plan(t):
    """one round = 8192 rows: behind it the first 8192 rows go to a launch of their own, the rest's plan depends on the rest"""
    m = 8192 * (t // 8192) if t % 8192 else 0
    rest = t - m
    return ("small" if rest <= 1536 else "big", m)


def test_the_finder_gives_the_known_lines_and_asks_every_t():
    asked = []

    def plan(t):
        asked.append(t)
        return step_plan(t)

    ivs = L.intervals(plan, 6000)
    assert asked == list(range(1, 6001))
    assert [tuple(iv) for iv in ivs] == [(1, 768, (0,)), (769, 1536, (1,)), (1537, 4096, (2,)), (4097, 6000, (3,))]
    assert L.lines(ivs) == list(STEPS)
    # a plan that comes back after a gap is a new interval, not merged with its first stretch
    back = L.intervals(lambda t: (t % 100 < 50,), 250)
    assert [(iv.lo, iv.hi) for iv in back] == [(1, 49), (50, 99), (100, 149), (150, 199), (200, 249), (250, 250)]
    with pytest.raises(ValueError):
        L.intervals(step_plan, 0)


def test_every_interval_and_both_sides_of_every_line_get_a_total():
    ivs = L.intervals(step_plan, 6000)
    tot = L.totals(ivs, min(PROBES))
    for iv in ivs:
        assert any(iv.lo <= t <= iv.hi and any(w.startswith("inside") for w in why) for t, why in tot.items()), iv
    for line in STEPS:
        assert line in tot and line + 1 in tot, (line, sorted(tot))
        assert step_plan(line) != step_plan(line + 1)
    assert list(tot) == sorted(tot) and all(1 <= t <= 6000 for t in tot)
    # the pp2 planner: lines at 1536, 8192, 8192 + 1536
    ivs = L.intervals(pp2_plan, 10240)
    assert L.lines(ivs) == [1536, 8192, 9728]
    assert [iv.plan for iv in ivs] == [("small", 0), ("big", 0), ("small", 8192), ("big", 8192)]
    tot = L.totals(ivs, min(PROBES))
    assert {1536, 1537, 8192, 8193, 9728, 9729} <= set(tot)


def test_a_total_smaller_than_the_probes_is_refused_not_dropped():
    ivs = L.intervals(lambda t: (t > 30,), 200)              # a line at 30 | 31: below the shortest probe
    with pytest.raises(ValueError, match="below the smallest batch"):
        L.totals(ivs, min(PROBES))
    with pytest.raises(ValueError, match="cannot hold the probes"):
        L.build(473, PROBES, "first", max_seqs=32)
    with pytest.raises(ValueError, match="no filler"):
        L.build(475, PROBES, "first", max_seqs=32)            # one token beside the probes
    with pytest.raises(ValueError, match="no room"):
        L.fitting_probes(PROBES, 44)
    with pytest.raises(ValueError, match="no room"):
        L.fitting_probes(PROBES, 46)
    assert L.fitting_probes(PROBES, 45) == [0] and L.fitting_probes(PROBES, 64) == [0]
    assert L.fitting_probes(PROBES, 174) == [0, 1] and L.fitting_probes(PROBES, 175) == [0] and L.fitting_probes(PROBES, 256) == [0, 1]
    assert L.fitting_probes(PROBES, 474) == [0, 1, 2] and L.fitting_probes(PROBES, 475) == [0, 1] and L.fitting_probes(PROBES, 9000) == [0, 1, 2]
    with pytest.raises(ValueError, match="max_seqs"):
        L.build(474 + 30 * 512, PROBES, "last", max_seqs=32)


def test_a_constant_planner_still_gets_cases_and_the_vacuity_check_fires():
    ivs = L.intervals(lambda t: (6, 0, 1), 3000)
    assert [tuple(iv) for iv in ivs] == [(1, 3000, (6, 0, 1))] and L.lines(ivs) == []
    tot = L.totals(ivs, min(PROBES))
    assert len(tot) == 1 and 45 <= next(iter(tot)) <= 3000
    for t in tot:
        for how in L.ARRANGEMENTS:
            assert sum(L.build(t, PROBES, how, max_seqs=32).lens) == t
    kinds = {"64x64": lambda p: p[0] == 6, "ping-pong": lambda p: p[0] == 5}
    with pytest.raises(AssertionError, match="no ping-pong plan"):
        L.require_kinds(ivs, kinds)
    L.require_kinds(ivs, {"64x64": kinds["64x64"]})
    L.require_kinds(L.intervals(lambda t: (5 if t > 100 else 6,), 200), kinds)


def _check(b, T, lens, how, max_seqs):
    assert sum(b.lens) == T and len(b.lens) <= max_seqs, (T, how)
    rows = [sum(b.lens[:k]) for k in range(len(b.lens))]
    for i, n in enumerate(lens):
        assert b.lens[b.probe_at[i]] == n and b.row0[i] == rows[b.probe_at[i]], (T, how, i)
    assert len(set(b.probe_at)) == len(lens)
    if not b.cuts:
        assert list(b.probe_at) == sorted(b.probe_at)                            # the probes keep their order
    fillers = [n for k, n in enumerate(b.lens) if k not in b.probe_at]
    assert all(L.MIN_FILLER <= n <= L.MAX_FILLER for n in fillers), (T, how, fillers)
    if how == "first":
        assert b.probe_at == tuple(range(len(lens)))
    if how == "last":
        assert b.probe_at == tuple(range(len(b.lens) - len(lens), len(b.lens)))


@pytest.mark.parametrize("how", L.ARRANGEMENTS)
def test_totals_are_exact_and_fillers_bounded(how):
    for T in list(range(474, 474 + 40)) + [768, 769, 1536, 1537, 4096, 4097, 8191, 8192, 8193, 10240, 474 + 26 * 512]:
        if T == 475:
            continue
        _check(L.build(T, PROBES, how, max_seqs=32), T, PROBES, how, 32)
    for T in (45, 47, 64, 100):
        _check(L.build(T, PROBES[:1], how, max_seqs=32), T, PROBES[:1], how, 32)
    for T in (174, 176, 256, 257):
        _check(L.build(T, PROBES[:2], how, max_seqs=32), T, PROBES[:2], how, 32)
    if how != "spread":                                                          # (spread chops four gaps: up to three sequences more)
        _check(L.build(474 + 29 * 512, PROBES, how, max_seqs=32), 474 + 29 * 512, PROBES, how, 32)
    spread = L.build(4096, PROBES, "spread", max_seqs=32)
    assert spread.probe_at[0] > 0 and spread.probe_at[-1] < len(spread.lens) - 1    # fillers on both ends and between
    assert all(b - a > 1 for a, b in zip(spread.probe_at, spread.probe_at[1:]))


def test_probes_stand_on_both_sides_of_a_cut_and_the_report_is_true():
    cut = 8192
    for T in (8192 + 45, 8192 + 46, 8192 + 300, 9000, 9728, 9729, 10240):
        for how in L.ARRANGEMENTS:
            b = L.build(T, PROBES, how, max_seqs=32, cuts=[cut])
            _check(b, T, PROBES, how, 32)
            assert b.cuts == (cut,)
            for i, n in enumerate(PROBES):                                        # the report against the rows themselves
                rows = range(b.row0[i], b.row0[i] + n)
                assert (i in b.below[0]) == all(r < cut for r in rows), (T, how, i)
                assert (i in b.above[0]) == all(r >= cut for r in rows), (T, how, i)
        b = L.build(T, PROBES, "spread", max_seqs=32, cuts=[cut])
        assert b.below[0] and b.above[0], (T, b)                                  # one wholly below, one wholly above
        assert set(b.below[0]) | set(b.above[0]) == {0, 1, 2}, (T, b)             # and the one between straddles nothing
    # "last" at a rest shorter than the probes: some probe straddles, and the report says so
    b = L.build(8192 + 100, PROBES, "last", max_seqs=32, cuts=[cut])
    assert set(b.below[0]) | set(b.above[0]) != {0, 1, 2}
    # a rest shorter than the shortest probe: nothing can stand above, the builder does not pretend
    b = L.build(8192 + 10, PROBES, "spread", max_seqs=32, cuts=[cut])
    assert b.below[0] and not b.above[0]
    # a cut outside the call is none; two cuts: below / above each
    assert L.build(5000, PROBES, "spread", max_seqs=32, cuts=[8192]).cuts == ()
    b = L.build(10240, PROBES, "spread", max_seqs=32, cuts=[8192, 6400])
    assert b.cuts == (6400, 8192) and all(b.below) and all(b.above)
    assert all(set(lo) | set(hi) == {0, 1, 2} for lo, hi in zip(b.below, b.above))
