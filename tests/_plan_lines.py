"""Plan lines: where a launch planner, read as a function plan(T) -> tuple of the number of rows T in a call, changes its answer,
and batches that stand on both sides of every such line.  Plain Python over a callable - the GPU test (test_gpu_llama_plan_lines.py)
hands in the engine's own plan_only calls, the host test (test_plan_lines_host.py) fake planners with known lines.

Nothing here knows a tile size or a threshold: the lines are FOUND, by asking the planner for every T.

    intervals(plan, t_max)          the maximal T-intervals of equal plan(T)
    totals(ivs, t_min)              one T inside every interval and both sides of every line; refuses what lies below t_min
    require_kinds(ivs, kinds)       the sweep is not vacuous: every named predicate holds on some interval
    fitting_probes(lens, T)         the probes a batch of T tokens has room for
    build(T, lens, how, ...)        the batch: probes first / last / spread, fillers in between, T tokens exactly
"""
from typing import Callable, Dict, List, NamedTuple, Sequence, Tuple

MAX_FILLER = 512          # tokens per filler sequence, at most
MIN_FILLER = 2            # ... and at least (a sequence that is scored needs a token in front of its label)
ARRANGEMENTS = ("first", "last", "spread")


class Interval(NamedTuple):
    lo: int
    hi: int               # inclusive
    plan: tuple


def intervals(plan: Callable[[int], tuple], t_max: int, t_min: int = 1) -> List[Interval]:
    """The maximal intervals [lo, hi] of t_min..t_max on which plan(T) is one value, in order: every T asked, none skipped."""
    if t_max < t_min:
        raise ValueError(f"empty sweep {t_min}..{t_max}")
    out, lo, cur = [], t_min, plan(t_min)
    for t in range(t_min + 1, t_max + 1):
        p = plan(t)
        if p != cur:
            out.append(Interval(lo, t - 1, cur))
            lo, cur = t, p
    out.append(Interval(lo, t_max, cur))
    return out


def lines(ivs: Sequence[Interval]) -> List[int]:
    """T_line of every line: the last T of every interval but the last (T_line + 1 is the first T of the next plan)."""
    return [iv.hi for iv in ivs[:-1]]


def totals(ivs: Sequence[Interval], t_min: int) -> Dict[int, List[str]]:
    """{T: why}: the middle of every interval (of its part from t_min on) and T_line, T_line + 1 of every line.  t_min: the smallest
    batch the caller can build.  An interval or a side of a line below t_min cannot get a case: ValueError - never dropped."""
    out: Dict[int, List[str]] = {}
    for k, iv in enumerate(ivs):
        if iv.hi < t_min:
            raise ValueError(f"interval {iv.lo}..{iv.hi} lies below the smallest batch ({t_min} tokens): it cannot get a case")
        out.setdefault((max(iv.lo, t_min) + iv.hi) // 2, []).append(f"inside {iv.lo}..{iv.hi}")
        if k + 1 < len(ivs):
            out.setdefault(iv.hi, []).append(f"line {iv.hi}|{iv.hi + 1}: below")
            out.setdefault(iv.hi + 1, []).append(f"line {iv.hi}|{iv.hi + 1}: above")
    return dict(sorted(out.items()))


def require_kinds(ivs: Sequence[Interval], kinds: Dict[str, Callable[[tuple], bool]]) -> None:
    """AssertionError unless every predicate of `kinds` holds for the plan of at least one interval: a sweep that never met, say,
    the ping-pong kernel has no line to stand on, and a test over it would pass for lack of cases."""
    missing = [name for name, pred in kinds.items() if not any(pred(iv.plan) for iv in ivs)]
    assert not missing, f"the sweep found no {' / '.join(missing)} plan in {[tuple(iv) for iv in ivs]}"


def table(name: str, ivs: Sequence[Interval], fields: Sequence[str]) -> str:
    """The interval table of one sweep, one line per interval."""
    rows = [f"{name}: {len(ivs)} intervals, lines at {lines(ivs)}"]
    for iv in ivs:
        rows.append(f"  T {iv.lo:>6} .. {iv.hi:<6} " + "  ".join(f"{f}={v}" for f, v in zip(fields, iv.plan)))
    return "\n".join(rows)


def fitting_probes(lens: Sequence[int], T: int) -> List[int]:
    """Indices of the probes a batch of exactly T tokens takes: the longest prefix of `lens` whose sum leaves no room or room for a
    filler (T - sum == 0 or >= MIN_FILLER).  ValueError when not even the first fits."""
    best = None
    for n in range(1, len(lens) + 1):
        rest = T - sum(lens[:n])
        if rest == 0 or rest >= MIN_FILLER:
            best = n
    if best is None:
        raise ValueError(f"a batch of {T} tokens has no room for a probe of {lens[0]}")
    return list(range(best))


class Batch(NamedTuple):
    lens: Tuple[int, ...]                 # every sequence's length, in batch order: sum == T
    probe_at: Tuple[int, ...]             # probe i is sequence probe_at[i]
    row0: Tuple[int, ...]                 # ... and starts at this row of the call
    cuts: Tuple[int, ...]                 # the cuts inside the call, ascending
    below: Tuple[Tuple[int, ...], ...]    # per cut: the probes that end at or in front of it (rows [row0, row0 + len) all < cut)
    above: Tuple[Tuple[int, ...], ...]    # per cut: the probes that start at or behind it
    # (a probe in neither list straddles the cut)


def _chop(n: int) -> List[int]:
    """n filler tokens as sequences of MIN_FILLER..MAX_FILLER tokens, as few as possible, as even as possible"""
    if n == 0:
        return []
    if n < MIN_FILLER:
        raise ValueError(f"a gap of {n} token(s) holds no filler of at least {MIN_FILLER}")
    k = -(-n // MAX_FILLER)
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


def _groups(n: int, k: int) -> List[int]:
    """n filler tokens in at most k groups, each 0 or >= MIN_FILLER, the non-empty ones first"""
    k = max(1, min(k, n // MIN_FILLER))
    return [n // k + (1 if i < n % k else 0) for i in range(k)] if n else []


def build(T: int, probe_lens: Sequence[int], how: str, *, max_seqs: int, cuts: Sequence[int] = ()) -> Batch:
    """A batch of exactly T tokens: the probes (lengths probe_lens, in this order of rows) and fillers of MIN_FILLER..MAX_FILLER
    tokens each, at most max_seqs sequences.

    how = "first": the probes, then the fillers; "last": the fillers, then the probes; "spread": fillers in front of, between and
    behind the probes.  cuts: rows at which the call is cut into launches (a plan's m_pp2).  With cuts, "spread" pins the first
    probe to row 0 and the SHORTEST probe to the call's end, and moves the ones between off every cut - so that, wherever the
    lengths allow it at all, one probe lies wholly below and one wholly above every cut; the result says, per cut, which probes lie
    where.

    ValueError: T smaller than the probes (or one token larger: no filler fits), more than max_seqs sequences, no placement."""
    if how not in ARRANGEMENTS:
        raise ValueError(how)
    n, need = len(probe_lens), sum(probe_lens)
    if n == 0 or min(probe_lens) < 1:
        raise ValueError("no probes")
    if T < need:
        raise ValueError(f"a batch of {T} tokens cannot hold the probes ({need} tokens)")
    fill = T - need
    if 0 < fill < MIN_FILLER:
        raise ValueError(f"a batch of {T} tokens leaves {fill} token(s) beside the probes: no filler of at least {MIN_FILLER}")
    cuts = sorted(c for c in cuts if 0 < c < T)
    order = list(range(n))                                          # the probes' order of rows
    if how == "spread" and cuts and n > 1:                          # the shortest goes to the end: it fits behind a cut soonest
        short = min(range(n), key=lambda i: (probe_lens[i], i))
        order = [i for i in range(n) if i != short] + [short]
    pl = [probe_lens[i] for i in order]
    # gaps[k]: filler tokens in front of the k-th probe; gaps[n]: behind the last
    if how == "first":
        gaps = [0] * n + [fill]
    elif how == "last":
        gaps = [fill] + [0] * n
    elif not cuts or n == 1:
        g = _groups(fill, n + 1)
        gaps = g + [0] * (n + 1 - len(g))
    else:
        start = [0] * n
        start[-1] = T - pl[-1]
        lo = pl[0]
        for k in range(1, n - 1):                                   # the ones between: the first free place that straddles no cut
            hi_free = start[-1] - sum(pl[k + 1:n - 1])              # what the probes behind this one still need stays free
            cands = [lo] + [c for c in cuts] + [c - pl[k] for c in cuts]
            ok = [s for s in sorted(cands) if s >= lo and s + pl[k] <= hi_free and (s - lo == 0 or s - lo >= MIN_FILLER)
                  and (hi_free - s - pl[k] == 0 or hi_free - s - pl[k] >= MIN_FILLER)
                  and not any(s < c < s + pl[k] for c in cuts)]
            if not ok:
                raise ValueError(f"no place for probe {order[k]} between rows {lo} and {hi_free} off the cuts {cuts}")
            start[k] = ok[0]
            lo = ok[0] + pl[k]
        gaps = [start[0]] + [start[k] - start[k - 1] - pl[k - 1] for k in range(1, n)] + [0]
    lens: List[int] = []
    probe_at, row0 = [0] * n, [0] * n
    for k in range(n + 1):
        lens += _chop(gaps[k])
        if k < n:
            probe_at[order[k]], row0[order[k]] = len(lens), sum(lens)
            lens.append(pl[k])
    if sum(lens) != T:
        raise AssertionError((T, lens))
    if len(lens) > max_seqs:
        raise ValueError(f"{len(lens)} sequences for {T} tokens, max_seqs {max_seqs}")
    below = tuple(tuple(i for i in range(n) if row0[i] + probe_lens[i] <= c) for c in cuts)
    above = tuple(tuple(i for i in range(n) if row0[i] >= c) for c in cuts)
    return Batch(tuple(lens), tuple(probe_at), tuple(row0), tuple(cuts), below, above)
