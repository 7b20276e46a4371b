"""Batch independence of the Llama engine where the prefill's GEMM plan changes with the number of tokens in the call.

include/rk_engine.h promises that a sequence's rk_llama_qlm score, its rk_llama_last_logits row, its generated tokens and a
session's tokens do not depend on what shares the call, bit for bit.  The other suites hold that at toy widths (K = 512), where
plan_gemm has one answer for every call.  Here the engine has the smallest widths at which the planner's answers differ by T

    LlamaDims(vocab=512, hidden=2048, n_heads=16, n_kv_heads=2, head_dim=128, intermediate=6144, n_layers=2)

(two layers: layer 1's K / V and everything behind them depend on layer 0's `down`), and the lines are not written down here but
FOUND: the four prefill projections, described as llama_prefill describes them, are planned (plan_only: nothing is launched) for
every T in 1 .. max_tokens, and tests/_plan_lines.py turns the answers into the maximal T-intervals of equal (variant, m_pp2,
ksplit, the rest's plan).  A batch of exactly T tokens is then built inside every interval and on both sides of every line - three
fixed probes of 45, 129 and 300 tokens among seeded fillers, the probes first, last and spread (behind a whole ping-pong round,
where the first m_pp2 rows go to a launch of their own: one probe wholly below that row and one wholly above) - and every
observable of every probe is compared with the probe alone.  Bit equality; there is no tolerance in this file.

That the observable can see a summation order at all is a test of its own (gemm_sk 0 against 2: the logits must differ), and the
rule the engine keeps is stated once more at the widths of the served checkpoints, on the planner alone (no weights): no T in
1 .. 32768 gives `o` or `down` a plan that sums K differently from another T's.

DESIGN.md "How batch independence is tested at plan lines" holds the interval table this module printed on the MI355X."""
import numpy as np
import pytest

import _gemm_ref as R
import _plan_lines as L

pytestmark = pytest.mark.gpu

MAX_TOKENS, MAX_SEQS = 10240, 32
PROBE_LENS = (45, 129, 300)
N_IDS = 64
FIELDS = ("variant", "m_pp2", "ksplit", "rest(variant, ksplit)")
REAL_T_MAX = 32768


def _dims():
    from llmrankers import _synth
    return _synth.LlamaDims(vocab=512, hidden=2048, n_heads=16, n_kv_heads=2, head_dim=128, intermediate=6144, n_layers=2)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def projections(d):
    """name -> (epilogue, N, K, folded-norm consumer, producer) of the prefill's GEMMs, as llama_prefill builds them: every consumer
    takes ready-made row factors, `o` and every layer's `down` but the last leave the next layer's statistics"""
    q, kv = d.n_heads * d.head_dim, d.n_kv_heads * d.head_dim
    return {"qkv": (R.EPI_STORE_F16, q + 2 * kv, d.hidden, True, False),
            "o": (R.EPI_RESID_F32, d.hidden, q, False, True),
            "gate|up": (R.EPI_SWIGLU_F16, 2 * d.intermediate, d.hidden, True, False),
            "down": (R.EPI_RESID_F32, d.hidden, d.intermediate, False, True),
            "down (last layer)": (R.EPI_RESID_F32, d.hidden, d.intermediate, False, False)}


def planner(eng, epi, n, k, consumer, producer):
    """plan(T) -> (variant, m_pp2, ksplit, rest) of the call on T rows under the engine's current options.  m_pp2 > 0: the first
    m_pp2 rows run on the ping-pong kernel (variant 5) with K split `ksplit`, the others as a launch of their own, which is planned
    like a call of T - m_pp2 rows (plan_gemm) - asked as one: rest = its (variant, ksplit); else rest = None."""
    z = np.zeros(8, np.float16)
    kw = dict(plan_only=True, producer=producer, rowscale=z if consumer else None)

    def raw(m):
        p = eng.debug_gemm_ex(epi, R.TILED, z, z, m, n, k, **kw)
        assert p["family"] == R.TILED, p
        return p["variant"], p["m_pp2"], p["ksplit"]

    def plan(t):
        v, m, ks = raw(t)
        if m == 0:
            return (v, 0, ks, None)
        rv, rm, rks = raw(t - m)
        assert 0 < m < t and rm == 0 and rv == v, (t, (v, m, ks), (rv, rm, rks))
        return (5, m, ks, (rv, rks))

    return plan


def k_orders(plan_tuple):
    """the K splits of the launches of one plan (variants 1 .. 6 sum K in one order, the split in another)"""
    return {plan_tuple[2]} | ({plan_tuple[3][1]} if plan_tuple[3] else set())


class World:
    """The engine and everything the tests of this module read, computed once and never modified."""

    def __init__(self):
        from llmrankers import _synth
        from llmrankers._engine import RkLlamaEngine
        self.dims = d = _dims()
        self.eng = RkLlamaEngine(d, device=0, max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS).load_state(_synth.synth_state_dict(d, seed=929, threads=8).items())
        self.ids = [int(i) for i in np.linspace(0, d.vocab - 1, N_IDS).round()]
        self.probes = [[int(t) for t in _synth.synth_token_batch(1, n, n, d.vocab, seed=5100 + n)[0]] for n in PROBE_LENS]
        # ---- the lines, from the planner ----
        self.sweeps = {name: L.intervals(planner(self.eng, *spec), MAX_TOKENS) for name, spec in projections(d).items()}
        self.totals = {}
        for name, ivs in self.sweeps.items():
            for t, why in L.totals(ivs, min(PROBE_LENS)).items():
                self.totals.setdefault(t, []).extend(f"{name}: {w}" for w in why)
        self.totals = dict(sorted(self.totals.items()))
        # a T whose `down` runs on the ping-pong kernel in one launch - split two ways, if the default rule ever splits
        pp = [iv for iv in self.sweeps["down"] if iv.plan[0] == 5 and iv.plan[1] == 0]
        pp.sort(key=lambda iv: -iv.plan[2])
        self.t_pp = (pp[0].lo + pp[0].hi) // 2 if pp else None
        # ---- every probe alone ----
        e = self.eng
        self.alone = []
        for p in self.probes:
            gen, steps = e.generate([p], 2, [], 0)
            assert steps == 2
            last = e.debug_read("llama_last", d.hidden).copy()
            self.alone.append(dict(logits=e.last_logits([p], self.ids)[0].copy(), qlm3=e.qlm([p], [3])[0], qlm_all=e.qlm([p], [len(p) - 1])[0],
                                   greedy1=int(e.greedy1([p])[0]), gen=[int(t) for t in gen[0]], last=last))
        self._batches = {}

    def cuts(self, t):
        """the rows at which some projection's plan cuts a call of t tokens into two launches"""
        return sorted({iv.plan[1] for ivs in self.sweeps.values() for iv in ivs if iv.lo <= t <= iv.hi and iv.plan[1] > 0})

    def batch(self, t, how):
        """(sequences, which probes, the builder's Batch) of the case (T, arrangement): built once"""
        if (t, how) not in self._batches:
            which = L.fitting_probes(PROBE_LENS, t)
            b = L.build(t, [PROBE_LENS[i] for i in which], how, max_seqs=MAX_SEQS, cuts=self.cuts(t))
            rs = np.random.RandomState(7000 + t)
            seqs = [rs.randint(3, self.dims.vocab - 28, size=n).astype(np.int32).tolist() for n in b.lens]
            for i, at in zip(which, b.probe_at):
                seqs[at] = self.probes[i]
            assert sum(len(s) for s in seqs) == t and all(len(s) <= max(L.MAX_FILLER, max(PROBE_LENS)) for s in seqs)
            self._batches[(t, how)] = (seqs, which, b)
        return self._batches[(t, how)]

    def cases(self):
        for t in self.totals:
            for how in L.ARRANGEMENTS:
                yield (t, how) + self.batch(t, how)

    def plans(self, t):
        return {name: next(iv.plan for iv in self.sweeps[name] if iv.lo <= t <= iv.hi) for name in self.sweeps}


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()


def _report(what, bad, n_cases):
    """every case that differs, with the plans its call ran under"""
    assert not bad, f"{what}: {len(bad)} of {n_cases} (T, arrangement, probe) cases differ from the probe alone:\n" + "\n".join(map(str, bad[:40]))


def test_the_lines_are_found_and_every_one_gets_cases_on_both_sides(world):
    w = world
    for name, ivs in w.sweeps.items():
        print(L.table(name, ivs, FIELDS))
        assert ivs[0].lo == 1 and ivs[-1].hi == MAX_TOKENS and all(a.hi + 1 == b.lo for a, b in zip(ivs, ivs[1:]))
        for iv in ivs:                                               # a case inside, and one on each side of each line
            assert any(iv.lo <= t <= iv.hi for t in w.totals), (name, iv)
        for line in L.lines(ivs):
            assert line in w.totals and line + 1 in w.totals, (name, line)
    print(f"{len(w.totals)} totals x {len(L.ARRANGEMENTS)} arrangements: {list(w.totals)}")
    for name in ("down", "down (last layer)"):                       # not vacuous: both kernel families, and a line between them
        L.require_kinds(w.sweeps[name], {"64x64": lambda p: p[0] == 6 and p[1] == 0, "ping-pong": lambda p: p[0] == 5})
    assert w.t_pp is not None
    print(f"K splits of the default plans: " + ", ".join(f"{name} {sorted(set().union(*(k_orders(iv.plan) for iv in ivs)))}" for name, ivs in w.sweeps.items()))
    # every case holds exactly T tokens, the probes where the builder says; behind a whole ping-pong round one probe stands wholly
    # below the cut and one wholly above it wherever the rest is long enough to hold a probe - and in every such interval it is
    for t, how, seqs, which, b in w.cases():
        assert sum(map(len, seqs)) == t and len(seqs) <= MAX_SEQS and [seqs[at] for at in b.probe_at] == [w.probes[i] for i in which]
    for name, ivs in w.sweeps.items():
        for iv in ivs:
            if iv.plan[1] == 0:
                continue
            stood = 0
            for t in (t for t in w.totals if iv.lo <= t <= iv.hi):
                b = w.batch(t, "spread")[2]
                k = b.cuts.index(iv.plan[1])
                if t - max(b.cuts) >= min(PROBE_LENS):
                    assert b.below[k] and b.above[k], (name, iv, t, b)
                stood += bool(b.below[k] and b.above[k])
            assert stood, f"{name} {iv}: no case with a probe on each side of row {iv.plan[1]}"


def test_last_logits_do_not_depend_on_the_call(world):
    w = world
    bad, n = [], 0
    for t, how, seqs, which, b in w.cases():
        got = w.eng.last_logits(seqs, w.ids)
        for i, at in zip(which, b.probe_at):
            n += 1
            diff = int((_u32(got[at]) != _u32(w.alone[i]["logits"])).sum())
            if diff:
                bad.append((t, how, f"probe {PROBE_LENS[i]} at row {b.row0[which.index(i)]}", f"{diff} of {N_IDS} logits differ",
                            f"max |d| {float(np.abs(got[at] - w.alone[i]['logits']).max()):.3e}", w.plans(t)["down"]))
    print(f"last_logits: {n} (T, arrangement, probe) cases, {len(bad)} differ")
    _report("last_logits", bad, n)


def test_qlm_scores_do_not_depend_on_the_call(world):
    w = world
    bad, n = [], 0
    for t, how, seqs, which, b in w.cases():
        for key, labels in (("qlm3", lambda s: 3), ("qlm_all", lambda s: len(s) - 1)):
            counts = [1] * len(seqs)
            for at in b.probe_at:
                counts[at] = labels(seqs[at])
            got = w.eng.qlm(seqs, counts)
            for i, at in zip(which, b.probe_at):
                n += 1
                if _u32(got[at]) != _u32(w.alone[i][key]):
                    bad.append((t, how, key, f"probe {PROBE_LENS[i]}", float(got[at]), float(w.alone[i][key]), w.plans(t)["down"]))
    print(f"qlm: {n} (T, arrangement, probe, label count) cases, {len(bad)} differ")
    _report("qlm", bad, n)


def test_greedy1_tokens_do_not_depend_on_the_call(world):
    w = world
    bad, n = [], 0
    for t, how, seqs, which, b in w.cases():
        got = w.eng.greedy1(seqs)
        for i, at in zip(which, b.probe_at):
            n += 1
            if int(got[at]) != w.alone[i]["greedy1"]:
                bad.append((t, how, f"probe {PROBE_LENS[i]}", int(got[at]), w.alone[i]["greedy1"]))
    _report("greedy1", bad, n)


def test_generate_tokens_and_step_rows_do_not_depend_on_the_call(world):
    """the prefill's cache feeding one step: the batch's cache has another P than the probe's alone"""
    w = world
    hid = w.dims.hidden
    bad, n = [], 0
    for t, how, seqs, which, b in w.cases():
        gen, steps = w.eng.generate(seqs, 2, [], 0)
        assert steps == 2
        last = w.eng.debug_read("llama_last", len(seqs) * hid).reshape(len(seqs), hid)
        for i, at in zip(which, b.probe_at):
            n += 1
            toks = [int(x) for x in gen[at]]
            diff = int((_u32(last[at]) != _u32(w.alone[i]["last"])).sum())
            if toks != w.alone[i]["gen"] or diff:
                bad.append((t, how, f"probe {PROBE_LENS[i]}", toks, w.alone[i]["gen"], f"{diff} of {hid} values of the step's final row differ",
                            w.plans(t)["down"]))
    print(f"generate: {n} (T, arrangement, probe) cases, {len(bad)} differ")
    _report("generate", bad, n)


@pytest.mark.parametrize("how", L.ARRANGEMENTS)
def test_session_tokens_and_first_step_rows_equal_generate_alone(world, how):
    """one admit whose prefill has T tokens, `down` on the ping-pong kernel (K split, wherever the default rule splits): the probes'
    tokens and, behind the first step, their final rows are those of rk_llama_generate on the probe alone"""
    w = world
    hid = w.dims.hidden
    plan = w.plans(w.t_pp)["down"]
    assert plan[0] == 5 and plan[1] == 0, plan
    seqs, which, b = w.batch(w.t_pp, how)
    assert which == [0, 1, 2]
    n_slots = len(seqs)
    toks = {}
    with w.eng.session(n_slots, L.MAX_FILLER + 8, 2, [], 0) as s:
        s.admit(seqs, list(range(n_slots)), [2] * n_slots)
        fin, steps = s.run(1)
        assert steps == 1
        rows = w.eng.debug_read("llama_last", n_slots * hid).reshape(n_slots, hid).copy()
        fin = list(fin)
        while len(fin) < n_slots:
            more, _ = s.run()
            assert more
            fin += more
        for at in b.probe_at:
            toks[at] = [int(x) for x in s.read(at)]
    print(f"session admit of {w.t_pp} tokens in {n_slots} slots, probes {how}: down plan {dict(zip(FIELDS, plan))}")
    for i, at in zip(which, b.probe_at):
        assert toks[at] == w.alone[i]["gen"], (how, PROBE_LENS[i], toks[at], w.alone[i]["gen"])
        diff = int((_u32(rows[at]) != _u32(w.alone[i]["last"])).sum())
        assert diff == 0, f"session, probes {how}: {diff} of {hid} values of probe {PROBE_LENS[i]}'s first step row differ from generate alone (down plan {plan})"


def test_the_logits_can_see_a_summation_order(world):
    """The condition of everything above: were the K split invisible in 64 logits of three probes, bit equality would prove nothing.
    The same batch with every projection on the ping-pong kernel, never split (gemm_sk = 0) and split wherever it fits (2)."""
    from test_gpu_gemm_handoff import Options
    w = world
    epi, n, k, consumer, producer = projections(w.dims)["down"]
    got, plans = {}, {}
    with Options(w.eng, gemm_variant=5, gemm_sk=2):
        split = [iv for iv in L.intervals(planner(w.eng, epi, n, k, consumer, producer), MAX_TOKENS) if iv.plan[:3] == (5, 0, 2)]
    assert split, "gemm_sk = 2 never splits `down`"
    t = (max(split[0].lo, sum(PROBE_LENS)) + split[0].hi) // 2
    seqs, which, b = w.batch(t, "spread")
    assert which == [0, 1, 2]
    before = w.eng.last_logits(seqs, w.ids)[list(b.probe_at)]
    for sk in (0, 2):
        with Options(w.eng, gemm_variant=5, gemm_sk=sk):
            plans[sk] = planner(w.eng, epi, n, k, consumer, producer)(t)
            got[sk] = w.eng.last_logits(seqs, w.ids)[list(b.probe_at)]
    assert plans[0][:3] == (5, 0, 1) and plans[2][:3] == (5, 0, 2), plans
    again = w.eng.last_logits(seqs, w.ids)[list(b.probe_at)]                  # the defaults are back
    differ = (_u32(got[0]) != _u32(got[2])).sum(axis=1)
    print(f"T = {t}: gemm_sk 0 against 2, logits that differ per probe {differ.tolist()} of {N_IDS}, "
          f"max |d| {float(np.abs(got[0] - got[2]).max()):.3e} at scale {float(np.abs(got[0]).max()):.2f}")
    assert differ.sum() > 0, "64 logits of three probes cannot tell the split sum from the unsplit one: widen the observable"
    assert (_u32(again) == _u32(before)).all()


REAL = ["LLAMA_3_8B", "LLAMA_32_1B", "QWEN25_7B", "QWEN3_4B", "QWEN3_8B", "MISTRAL_7B"]


@pytest.mark.parametrize("model", REAL)
def test_no_t_changes_the_k_order_at_served_widths(world, model):
    """The rule at real widths, on the planner alone: under the default options no T in 1 .. 32768 gives `o` or `down` a plan whose
    launches sum K differently from another T's - one K split for every launch of every T."""
    from llmrankers import _synth
    d = getattr(_synth, model)
    for name in ("o", "down", "down (last layer)"):
        spec = projections(d)[name]
        ivs = L.intervals(planner(world.eng, *spec), REAL_T_MAX)
        print(L.table(f"{model} {name} (N = {spec[1]}, K = {spec[2]})", ivs, FIELDS))
        orders = sorted(set().union(*(k_orders(iv.plan) for iv in ivs)))
        assert len(orders) == 1, (f"{model} {name}: the K split depends on T - " +
                                  "; ".join(f"T {iv.lo}..{iv.hi}: ksplit {sorted(k_orders(iv.plan))}" for iv in ivs))
