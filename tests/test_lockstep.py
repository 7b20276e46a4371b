"""The lock-step driver (llmrankers/_lockstep.py) on toy chains, the two-slot loop on a recording fake, and the setwise and
pairwise sorts through all of their drivers.

CPU only, no model and no runtime: the comparator is a function of the window's docids, so a label does not depend on the order
in which the windows are compared and the three ways to run a sort - the reference's one-by-one order (the one
tests/golden/sort_traces.json ties to the reference, test_host_logic.py), the level-batched build phase, and rerank_many over
several queries - can be held against each other compare by compare."""
import contextlib
import io

import pytest

from llmrankers import pairwise
from llmrankers._lockstep import Lockstep, alternate, drive
from llmrankers.pairwise import DuoT5LlmRanker, PairwiseLlmRanker
from llmrankers.rankers import SearchResult
from llmrankers.setwise import SetwiseLlmRanker


def toy(name, script, sent, result=None):
    """a chain that yields the window lists of `script` one after another and notes what it is sent"""
    for windows in script:
        labels = yield windows
        sent.append((name, windows, labels))
    return name if result is None else result


def answer(windows):
    return [w.upper() for w in windows]


def test_chains_of_unequal_length_advance_together():
    sent = []
    chains = Lockstep({"c": toy("c", [["c1"], ["c2"], ["c3"]], sent),
                       "a": toy("a", [["a1"]], sent, result=[7, 8]),
                       "d": toy("d", [], sent),                                   # ends before its first yield
                       "b": toy("b", [["b1", "b2", "b3"], ["b4"]], sent)})       # several windows at once
    assert chains.returned == {"d": "d"} and chains.live() == ["a", "b", "c"]
    steps = []
    while chains:
        keys, windows = chains.pending()
        steps.append((keys, windows))
        chains.advance(answer(windows))
    assert steps == [(["a", "b", "b", "b", "c"], ["a1", "b1", "b2", "b3", "c1"]),   # sorted key order, a key per window
                     (["b", "c"], ["b4", "c2"]),
                     (["c"], ["c3"])]
    # every chain got the labels of its own windows, each step once, chains in sorted key order inside a step
    assert sent == [("a", ["a1"], ["A1"]), ("b", ["b1", "b2", "b3"], ["B1", "B2", "B3"]), ("c", ["c1"], ["C1"]),
                    ("b", ["b4"], ["B4"]), ("c", ["c2"], ["C2"]), ("c", ["c3"], ["C3"])]
    assert chains.returned == {"a": [7, 8], "b": "b", "c": "c", "d": "d"}
    assert not chains and chains.pending() == ([], []) and chains.live() == []


def test_no_chain_and_only_finished_chains():
    assert not Lockstep({}) and Lockstep({}).returned == {}
    done = Lockstep({1: toy(1, [], []), 0: toy(0, [], [])})
    assert not done and done.returned == {0: 0, 1: 1}


def test_an_exception_inside_a_chain_propagates_and_nothing_is_sent_twice():
    sent = []

    def failing():
        labels = yield ["f1"]
        sent.append(("f", ["f1"], labels))
        labels = yield ["f2"]
        sent.append(("f", ["f2"], labels))
        raise RuntimeError("chain f fell over")

    chains = Lockstep({0: toy("e", [["e1"], ["e2"], ["e3"]], sent), 1: failing(), 2: toy("g", [["g1"], ["g2"], ["g3"]], sent)})
    chains.advance(answer(chains.pending()[1]))
    assert chains.pending() == ([0, 1, 2], ["e2", "f2", "g2"])
    with pytest.raises(RuntimeError, match="fell over"):
        chains.advance(answer(chains.pending()[1]))
    # chain e (before f in key order) has its label, f had its own, g was not reached; no (chain, window) pair appears twice
    assert sent == [("e", ["e1"], ["E1"]), ("f", ["f1"], ["F1"]), ("g", ["g1"], ["G1"]), ("e", ["e2"], ["E2"]), ("f", ["f2"], ["F2"])]
    assert len({(name, tuple(windows)) for name, windows, _ in sent}) == len(sent)


def test_a_driver_is_a_chain_of_another_and_chains_move_between_drivers():
    sent = []

    def level(names):                                  # the nesting of the heapsort's level-batched build phase
        inner = Lockstep({n: toy(n, [[n + "1"], [n + "2"]] if n != "y" else [[n + "1"]], sent) for n in names})
        while inner:
            inner.advance((yield inner.pending()[1]))
        return sorted(inner.returned)

    outer = Lockstep({"q1": level("yx"), "q0": toy("p", [["p1"]], sent)})
    assert outer.pending() == (["q0", "q1", "q1"], ["p1", "x1", "y1"])
    outer.advance(["P", "X", "Y"])
    assert outer.pending() == (["q1"], ["x2"]) and outer.returned == {"q0": "p"}
    # the live chain moves to another driver with its pending windows, and back
    other = Lockstep({"q2": toy("r", [["r1"], ["r2"]], sent)})
    other.absorb(outer, ["q1"])
    assert not outer and other.pending() == (["q1", "q2"], ["x2", "r1"])
    outer.absorb(other)
    assert not other and outer.pending() == (["q1", "q2"], ["x2", "r1"])
    outer.advance(["X2", "R1"])
    outer.advance(["R2"])
    assert outer.returned == {"q0": "p", "q1": ["x", "y"], "q2": "r"}
    assert [s for s in sent if s[0] == "x"] == [("x", ["x1"], ["X"]), ("x", ["x2"], ["X2"])]


def test_drive_runs_one_chain_and_returns_its_value():
    sent = []
    assert drive(toy("a", [["a1", "a2"], ["a3"]], sent, result=[7]), answer) == [7]
    assert sent == [("a", ["a1", "a2"], ["A1", "A2"]), ("a", ["a3"], ["A3"])]
    assert drive(toy("d", [], sent), answer) == "d" and len(sent) == 2


# ---- alternate: two groups of chains over two batch slots ------------------------------------------------------------------

class Slots:
    """A recording fake of a runtime with two batch slots.  `refuse`: the numbers (from 1) of the launches that do not fit;
    `fail_launch` / `fail_collect`: the number of the launch that raises / whose collect raises.  Every call is noted in
    `events`; a launch on a slot still in flight, a second collect of a handle and a blocking call while a slot is in flight
    are assertion errors."""

    def __init__(self, refuse=(), fail_launch=None, fail_collect=()):
        self.refuse, self.fail_launch, self.fail_collect = refuse, fail_launch, fail_collect
        self.events, self.busy, self.launched, self.collected, self.n = [], {}, {}, [], 0

    def launch(self, keys, windows, slot):
        self.n += 1
        if self.n == self.fail_launch:
            raise RuntimeError("launch fell over")
        if self.n in self.refuse:
            self.events.append(("refused", slot, keys, windows))
            return None
        assert slot not in self.busy, "launched on a slot that was not collected"
        self.busy[slot] = self.n
        self.launched[self.n] = windows
        self.events.append(("launch", slot, keys, windows))
        return self.n

    def collect(self, keys, handle):
        slot = next(s for s, h in self.busy.items() if h == handle)     # (StopIteration: collected twice, or never launched)
        del self.busy[slot]
        self.collected.append(handle)
        self.events.append(("collect", slot, keys))
        if handle in self.fail_collect:
            raise RuntimeError("collect fell over")
        return answer(self.launched[handle])

    def blocking(self, keys, windows):
        assert not self.busy, "a blocking call while a slot is in flight"
        self.events.append(("blocking", keys, windows))
        return answer(windows)

    def run(self, chains):
        alternate(chains, self.launch, self.collect, self.blocking)


def four(sent):
    """chains 0 and 2 make group 0, chains 1 and 3 group 1; they end after 3, 2, 2 and 1 rounds"""
    return Lockstep({0: toy("a", [["a1"], ["a2"], ["a3"]], sent), 1: toy("b", [["b1", "b2"], ["b3"]], sent),
                     2: toy("c", [["c1"], ["c2", "c3"]], sent), 3: toy("d", [["d1"]], sent)})


def test_alternate_every_launch_fits():
    sent, slots = [], Slots()
    chains = four(sent)
    slots.run(chains)
    assert slots.events == [("launch", 0, [0, 2], ["a1", "c1"]),
                            ("launch", 1, [1, 1, 3], ["b1", "b2", "d1"]),         # ... while slot 0 is uncollected
                            ("collect", 0, [0, 2]),
                            ("launch", 0, [0, 2, 2], ["a2", "c2", "c3"]),           # ... while slot 1 is uncollected
                            ("collect", 1, [1, 1, 3]),
                            ("launch", 1, [1], ["b3"]),                            # chain d has ended
                            ("collect", 0, [0, 2, 2]),
                            ("launch", 0, [0], ["a3"]),                            # chain c has ended
                            ("collect", 1, [1]),                                   # group 1 has ended: slot 1 stays empty
                            ("collect", 0, [0])]
    # every chain got the answers of its own windows, and the chains are back where they came from
    assert sorted(sent) == [("a", ["a1"], ["A1"]), ("a", ["a2"], ["A2"]), ("a", ["a3"], ["A3"]),
                            ("b", ["b1", "b2"], ["B1", "B2"]), ("b", ["b3"], ["B3"]),
                            ("c", ["c1"], ["C1"]), ("c", ["c2", "c3"], ["C2", "C3"]), ("d", ["d1"], ["D1"])]
    assert not chains and chains.returned == {0: "a", 1: "b", 2: "c", 3: "d"} and not slots.busy


def test_alternate_a_launch_that_does_not_fit_takes_the_blocking_call_for_that_round():
    sent, slots = [], Slots(refuse={3})
    chains = four(sent)
    slots.run(chains)
    assert slots.events == [("launch", 0, [0, 2], ["a1", "c1"]),
                            ("launch", 1, [1, 1, 3], ["b1", "b2", "d1"]),
                            ("collect", 0, [0, 2]),
                            ("refused", 0, [0, 2, 2], ["a2", "c2", "c3"]),
                            ("collect", 1, [1, 1, 3]),                             # everything in flight, before ...
                            ("blocking", [0, 2, 2], ["a2", "c2", "c3"]),           # ... exactly this group's round
                            ("launch", 1, [1], ["b3"]),
                            ("launch", 0, [0], ["a3"]),                            # group 0's next round is launched again
                            ("collect", 1, [1]),
                            ("collect", 0, [0])]
    assert len(sent) == 8 and ("c", ["c2", "c3"], ["C2", "C3"]) in sent and chains.returned == {0: "a", 1: "b", 2: "c", 3: "d"}
    # the first launch of all, with nothing in flight, and one of group 1
    sent, slots = [], Slots(refuse={1, 4})
    chains = four(sent)
    slots.run(chains)
    assert slots.events == [("refused", 0, [0, 2], ["a1", "c1"]),
                            ("blocking", [0, 2], ["a1", "c1"]),
                            ("launch", 1, [1, 1, 3], ["b1", "b2", "d1"]),
                            ("launch", 0, [0, 2, 2], ["a2", "c2", "c3"]),
                            ("collect", 1, [1, 1, 3]),
                            ("refused", 1, [1], ["b3"]),
                            ("collect", 0, [0, 2, 2]),
                            ("blocking", [1], ["b3"]),
                            ("launch", 0, [0], ["a3"]),
                            ("collect", 0, [0])]
    assert len(sent) == 8 and chains.returned == {0: "a", 1: "b", 2: "c", 3: "d"}


def failing_chain(sent):
    labels = yield ["f1"]
    sent.append(("f", ["f1"], labels))
    raise RuntimeError("chain f fell over")


@pytest.mark.parametrize("what", ["launch", "collect", "launch_and_drain", "chain"])
def test_alternate_collects_what_is_in_flight_before_an_exception_leaves(what):
    sent = []
    slots, message = {"launch": (Slots(fail_launch=3), "launch fell over"),      # group 0's second launch, slot 1 in flight
                      "collect": (Slots(fail_collect={1}), "collect fell over"),  # group 0's first collect, slot 1 in flight
                      # the launch again, and the drain's own error is swallowed
                      "launch_and_drain": (Slots(fail_launch=3, fail_collect={2}), "launch fell over"),
                      "chain": (Slots(), "chain f fell over")}[what]
    chains = four(sent)
    if what == "chain":                                            # chain f (group 0) raises when its first answer arrives
        chains = Lockstep({0: toy("a", [["a1"], ["a2"]], sent), 1: toy("b", [["b1"], ["b2"]], sent), 2: failing_chain(sent),
                           3: toy("d", [["d1"]], sent)})
    with pytest.raises(RuntimeError, match=message):
        slots.run(chains)
    # every launched handle was collected exactly once, the one in flight after the error
    assert sorted(slots.collected) == sorted(slots.launched) == [1, 2] and not slots.busy
    assert [e[:2] for e in slots.events] == [("launch", 0), ("launch", 1), ("collect", 0), ("collect", 1)]
    assert not any(e[0] == "blocking" for e in slots.events)


def test_alternate_fewer_chains_than_groups_and_chains_of_unequal_length():
    slots = Slots()
    slots.run(Lockstep({}))
    slots.run(Lockstep({0: toy("d", [], [])}))
    assert slots.events == []
    # one live chain: group 1 stays empty, every round on slot 0, collected before the next launch
    sent, slots = [], Slots()
    chains = Lockstep({5: toy("a", [["a1"], ["a2", "a3"]], sent), 2: toy("d", [], sent)})
    slots.run(chains)
    assert slots.events == [("launch", 0, [5], ["a1"]), ("collect", 0, [5]), ("launch", 0, [5, 5], ["a2", "a3"]), ("collect", 0, [5, 5])]
    assert chains.returned == {2: "d", 5: "a"}
    # five chains; group 1 (chains 1 and 3) ends after its first round, group 0 goes on alone, its chains ending one by one
    sent, slots = [], Slots()
    chains = Lockstep({0: toy("a", [["a1"], ["a2"], ["a3"]], sent), 1: toy("b", [["b1"]], sent), 2: toy("c", [["c1"], ["c2"]], sent),
                       3: toy("d", [["d1"]], sent), 4: toy("e", [["e1"]], sent)})
    slots.run(chains)
    assert slots.events == [("launch", 0, [0, 2, 4], ["a1", "c1", "e1"]), ("launch", 1, [1, 3], ["b1", "d1"]),
                            ("collect", 0, [0, 2, 4]), ("launch", 0, [0, 2], ["a2", "c2"]), ("collect", 1, [1, 3]),
                            ("collect", 0, [0, 2]), ("launch", 0, [0], ["a3"]), ("collect", 0, [0])]
    assert chains.returned == {0: "a", 1: "b", 2: "c", 3: "d", 4: "e"} and len(sent) == 8


# ---- the setwise sorts: reference order = level order = rerank_many ---------------------------------------------------------

def docs_of(q, n):
    return [SearchResult(docid=f"q{q}d{i}", score=float(n - i), text=f"t{i}") for i in range(n)]


def label_of(docs, mode):
    """the comparator: the label depends on the window's docids alone.  `garbage` mixes in malformed labels ("?", "Z", "zz": no
    label at all -> the first document wins) and "W", a label beyond every window here (num_child <= 4): the heap keeps the
    parent, the bubblesort raises IndexError as the reference does."""
    if not docs:
        return "A"
    q, idx = int(docs[0].docid[1:].split("d")[0]), [int(d.docid.split("d")[1]) for d in docs]
    rel = [(7 * i + 3 * q) % 11 for i in idx]                   # with ties: the first maximum wins
    h = sum((j + 1) * (i + 1) for j, i in enumerate(idx)) + q
    if mode == "garbage" and h % 3 == 0:
        return ["?", "Z", "zz"][h % 9 // 3]
    if mode == "garbage" and h % 7 == 0:
        return "W"
    return SetwiseLlmRanker.CHARACTERS[max(range(len(docs)), key=lambda j: rel[j])]


class _Labelled(SetwiseLlmRanker):
    """the shipped class with the engine call replaced: compare(), _compare_many() and rerank_many() all end here"""

    def _compare_windows(self, queries, doc_lists):
        for query, docs in zip(queries, doc_lists):
            self.log.append((query, [d.docid for d in docs]))
        self.calls.append(len(doc_lists))
        return [label_of(docs, self.mode) for docs in doc_lists], [len(docs) for docs in doc_lists], [1] * len(doc_lists)


def _ranker(cls, c, k, method, mode, batched):
    rk = cls.__new__(cls)
    rk.num_child, rk.k, rk.method, rk.num_permutation = c, k, method, 1
    rk.model_type, rk.scoring, rk.llm, rk.batch_independent_compares = "t5", "likelihood", None, batched
    rk.mode, rk.log, rk.calls = mode, [], []
    return rk


def _run(rk, q, n):
    """-> (raised, result, caller's list after, compared windows, total_compare) of one rerank of query q"""
    ranking, raised, res = docs_of(q, n), False, []
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            res = rk.rerank(f"query {q}", ranking)
    except IndexError:
        raised = True
    return raised, [(r.docid, r.score, r.text) for r in res], [d.docid for d in ranking], [w for _, w in rk.log], rk.total_compare


def _by_parent(windows):
    """the windows of each sift-down chain in their order: a chain sifts ONE document down, the first of each of its windows"""
    chains = {}
    for w in windows:
        chains.setdefault(w[0] if w else None, []).append(w)
    return chains


@pytest.mark.parametrize("mode", ["clean", "garbage"])
@pytest.mark.parametrize("method", ["heapsort", "bubblesort"])
@pytest.mark.parametrize("c", [2, 3, 4])
def test_reference_order_level_order_and_rerank_many_sort_alike(c, method, mode):
    n_raised = n_level_calls = n_shared_calls = 0
    for n in range(15):
        for k in sorted({1, 3, n}):
            tag = (n, c, k, method, mode)

            def reference(q, m):                                 # one compare at a time, the comparator on the instance
                rk = _ranker(SetwiseLlmRanker, c, k, method, mode, False)
                rk.compare = lambda query, docs, _rk=rk: (_rk.log.append((query, [d.docid for d in docs])),
                                                          setattr(_rk, "total_compare", _rk.total_compare + 1), label_of(docs, mode))[2]
                assert not rk._batched_ok()
                return _run(rk, q, m)

            want = reference(0, n)
            n_raised += want[0]
            assert not want[0] or method == "bubblesort", tag
            # the level-batched single-query path
            rk = _ranker(_Labelled, c, k, method, mode, True)
            assert rk._batched_ok()
            got = _run(rk, 0, n)
            assert got[:3] == want[:3] and got[4] == want[4], tag
            assert sorted(got[3]) == sorted(want[3]) and _by_parent(got[3]) == _by_parent(want[3]), tag
            assert (got[3] == want[3]) or method == "heapsort", tag
            n_level_calls += sum(1 for m in rk.calls if m > 1)
            # four queries of different sizes in lock step
            sizes = [n, 14 - n, (n + 7) % 15, 1]
            wants = [want] + [reference(q, m) for q, m in enumerate(sizes) if q > 0]
            rk = _ranker(_Labelled, c, k, method, mode, True)
            rankings = [docs_of(q, m) for q, m in enumerate(sizes)]
            if any(w[0] for w in wants):
                with pytest.raises(IndexError), contextlib.redirect_stdout(io.StringIO()):
                    rk.rerank_many([(f"query {q}", r) for q, r in enumerate(rankings)])
                continue
            with contextlib.redirect_stdout(io.StringIO()):
                results, counters = rk.rerank_many([(f"query {q}", r) for q, r in enumerate(rankings)])
            n_shared_calls += sum(1 for m in rk.calls if m > 1)
            for q, w in enumerate(wants):
                mine = [w for query, w in rk.log if query == f"query {q}"]
                assert [(r.docid, r.score, r.text) for r in results[q]] == w[1], (tag, q)
                assert [d.docid for d in rankings[q]] == w[2], (tag, q)
                assert sorted(mine) == sorted(w[3]) and _by_parent(mine) == _by_parent(w[3]), (tag, q)
                assert counters[q] == (w[4], sum(len(x) for x in w[3]), w[4]), (tag, q)
    assert n_level_calls > 0 or method == "bubblesort"
    assert n_shared_calls > 0
    assert (n_raised > 0) == (method == "bubblesort" and mode == "garbage")


# ---- the binary pair heaps: PRP = duoT5 reference order = duoT5 level order = duoT5 rerank_many --------------------------------

def pair_docs(q, n):
    return [SearchResult(docid=f"q{q}d{i}", score=float(n - i), text=f"q{q}d{i}") for i in range(n)]     # text = docid


def first_wins(a, b):
    """the comparator on two docids, strict, with ties (five relevance grades): a tie is False, as duoT5's verdict"""
    rel = [(7 * int(d.split("d")[1]) + 3 * int(d[1:].split("d")[0])) % 5 for d in (a, b)]
    return rel[0] > rel[1]


class _Paired(DuoT5LlmRanker):
    """the shipped class with the engine call replaced: compare(), _compare_many() and rerank_many() all end here"""

    def _compare_pairs(self, queries, pairs):
        self.log.extend(zip(queries, pairs))
        self.calls.append(len(pairs))
        return [first_wins(a, b) for a, b in pairs], [len(a) + len(b) for a, b in pairs]


def _pair_ranker(cls, k):
    rk = cls.__new__(cls)
    rk.method, rk.k, rk.llm, rk.batch_independent_compares = "heapsort", k, None, True
    rk.log, rk.calls = [], []
    return rk


def _pair_run(rk, q, n):
    """-> (result, compared pairs in order) of one rerank of query q; the caller's list is left as it was"""
    ranking = pair_docs(q, n)
    before = list(ranking)
    res = rk.rerank(f"query {q}", ranking)
    assert ranking == before
    return [(r.docid, r.score, r.text) for r in res], [pair for _, pair in rk.log]


def test_prp_duot5_reference_order_level_order_and_rerank_many_sort_alike(monkeypatch):
    real, trace = pairwise.sift, {}

    def traced(arr, n, i):                                   # the pairs of each sift-down chain (query, n, i), in its own order
        mine = trace.setdefault((arr[0].docid.split("d")[0], n, i), []) if arr else []
        return drive_through(real(arr, n, i), mine)

    def drive_through(chain, mine):
        verdicts = None
        while True:
            try:
                pairs = chain.send(verdicts)
            except StopIteration:
                return
            mine.extend((a.docid, b.docid) for a, b in pairs)
            verdicts = yield pairs

    monkeypatch.setattr(pairwise, "sift", traced)

    def traced_run(run):
        trace.clear()
        out = run()
        return out, {key: pairs for key, pairs in trace.items() if pairs}

    n_level_calls = n_shared_calls = n_ties = 0
    for n in range(15):
        for k in sorted({1, 3, n}):
            tag = (n, k)

            def prp(q, m):                                   # PairwiseLlmRanker's heapsort, the comparator behind _first_wins
                rk = _pair_ranker(PairwiseLlmRanker, k)
                rk._first_wins = lambda query, a, b, _rk=rk: (_rk.log.append((query, (a, b))), first_wins(a, b))[1]
                return _pair_run(rk, q, m)

            def reference(q, m):                             # duoT5, one compare at a time, the comparator on the instance
                rk = _pair_ranker(DuoT5LlmRanker, k)
                rk.compare = lambda query, docs, _rk=rk: (_rk.log.append((query, tuple(docs))),
                                                          setattr(_rk, "total_compare", _rk.total_compare + 1), first_wins(*docs))[2]
                assert not rk._batched_ok()
                return _pair_run(rk, q, m) + (rk.total_compare,)

            want, want_chains = traced_run(lambda: reference(0, n))
            n_ties += sum(1 for a, b in want[1] if not first_wins(a, b) and not first_wins(b, a))
            got, got_chains = traced_run(lambda: prp(0, n))
            assert got == want[:2] and got_chains == want_chains, tag          # PRP's order IS duoT5's reference order
            # the level-batched single-query path
            rk = _pair_ranker(_Paired, k)
            assert rk._batched_ok()
            got, got_chains = traced_run(lambda: _pair_run(rk, 0, n))
            assert got[0] == want[0] and sorted(got[1]) == sorted(want[1]) and got_chains == want_chains, tag
            assert (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens) == (want[2], sum(len(a) + len(b) for a, b in want[1]), 0), tag
            n_level_calls += sum(1 for m in rk.calls if m > 1)
            # four queries of different sizes in lock step
            sizes = [n, 14 - n, (n + 7) % 15, 1]
            wants, wants_chains = traced_run(lambda: [want] + [reference(q, m) for q, m in enumerate(sizes) if q > 0])
            wants_chains.update(want_chains)
            rk = _pair_ranker(_Paired, k)
            rankings = [pair_docs(q, m) for q, m in enumerate(sizes)]
            before = [list(r) for r in rankings]
            (results, counters), got_chains = traced_run(lambda: rk.rerank_many([(f"query {q}", r) for q, r in enumerate(rankings)]))
            assert rankings == before and got_chains == wants_chains, tag
            n_shared_calls += sum(1 for m in rk.calls if m > 1)
            for q, w in enumerate(wants):
                mine = [pair for query, pair in rk.log if query == f"query {q}"]
                assert [(r.docid, r.score, r.text) for r in results[q]] == w[0], (tag, q)
                assert sorted(mine) == sorted(w[1]), (tag, q)
                assert counters[q] == (w[2], sum(len(a) + len(b) for a, b in w[1]), 0), (tag, q)
    assert n_level_calls > 0 and n_shared_calls > 0 and n_ties > 0
