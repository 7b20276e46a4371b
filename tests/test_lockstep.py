"""The lock-step driver (llmrankers/_lockstep.py) on toy chains, and the setwise sorts through all of their drivers.

CPU only, no model and no runtime: the comparator is a function of the window's docids, so a label does not depend on the order
in which the windows are compared and the three ways to run a sort - the reference's one-by-one order (the one
tests/golden/sort_traces.json ties to the reference, test_host_logic.py), the level-batched build phase, and rerank_many over
several queries - can be held against each other compare by compare."""
import contextlib
import io

import pytest

from llmrankers._lockstep import Lockstep
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
