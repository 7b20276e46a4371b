"""The T5 entry points against each other on ONE engine.  They share a slot's decoder index buffers (decoder ids, last rows,
output ids, row labels / offsets / sequences, tree keys / positions) and the host-side record of what those buffers hold, which
lets a repeated call skip its uploads.  A writer that leaves that record stale makes a LATER call of another entry point score
against the wrong ids - silently.  So: every writer directly after every other writer and after itself, every result bit for
bit what the same call gives as the first call of a fresh engine."""
import numpy as np
import pytest

from _entry_util import _bytes, _each_after_each
from conftest import load_state

pytestmark = pytest.mark.gpu


def _engine(dims, state):
    from llmrankers._engine import RkEngine
    return RkEngine(dims, device=0, max_tokens=4096, max_seqs=64, max_dec_len=40).load_state(state.items())


def _staged(eng, seqs, prefix, out_ids, slot):
    eng.stage(seqs, slot)
    eng.score_staged(prefix, out_ids, slot)
    return eng.read_scores(slot)


@pytest.mark.parametrize("ckpt", ["ckpt_gated_untied", "ckpt_relu_tied"])
def test_every_entry_point_after_every_other_on_one_engine_equals_a_fresh_engine(ckpt_dirs, ckpt):
    from llmrankers import _synth
    dims, state = load_state(ckpt_dirs[ckpt])
    batch = {k: _synth.synth_token_batch(n, 3, 120, dims.vocab, seed=70 + k) for k, n in enumerate((6, 4, 5, 7, 3))}
    rng = np.random.default_rng(17)
    qlm_labels = rng.integers(2, dims.vocab, size=6).tolist()                                   # the class 5..16
    many_labels = [rng.integers(2, dims.vocab, size=n).tolist() for n in (1, 3, 7, 20, 2, 1, 9)]  # four classes in one call
    g2_prefix = [0, 17]
    probe = _engine(dims, state)
    firsts = sorted(set(int(t) for t in probe.greedy(batch[2], g2_prefix, 2)[0][:, 0]))
    probe.close()
    hit = firsts + [t for t in (3, 4) if t not in firsts]
    miss = [t for t in range(5, 12) if t not in firsts][:3]
    assert set(firsts) <= set(hit) and miss and not set(firsts) & set(miss)
    calls = [
        ("score, slot 0", lambda e: _staged(e, batch[0], [0, 11], [10, 20, 30], 0)),
        ("score, slot 1", lambda e: _staged(e, batch[1], [0], [5, 6], 1)),
        ("qlm", lambda e: e.qlm(batch[0], qlm_labels)),
        ("qlm_many", lambda e: e.qlm_many(batch[3], many_labels)),
        ("greedy", lambda e: e.greedy(batch[4], [0], 3)),
        ("greedy2, hit", lambda e: e.greedy(batch[2], g2_prefix, 2, candidates=hit)),
        ("greedy2, miss", lambda e: e.greedy(batch[2], g2_prefix, 2, candidates=miss)),
        ("generate", lambda e: e.generate(batch[1], [0, 23], 4)),
    ]
    want = []
    for name, call in calls:
        fresh = _engine(dims, state)
        want.append(_bytes(call(fresh)))
        fresh.close()
    order = _each_after_each(len(calls))
    assert {(a, b) for a, b in zip(order, order[1:])} == {(a, b) for a in range(len(calls)) for b in range(len(calls))}
    eng = _engine(dims, state)
    try:
        for step, k in enumerate(order):
            got = _bytes(calls[k][1](eng))
            before = calls[order[step - 1]][0] if step else "nothing"
            assert got == want[k], f"call {step}: {calls[k][0]} directly after {before} differs from the fresh engine's"
    finally:
        eng.close()
