"""The Llama entry points against each other on ONE engine: the twin of test_gpu_entry_sequence.py.  rk_llama_greedy1,
rk_llama_last_logits, rk_llama_generate and the session calls share slot 0's prefill buffers, the K / V cache, the attention
partials and the int block (lkv / lpart / lints), the arg-max buffers and the decode ring; the grown ones are freed and
reallocated when a call needs more, and a cached step graph holds their addresses.  So: every call directly after every other
call and after itself, every result bit for bit what the same call gives as the first call of a fresh engine.  Over the 65 calls
buffers move both before and after graphs were captured.  Nothing here looks at counters; the default engine only."""
import dataclasses

import numpy as np
import pytest

from _entry_util import _bytes, _each_after_each
from _graph_util import LLAMA_CKPTS, _session_script, _tokens, _unused_id, llama_checkpoint

pytestmark = pytest.mark.gpu
WINDOW = 64


def _engine(dims, state):
    from llmrankers._engine import RkLlamaEngine
    return RkLlamaEngine(dims, device=0, max_tokens=1024, max_seqs=16).load_state(state.items())


@pytest.fixture(scope="module", params=LLAMA_CKPTS + ["toy-mistral"])
def model(request, ckpt_dirs, tmp_path_factory):
    """(dims, state): the toy Llama (128-wide heads), the toy Qwen2 (64-wide heads, biases), and test_gpu_mistral.py's toy with a
    window of 64 keys (generated weights: that file's seed)"""
    if request.param in LLAMA_CKPTS:
        return llama_checkpoint(request.param, ckpt_dirs, tmp_path_factory.mktemp("llama_entry_sequence"))
    from llmrankers import _synth
    dims = dataclasses.replace(_synth.NAMED_DIMS[request.param], sliding_window=WINDOW)
    return dims, _synth.synth_state_dict(dims, seed=929)


def _refill_script(prompts, eos, pad):
    """a session of (4, 64, 6): three prompts admitted, slot 3's finishes AT its admit (its first token is the eos id), so the first
    run steps nothing; the slot is read and refilled with the fourth prompt while the others decode -> the whole log"""
    def call(eng):
        log = []
        with eng.session(4, 64, 6, [eos], pad) as s:
            s.admit([prompts[0], prompts[1], prompts[2]], [0, 1, 3], [6, 2, 4])
            fin, steps = s.run()
            assert steps == 0 and fin == [3], f"slot 3 did not finish at its admit ({fin}, {steps} steps): the inputs need changing"
            log.append(np.asarray([steps] + fin, dtype=np.int32))
            log.append(np.asarray([3] + [int(t) for t in s.read(3)], dtype=np.int32))
            s.admit([prompts[3]], [3], [3])
            while s.busy:
                fin, steps = s.run()
                log.append(np.asarray([steps] + fin, dtype=np.int32))
                if steps:
                    log.append(eng.debug_read("llama_last", 4 * eng.dims.hidden))
                for slot in fin:
                    log.append(np.asarray([slot] + [int(t) for t in s.read(slot)], dtype=np.int32))
        return tuple(log)
    return call


def test_every_llama_entry_point_after_every_other_on_one_engine_equals_a_fresh_engine(model):
    dims, state = model
    v = dims.vocab
    five, three, six = _tokens((33, 80, 7, 1, 64), v, 1300), _tokens((40, 23, 9), v, 1301), _tokens((12, 65, 3, 90, 64, 31), v, 1302)
    two, cut = _tokens((80, 17), v, 1303), _tokens((40, 23, 9), v, 1304)        # 80 and 90 tokens: longer than the Mistral toy's window
    sess1, sess2 = _tokens((30, 12, 5), v, 1305), _tokens((20, 9, 14, 27), v, 1306)
    probe = _engine(dims, state)
    free = probe.generate(five, 9, [], 0)[0]
    eos5 = [int(free[0, 2]), _unused_id([free], v)]                             # row 0 ends at column 2 at the latest, then pads
    firsts = [int(t) for t in probe.greedy1(sess2[:3])]
    probe.close()
    k = next((i for i in range(3) if firsts.count(firsts[i]) == 1), None)        # the prompt whose first token no other prompt emits ...
    assert k is not None, f"the session's first three prompts all share their first token ({firsts}): the inputs need changing"
    sess2[k], sess2[2] = sess2[2], sess2[k]                                      # ... goes to slot 3, and that token is the eos id
    eos_s = firsts[k]
    calls = [
        ("greedy1, 5 prompts", lambda e: e.greedy1(five)),
        ("last_logits, 3 x 4", lambda e: e.last_logits(three, [7, 100, 3, 41])),
        ("last_logits, 6 x 64", lambda e: e.last_logits(six, list(range(v - 64, v)))),
        ("generate, 2 prompts", lambda e: e.generate(two, 4, [], 0)),
        ("generate, 5 prompts, eos, pad", lambda e: e.generate(five, 9, eos5, 5)),
        ("generate, max_total", lambda e: e.generate(cut, 6, [], 0, max_total=43)),
        ("session (3, 96, 8)", lambda e: tuple(_session_script(sess1, [], 0)(e))),
        ("session (4, 64, 6), eos", _refill_script(sess2, eos_s, 7)),
    ]
    want = []
    for name, call in calls:
        fresh = _engine(dims, state)
        want.append(_bytes(call(fresh)))
        fresh.close()
    order = _each_after_each(len(calls))
    assert len(order) == 65 and {(a, b) for a, b in zip(order, order[1:])} == {(a, b) for a in range(len(calls)) for b in range(len(calls))}
    eng = _engine(dims, state)
    try:
        for step, k in enumerate(order):
            got = _bytes(calls[k][1](eng))
            before = calls[order[step - 1]][0] if step else "nothing"
            assert got == want[k], f"call {step}: {calls[k][0]} directly after {before} differs from the fresh engine's"
    finally:
        eng.close()
