"""The drafting session's two state kernels alone (llama_session_advance_draft_kernel, draft_lookup_kernel) on an MI355X through
rk_debug_draft_steps - the production launchers in the session's order, every state array a device allocation of its own between
sentinel bands - against tests/_draft_ref.py's DraftMachine: the complete state, array by array, after every launch of fixed scripts
(tests/test_draft_machine_host.py shows what edges they meet and that they tell wrong machines apart).  Integers only: no tolerance."""
import numpy as np
import pytest

import _draft_ref as D
from conftest import load_state
from llmrankers import _synth
from llmrankers._engine import DEBUG_SENTINEL as SENTINEL

pytestmark = pytest.mark.gpu

i32 = np.int32
BAND = 256
RK_ERR_INVALID, RK_ERR_HIP = -1, -3


@pytest.fixture(scope="module")
def llama():
    from llmrankers._engine import RkLlamaEngine
    dims = _synth.TOY_LLAMA
    e = RkLlamaEngine(dims, device=0, max_tokens=256, max_seqs=4).load_state(_synth.synth_state_dict(dims, seed=929).items())
    yield e
    e.close()


@pytest.fixture(scope="module")
def t5(ckpt_dirs):
    from llmrankers._engine import RkEngine
    dims, state = load_state(ckpt_dirs["ckpt_gated_untied"])
    e = RkEngine(dims, device=0, max_tokens=512, max_seqs=4, max_dec_len=4).load_state(state.items())
    yield e
    e.close()


def last_error(eng):
    return (eng.lib.rk_last_error(eng.h) or b"").decode()


def call(eng, n_slots, g1, script, init, max_admit, max_tokens, check=True):
    res = eng.debug_draft_steps(n_slots=n_slots, g1=g1, script=script, state=init, max_admit=max_admit, max_tokens=max_tokens, band=BAND, check=False)
    if res["rc"] == RK_ERR_HIP:
        pytest.exit(f"rk_debug_draft_steps: {last_error(eng)}", returncode=3)   # a fault on the device: nothing more is started on it from this module
    if check:
        assert res["rc"] == 0, last_error(eng)
    return res


def run_script(eng, n_slots, g1, ngram):
    steps, init, states, _, max_admit, max_tokens = D.build_script(n_slots, g1, ngram)
    script = D.pack_script(steps, n_slots, g1, max_admit, max_tokens)
    res = call(eng, n_slots, g1, script, init, max_admit, max_tokens)
    again = call(eng, n_slots, g1, script, init, max_admit, max_tokens)
    for name, a, b in zip(D.ARRAYS, res["all"], again["all"]):
        assert np.array_equal(a, b), f"{name}: a second run gives other bytes"
        assert (a[:, :BAND] == SENTINEL).all() and (a[:, -BAND:] == SENTINEL).all(), f"{name}: a band was written"
    for s, want in enumerate(states):
        for name, a, w in zip(D.ARRAYS, res["all"], want):
            g = np.ascontiguousarray(a[s, BAND:-BAND]).view(i32)
            if not np.array_equal(g, w):
                at = np.flatnonzero(g != w)[:8]
                raise AssertionError(f"n_slots={n_slots} g1={g1} ngram={ngram}: step {s} ({steps[s]['kind']}), {name} differs at {at.tolist()}: "
                                     f"{g[at].tolist()} != {w[at].tolist()}")
    return res


@pytest.mark.parametrize("ngram", D.NGRAMS)
@pytest.mark.parametrize("g1", D.G1S)
@pytest.mark.parametrize("n_slots", D.N_SLOTS)
def test_state_after_every_launch(llama, n_slots, g1, ngram):
    run_script(llama, n_slots, g1, ngram)


def test_a_t5_engine_gives_the_same_bytes(llama, t5):
    a, b = run_script(llama, 3, 4, (1, 3)), run_script(t5, 3, 4, (1, 3))
    assert all(np.array_equal(x, y) for x, y in zip(a["all"], b["all"]))


def _one_admit(slot=0, length=4, max_new=3, off=0):
    return [{"kind": 1, "slots": [slot], "lens": [length], "max_news": [max_new], "prompts": [[5] * max(length, 0)], "argmax": [5]}], off


REFUSED = {
    "len + max_new > max_len": dict(admit=dict(length=D.MAX_LEN - 2, max_new=3)),
    "max_new > cap": dict(admit=dict(max_new=D.CAP + 1)),
    "max_new = 0": dict(admit=dict(max_new=0)),
    "an empty prompt": dict(admit=dict(length=0)),
    "n_eos = 9": dict(st={2: 9}),
    "ngram_min = 0": dict(st={5: 0}),
    "ngram_min > ngram_max": dict(st={5: 4, 6: 3}),
    "ngram_max = 9": dict(st={6: 9}),
    "g1 = 9": dict(g1=9),
    "a slot twice": dict(twice=True),
    "a table beyond the cap": dict(table=D.CAP + 1),
    "a table's slot out of range": dict(table=2, slot=3),
    "an active slot at its max_new": dict(active=True),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_before_any_launch(llama, what):
    """Every extent the two kernels rely on: RK_ERR_INVALID and the state untouched (nothing was allocated, launched or copied back:
    the host buffers still hold the sentinel).  The accepted twin of every case runs first."""
    S, g1 = 3, 4
    for bad in (False, True):
        kw = REFUSED[what] if bad else {}
        m = D.DraftMachine(S, g1, D.MAX_LEN, D.CAP, D.EOS, D.PAD, (1, 3))
        for i, v in kw.get("st", {}).items():
            m.st[i] = v
        if kw.get("active"):
            m.done[1], m.len[1], m.col[1], m.max_new[1], m.hist[1, :8] = 0, 4, 3, 3, 5
        steps, _ = _one_admit(**kw.get("admit", {}))
        if kw.get("twice"):
            steps[0].update(slots=[1, 1], lens=[4, 4], max_news=[3, 3], prompts=[[5] * 4, [6] * 4], argmax=[5, 6])
        if "table" in kw:
            steps.append({"kind": 2, "slot": kw.get("slot", 0), "tokens": [5] * kw["table"]})
        script = D.pack_script(steps, S, g1, 2, D.MAX_LEN)
        res = call(llama, S, kw.get("g1", g1) if bad else g1, script, m.state(), 2, D.MAX_LEN, check=False)
        if not bad:
            assert res["rc"] == 0, (what, last_error(llama))
            continue
        assert res["rc"] == RK_ERR_INVALID, what
        assert all((a == SENTINEL).all() for a in res["all"]), what
