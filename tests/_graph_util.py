"""What the graph tests share (test_gpu_graph_replay.py, test_gpu_graph_moves.py): the G / E engine pair - G a default engine, E
one created for dec_graph = 0, the reference - the calls as closures `call(engine) -> outputs`, the bit-for-bit comparison and the
rk_debug_graph_stats bookkeeping around every step."""
import json
import os

import numpy as np

from conftest import GOLD, load_state

COUNTERS = ("n_keys", "n_ready", "eager", "captures", "replays", "failed", "evictions")
# encoder tokens per sequence.  A / B / C share ceil(longest / 64) = 2 chunks (the key of the query-side chains) and the longest
# sequence 128 is NOT in B (127): the materialised K / V chains, whose key holds the longest itself, use the M sets.
LEN_A = (70, 100, 65, 128, 90)
LEN_B = (3, 127, 64, 65, 1)                     # other T, shortest, longest row; a one-token sequence
LEN_C = (10, 66, 64, 2, 128)                    # the longest row last
LEN_MA, LEN_MB = (70, 100, 65, 128, 90), (128, 5, 64, 1, 33)
# rows above ATTX_MAXK = 192 keys go to the staged kernel, the others to the matrix-core kernel: rows 0 and 2 in A, row 1 in B
LEN_LA, LEN_LB = (200, 30, 193, 64, 100), (1, 200, 192, 3, 77)
DEC17_A = [0] + [5 + 3 * i for i in range(16)]
DEC17_B = [0] + [9 + 5 * i for i in range(16)]


def _tokens(lens, vocab, seed):
    rs = np.random.RandomState(seed)
    out = []
    for n in lens:
        t = rs.randint(3, vocab - 28, size=n).astype(np.int32)
        t[-1] = 1
        out.append(t)
    return out


def _delta(eng, before):
    now = eng.graph_stats()
    return {k: now[k] - before[k] for k in COUNTERS}


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype.kind == "f":
            g, w = g.view(np.uint32), w.view(np.uint32)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: output {i}")


def _differ(a, b):
    return any(np.asarray(x).shape != np.asarray(y).shape or not np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _eager(E, call):
    """The reference: `call` on the engine without graphs -> (its outputs, the number of chains it launched).  E never holds a key."""
    before = E.graph_stats()
    out = call(E)
    d = _delta(E, before)
    assert d == dict(d, n_keys=0, n_ready=0, captures=0, replays=0, failed=0, evictions=0) and E.graph_stats()["n_keys"] == 0, d
    return out, d["eager"]


def _step(G, call, want, what, **expect):
    """`call` on G: outputs bit for bit `want`, and the counters moved by exactly `expect` (everything unnamed: not at all)."""
    before = G.graph_stats()
    got = call(G)
    d = _delta(G, before)
    exp = dict.fromkeys(COUNTERS, 0)
    exp.update(expect)
    assert d == exp, f"{what}: counters moved by {d}, expected {exp}"
    _same(got, want, what)
    assert G.graph_stats()["failed"] == 0, what


def _prime(G, call, want, chains, keys, what):
    """Three calls: over them every one of the call's `keys` keys runs eagerly once, is captured once, and replays from then on
    (`chains` chains per call: a generate call meets its one key `chains` times, a greedy call `chains` keys once each)."""
    before = G.graph_stats()
    for i in range(3):
        _same(call(G), want, f"{what}: priming call {i}")
    d = _delta(G, before)
    exp = dict(n_keys=keys, n_ready=keys, eager=keys, captures=keys, replays=3 * chains - 2 * keys, failed=0, evictions=0)
    assert d == exp, f"{what}: priming moved the counters by {d}, expected {exp}"
    assert G.graph_stats()["failed"] == 0, what


def _report(G, since, what):
    """one line per test for the record in DESIGN.md section 4: what the test's calls did to G's counters"""
    d = _delta(G, since)
    print(f"[graph_stats] {what}: keys +{d['n_keys']}, eager {d['eager']}, captures {d['captures']}, replays {d['replays']}, "
          f"failed {d['failed']}, evictions {d['evictions']}")


def t5_checkpoint(ckpt_dirs):
    """(dims, state) of the committed gated / untied toy T5 checkpoint"""
    return load_state(ckpt_dirs["ckpt_gated_untied"])


def t5_engine(dims, state, graphs=True):
    """a default engine (G), or with graphs=False one created for dec_graph = 0 (E, the reference)"""
    from llmrankers._engine import RkEngine
    eng = RkEngine(dims, device=0, max_tokens=4096, max_seqs=64, max_dec_len=40).load_state(state.items())
    if not graphs:
        eng.set_option("dec_graph", 0)
    return eng


LLAMA_CKPTS = ["ckpt_llama", "ckpt_qwen2_hd64"]


def llama_checkpoint(name, ckpt_dirs, tmp_dir):
    """(dims, state) of the committed toy Llama (128-wide heads) or of the toy Qwen2 (64-wide heads, q / k / v biases) written
    into tmp_dir from its committed spec"""
    from safetensors.numpy import load_file
    from llmrankers import _synth
    if name == "ckpt_llama":
        return load_state(ckpt_dirs["ckpt_llama"])
    with open(os.path.join(GOLD, "llama_hd64_ckpts.json")) as f:
        spec = json.load(f)[name]
    path = str(tmp_dir / name)
    _synth.write_checkpoint(path, spec, os.path.join(GOLD, spec["tokenizer"]))
    assert _synth.checkpoint_sha256(path) == spec["sha256"], name
    with open(os.path.join(path, "config.json")) as f:
        dims = _synth.LlamaDims.from_hf_config(json.load(f))
    state = load_file(os.path.join(path, "model.safetensors"))
    assert dims.head_dim == 64 and dims.qkv_bias
    return dims, state


def llama_engine(dims, state, graphs=True):
    from llmrankers._engine import RkLlamaEngine
    eng = RkLlamaEngine(dims, device=0, max_tokens=1024, max_seqs=16).load_state(state.items())
    if not graphs:
        eng.set_option("dec_graph", 0)
    return eng


def _llama_pair(dims, state):
    return llama_engine(dims, state), llama_engine(dims, state, graphs=False)


def _score(seqs, prefix, ids):
    """blocking score on slot 0 -> (scores, the decoder's hidden rows [n_seq * dec_len, d_model])"""
    def call(eng):
        s = eng.score(seqs, prefix, ids)
        return s, eng.debug_read("dec_hidden", len(seqs) * len(prefix) * eng.dims.d_model)
    return call


def _score_slot1(seqs, prefix, ids):
    """the same batch through slot 1's staged calls -> (scores,)  (rk_debug_read reads slot 0's buffers only)"""
    def call(eng):
        eng.stage(seqs, slot=1)
        eng.score_staged(prefix, ids, slot=1)
        return (eng.read_scores(1),)
    return call


def _compare(seqs, start, false_id, true_id):
    def call(eng):
        logits, p_true, wins = eng.compare_pairs(seqs, start, false_id, true_id)
        return logits, p_true, wins, eng.debug_read("dec_hidden", len(seqs) * eng.dims.d_model)
    return call


def _unused_id(outs, vocab):
    used = set(int(t) for o in outs for t in np.asarray(o).reshape(-1))
    return next(i for i in range(vocab - 1, 2, -1) if i not in used)


def _greedy(seqs, prefix, max_new, eos, pad, rows_per_seq, candidates=None):
    def call(eng):
        toks, steps = eng.greedy(seqs, prefix, max_new, eos_id=eos, pad_id=pad, candidates=candidates)
        return toks, np.int32(steps), eng.debug_read("dec_hidden", len(seqs) * rows_per_seq * eng.dims.d_model)
    return call


def _generate(seqs, prefix, max_new, eos, pad):
    def call(eng):
        toks, steps = eng.generate(seqs, prefix, max_new, eos_id=eos, pad_id=pad)
        return toks, np.int32(steps), eng.debug_read("dec_hidden", len(seqs) * eng.dims.d_model)
    return call


def _llama_generate(seqs, max_new, eos, pad, max_total=0):
    def call(eng):
        toks, steps = eng.generate(seqs, max_new, eos, pad, max_total=max_total)
        return toks, np.int32(steps), eng.debug_read("llama_last", len(seqs) * eng.dims.hidden)
    return call


def _session_script(prompts, eos, pad, n_slots=3, max_len=96, cap=8):
    """admit two prompts, run, and admit the third into the free slot while another slot is still decoding; run / read until the
    session is empty -> the whole log: per run the finished slots, the steps and (behind a run that stepped) the step's final rows,
    per read the slot's tokens - so the finish order is part of what is compared"""
    def call(eng):
        log, late = [], True
        with eng.session(n_slots, max_len, cap, eos, pad) as s:
            s.admit([prompts[0], prompts[1]], [0, 2], [8, 3])
            while s.busy:
                fin, steps = s.run()
                log.append(np.asarray([steps] + fin, dtype=np.int32))
                if steps:
                    log.append(eng.debug_read("llama_last", n_slots * eng.dims.hidden))
                for slot in fin:
                    log.append(np.asarray([slot] + [int(t) for t in s.read(slot)], dtype=np.int32))
                    assert slot != 0 or not late, "slot 0 finished before the third prompt was admitted: the inputs need changing"
                if late and fin:
                    s.admit([prompts[2]], [1], [5])
                    late = False
            assert not late
        return log
    return call
