"""Llama / Qwen2 checkpoints with 64-wide heads on the HIP engine (csrc/llama_kernels_hd64.h), end to end: last logits and the
cached step against the fp32 oracle at every tile and chunk count, generated tokens against the oracle and the greedy1 re-prefill
loop, batch independence, the decoding session, the all-zero bias, the refusal of other widths, a 128-wide engine beside a 64-wide
one, and one case at Llama-3.2-1B widths.  Three toy shapes at synth seed 929: 8 query heads on 2 kv heads (G = 4), Qwen2's 7 on 1
with q / k / v biases (G = 7), and 3 on 3 (G = 1, q width 192).

The module stops at the first device error: nothing more is started on a device that has faulted."""
import dataclasses

import numpy as np
import pytest

from llmrankers import _synth
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu
FLOOR = 5e-3              # fp16 noise floor of the toy scale (test_gpu_rerank.py)
BOUND = 4e-3              # x logit scale: what the 128-wide prefill and step are held to (test_gpu_llama_listwise.py)
CHUNK = 128               # attn_dec_cached_kernel<64>: keys per workgroup (csrc/llama_kernels.h: LDC_CHUNK)
ERR_INVALID, ERR_HIP = -1, -3
TOYS = ["toy-llama-hd64", "toy-qwen2-hd64", "toy-llama-mha-hd64"]


def _guard(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{getattr(fn, '__name__', fn)}: {err}", returncode=3)
        raise


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 32768)
    kw.setdefault("max_seqs", 128)
    return _guard(RkLlamaEngine(dims, device=0, **kw).load_state, state.items())


def _oracle(dims, state):
    from oracle.llama_numpy import LlamaOracle
    from _qwen2_ref import Qwen2Oracle
    return (Qwen2Oracle if dims.qkv_bias else LlamaOracle)(dims, state)


def _head(dims, state):
    return np.asarray(state["model.embed_tokens.weight"] if dims.tied_head else state["lm_head.weight"], dtype=np.float32)


def _all_logits(eng, seqs, vocab):
    return np.concatenate([_guard(eng.last_logits, seqs, list(range(v0, v0 + 64))) for v0 in range(0, vocab, 64)], axis=1)


@pytest.fixture(scope="module", params=TOYS)
def toy(request):
    """dims, state, oracle, head, the oracle's greedy rows of the five token-test prompts - computed once, never modified"""
    from _llama_gen_stub import oracle_greedy
    dims = _synth.NAMED_DIMS[request.param]
    state = _synth.synth_state_dict(dims, seed=929)
    orc = _oracle(dims, state)
    seqs = _synth.synth_token_batch(5, 8, 120, dims.vocab, seed=7)
    ref = [oracle_greedy(orc, s, 20) for s in seqs]
    return dims, state, orc, _head(dims, state), seqs, ref


def test_dims():
    a, q, m = (_synth.NAMED_DIMS[n] for n in TOYS)
    assert (a.n_heads, a.n_kv_heads, a.head_dim, a.n_heads * a.head_dim, a.hidden) == (8, 2, 64, 512, 256)
    assert (q.n_heads, q.n_kv_heads, q.head_dim, q.qkv_bias, q.tied_head) == (7, 1, 64, True, True)
    assert (m.n_heads, m.n_kv_heads, m.head_dim, m.n_heads * m.head_dim) == (3, 3, 64, 192)


def test_last_logits_vs_oracle_at_every_tile_edge(toy):
    """prefixes of one 700-token sequence: 1, 2, 3, both sides of every multiple of 32 up to 128 and of every multiple of 128, and
    700; every vocabulary row of the prefill's last position against the oracle"""
    dims, state, orc, _, _, _ = toy
    base = _synth.synth_token_batch(1, 700, 700, dims.vocab, seed=17)[0]
    lens = sorted(set([1, 2, 3, 700] + [e + d for e in (32, 64, 96, 128, 256, 384, 512, 640) for d in (-1, 0, 1)]))
    seqs = [base[:n] for n in lens]
    eng = _engine(dims, state)
    got = _all_logits(eng, seqs, dims.vocab)
    eng.close()
    want = orc.last_logits(seqs)
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"max |logit - oracle| = {err:.3e} at scale {scale:.2f} (bound {BOUND * scale:.3e})")
    assert got.shape == want.shape
    assert err < BOUND * scale, (err, scale)


def test_step_kernel_vs_oracle_at_every_chunk_count(toy):
    """the lengths and the loop of test_gpu_llama_listwise.py::test_step_kernel_vs_oracle_at_every_chunk_count: max_new 1 .. 6, no
    EOS; the final-normed rows the LAST step's head read, times head^T, against the oracle's logits of prompt + generated tokens"""
    dims, state, orc, head, _, _ = toy
    base = _synth.synth_token_batch(1, 700, 700, dims.vocab, seed=17)[0]
    lens = sorted(set([1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97] + [k * CHUNK + d for k in range(1, 6) for d in (-6, -5, -2, -1, 0, 1)]
                      + [694, 700] + list(range(7, 700, 97))))
    seqs = [base[:n] for n in lens]
    eng = _engine(dims, state)
    worst = 0.0
    for max_new in range(1, 7):
        toks, steps = _guard(eng.generate, seqs, max_new, [], 0)
        assert steps == max_new and toks.shape == (len(seqs), max_new)
        last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), dims.hidden)
        got = last @ head.T
        want = orc.last_logits([list(s) + [int(t) for t in toks[b, :max_new - 1]] for b, s in enumerate(seqs)])
        scale = float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        worst = max(worst, err / scale)
        print(f"max_new {max_new}: max |logit - oracle| = {err:.3e} at scale {scale:.2f}")
        assert err < BOUND * scale, (max_new, err, scale)
    print(f"worst relative error {worst:.3e}")
    eng.close()


def test_tokens_vs_oracle_greedy1_and_the_reprefill_loop(toy):
    """5 prompts, 20 new tokens: generated tokens == the oracle's up to the first step whose ORACLE margin is under the floor;
    column 0 == greedy1; == a greedy1 re-prefill loop over the checked steps.  The oracle alone clears 83 (8 / 2 heads), 100 (7 / 1)
    and 100 (3 / 3) of the 100 steps."""
    dims, state, _, _, seqs, ref = toy
    eng = _engine(dims, state)
    gen, steps = _guard(eng.generate, seqs, 20, [], 0)
    assert steps == 20
    np.testing.assert_array_equal(gen[:, 0], _guard(eng.greedy1, seqs))
    checked = 0
    for b, (toks, margins) in enumerate(ref):
        low = next((i for i, m in enumerate(margins) if m < FLOOR), len(margins))
        assert list(gen[b, :low]) == toks[:low], (b, low)
        cur = list(seqs[b])
        for t in range(low):
            assert int(_guard(eng.greedy1, [cur])[0]) == int(gen[b, t]), (b, t)
            cur.append(int(gen[b, t]))
        checked += low
    eng.close()
    print(f"{checked} of 100 steps checked")
    assert checked >= 60, checked


def test_batch_and_reversed_batch_give_the_same_bits(toy):
    dims, state, _, _, _, _ = toy
    rs = np.random.RandomState(23)
    seqs = [rs.randint(3, dims.vocab - 28, size=n).astype(np.int32) for n in (3, 300, 129, 47, 256, 64, 190, 513)]
    eng = _engine(dims, state)
    batch, _ = _guard(eng.generate, seqs, 6, [], 0)
    last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), -1).copy()
    rev, _ = _guard(eng.generate, seqs[::-1], 6, [], 0)
    last_rev = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), -1)
    eng.close()
    np.testing.assert_array_equal(rev[::-1], batch)
    assert np.array_equal(last_rev[::-1].view(np.uint32), last.view(np.uint32))


def test_session_with_staggered_admits_equals_generate_alone(toy):
    """ten prompts through a session of 4 slots, free slots refilled while the others decode: every prompt's tokens are the tokens
    rk_llama_generate gives it alone"""
    dims, state, _, _, _, _ = toy
    lens = (1, 2, 63, 64, 65, 127, 128, 129, 255, 300)
    max_new = tuple((40, 5, 2, 1)[i % 4] for i in range(len(lens)))
    base = _synth.synth_token_batch(1, 300, 300, dims.vocab, seed=17)[0]
    prompts = [list(base[:n]) for n in lens]
    eng = _engine(dims, state, max_tokens=4096, max_seqs=16)
    want = []
    for p, m in zip(prompts, max_new):
        toks, steps = _guard(eng.generate, [p], m, [], 0)
        want.append([int(t) for t in toks[0, :steps]])
    got, refills, nxt = {}, 0, 0
    with eng.session(4, 384, 40, [], 0) as s:
        owner = {}
        while nxt < len(prompts) or s.busy:
            free = s.free_slots()
            take = list(range(nxt, min(nxt + len(free), len(prompts))))
            if take:
                refills += bool(s.busy)
                slots = free[:len(take)]
                _guard(s.admit, [prompts[r] for r in take], slots, [max_new[r] for r in take])
                owner.update(zip(slots, take))
                nxt += len(take)
            finished, _ = _guard(s.run)
            assert finished, "a run with busy slots must end with a finish"
            for slot in finished:
                got[owner.pop(slot)] = [int(t) for t in s.read(slot)]
    eng.close()
    assert refills >= 2, refills
    for r, w in enumerate(want):
        assert got[r] == w, (r, lens[r], got[r], w)


def test_zero_bias_equals_the_bias_free_engine_bit_for_bit():
    """the Qwen2 toy's weights without biases: the switch on with all-zero bias vectors == the switch off, in last_logits bytes and
    in generated tokens (rope64_pairs forms both the same way: by construction, not by a compiler's choice)"""
    off = dataclasses.replace(_synth.TOY_QWEN2_HD64, qkv_bias=False)
    on = dataclasses.replace(off, qkv_bias=True)
    state = dict(_synth.synth_state_dict(off, seed=929))
    assert not any(k.endswith(".bias") for k in state)
    zero = dict(state)
    for n, shape, _, _ in _synth.llama_tensor_specs(on):
        if n.endswith(".bias"):
            zero[n] = np.zeros(shape, np.float32)
    seqs = _synth.synth_token_batch(5, 2, 270, off.vocab, seed=9)
    ids = list(range(0, off.vocab, off.vocab // 64))
    res = []
    for dims, st in ((off, state), (on, zero)):
        eng = _engine(dims, st, max_tokens=4096, max_seqs=16)
        lg = _guard(eng.last_logits, seqs, ids)
        gen, _ = _guard(eng.generate, seqs, 5, [], 0)
        rows = eng.debug_read("llama_last", len(seqs) * dims.hidden).copy()
        eng.close()
        res.append((lg, gen, rows))
    assert np.array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32))
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][2].view(np.uint32), res[1][2].view(np.uint32))   # the step too: one form for both


def test_other_head_widths_are_refused():
    from llmrankers._engine import RkLlamaEngine
    dims = dataclasses.replace(_synth.TOY_LLAMA_HD64, head_dim=96)
    with pytest.raises(RkError) as ei:
        RkLlamaEngine(dims, device=0, max_tokens=512, max_seqs=4)
    assert ei.value.code == ERR_INVALID and "64" in str(ei.value) and "128" in str(ei.value) and "96" in str(ei.value)


def test_a_128_wide_engine_beside_a_64_wide_one():
    """a 128-wide toy engine created while a 64-wide one lives gives the bytes of a second 128-wide engine created after it closed"""
    d64, d128 = _synth.TOY_LLAMA_HD64, _synth.TOY_LLAMA
    s64, s128 = _synth.synth_state_dict(d64, seed=929), _synth.synth_state_dict(d128, seed=929)
    seqs = _synth.synth_token_batch(4, 3, 200, d128.vocab, seed=31)
    ids = list(range(0, 256, 4))
    e64 = _engine(d64, s64, max_tokens=2048, max_seqs=8)
    e128 = _engine(d128, s128, max_tokens=2048, max_seqs=8)
    _guard(e64.generate, seqs, 3, [], 0)
    a = (_guard(e128.last_logits, seqs, ids), _guard(e128.generate, seqs, 4, [], 0)[0])
    _guard(e64.generate, seqs, 3, [], 0)
    e64.close()
    e128.close()
    e128 = _engine(d128, s128, max_tokens=2048, max_seqs=8)
    b = (_guard(e128.last_logits, seqs, ids), _guard(e128.generate, seqs, 4, [], 0)[0])
    e128.close()
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1], b[1])


def test_llama_32_1b_widths_vs_oracle():
    """Llama-3.2-1B widths (32 query heads on 8 kv heads of 64, hidden 2048, tied head, rope type llama3) with two layers, the
    embedding / head rows of 23 label tokens boosted x 6 (test_llama_3_8b_widths_vs_oracle's rule: random heads are too flat for the
    floor of this scale), one 600-token and one 45-token prompt, 8 new tokens: tokens == the oracle's up to the first step whose
    oracle margin is under 0.02 x scale, == the greedy1 re-prefill loop there.  The oracle alone (seed 929, token seeds 700 / 145):
    8 clear steps on either prompt (smallest margin 895 at scale 1490: with a tied head a boosted row leads by its own norm)."""
    from _llama_gen_stub import oracle_greedy
    dims = dataclasses.replace(_synth.LLAMA_32_1B, n_layers=2)
    assert dims.tied_head and dims.rope_scaling is not None and dims.head_dim == 64
    state = _synth.synth_state_dict(dims, seed=929, threads=16)
    ids = np.arange(32, 32 + 23)
    w = state["model.embed_tokens.weight"].copy()
    w[ids] = (w[ids] * np.float32(6.0)).astype(np.float16).astype(np.float32)
    state["model.embed_tokens.weight"] = w
    eng = _engine(dims, state, max_tokens=4096, max_seqs=8)
    seqs = [s for n in (600, 45) for s in _synth.synth_token_batch(1, n, n, dims.vocab, seed=TOKEN_SEED + n)]
    gen, steps = _guard(eng.generate, seqs, 8, [], 0)
    assert steps == 8
    np.testing.assert_array_equal(gen[:, 0], _guard(eng.greedy1, seqs))
    orc = _oracle(dims, state)
    scale = float(np.abs(orc.last_logits(seqs)).max())
    for b, s in enumerate(seqs):
        toks, margins = oracle_greedy(orc, s, 8)
        low = next((i for i, m in enumerate(margins) if m <= 0.02 * scale), len(margins))
        print(f"prompt of {len(s)}: margins {[round(m, 3) for m in margins]}, scale {scale:.2f}, checked {low}")
        assert low >= 1, (b, margins, scale)
        assert list(gen[b, :low]) == toks[:low], (b, low)
        cur = list(s)
        for t in range(low):
            assert int(_guard(eng.greedy1, [cur])[0]) == int(gen[b, t]), (b, t)
            cur.append(int(gen[b, t]))
    np.testing.assert_array_equal(_guard(eng.generate, seqs[::-1], 8, [], 0)[0][::-1], gen)
    eng.close()


# ---- the reference's recorded cases on the 64-wide checkpoints (tools/make_llama_hd64_golden.py) ------------------------------
@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """the recorded cases, and the checkpoints (the adapter) written from their recipes with the sha256 asserted - once"""
    import json
    import os
    from conftest import GOLD
    with open(os.path.join(GOLD, "llama_hd64_cases.json")) as f:
        cases = json.load(f)
    with open(os.path.join(GOLD, "llama_hd64_ckpts.json")) as f:
        specs = json.load(f)
    root = tmp_path_factory.mktemp("llama_hd64_gold")
    paths = {}
    for name, spec in specs.items():
        path = str(root / name)
        if name.startswith("adapter"):
            assert _synth.write_lora_adapter(path, _synth.TOY_QWEN2_HD64, spec) == spec["sha256"]
        else:
            _synth.write_checkpoint(path, spec, os.path.join(GOLD, spec["tokenizer"]))
            assert _synth.checkpoint_sha256(path) == spec["sha256"], name
        paths[name] = path
    return cases, specs, paths


def _by_kind(cases, kind):
    out = [c for c in cases["cases"] if c["kind"] == kind]
    assert out, kind
    for c in out:                                                     # the four-times rule: no committed case is a coin-flip, none is skipped
        assert c["min_margin"] >= 4 * FLOOR == cases["keep"], (kind, c["min_margin"])
    return out


def test_setwise_and_pairwise_reference_cases_on_the_engine(gold):
    """SetwiseLlmRanker (generation; heapsort and bubblesort) and PairwiseLlmRanker (heapsort and bubblesort) through their PUBLIC
    constructors (checkpoint directory -> rk_llama engine with 64-wide heads): every compare in order, ranking, the caller's list,
    counters - the reference's own"""
    import random
    from llmrankers.pairwise import PairwiseLlmRanker
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import SetwiseLlmRanker
    cases, _, paths = gold
    ck = paths["ckpt_llama_hd64"]
    sw, pw = _by_kind(cases, "setwise-llama"), _by_kind(cases, "pairwise-llama")
    assert {c["method"] for c in sw} == {c["method"] for c in pw} == {"heapsort", "bubblesort"}
    for case in sw + pw:
        if case["kind"] == "setwise-llama":
            rk = SetwiseLlmRanker(ck, ck, "cuda", num_child=case["num_child"], k=case["k"], scoring=case["scoring"], method=case["method"],
                                  num_permutation=case["num_permutation"])
            ids_of = lambda docs: [d.docid for d in docs]
        else:
            rk = PairwiseLlmRanker(ck, ck, "cuda", method=case["method"], batch_size=2, k=case["k"])
            ids_of = list
        assert rk.llm.dims.head_dim == 64
        log, orig = [], rk.compare
        rk.compare = lambda q, d, _o=orig, _l=log, _i=ids_of: (_l.append([_i(d)]), _l[-1].append(_guard(_o, q, d)))[1] or _l[-1][1]
        ranking = [SearchResult(docid=d, score=s, text=t) for d, s, t in case["input"]]
        random.seed(929)
        res = rk.rerank(case["query"], ranking)
        tag = (case["kind"], case["method"], case["query"])
        assert log == case["compares"], tag
        assert [[r.docid, r.score] for r in res] == case["result"], tag
        assert [r.docid for r in ranking] == case["caller_list_after"], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
        rk.llm.engine.close()


def test_listwise_reference_cases_on_the_engine(gold):
    from transformers import AutoTokenizer
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.listwise import ListwiseLlmRanker
    from llmrankers.rankers import SearchResult
    cases, _, paths = gold
    ck = paths["ckpt_llama_hd64_listwise"]
    rt = LlamaRuntime(ck, "cuda", max_tokens=16384, max_seqs=16)
    assert rt.dims.head_dim == 64 and rt.generation["eos_token_ids"] == [cases["listwise_model_eos"]]
    tok = AutoTokenizer.from_pretrained(ck)
    tok.use_default_system_prompt = False
    for case in _by_kind(cases, "listwise-llama"):
        rk = ListwiseLlmRanker.from_runtime(rt, tok, window_size=case["window_size"], step_size=case["step_size"], scoring=case["scoring"],
                                            num_repeat=case["num_repeat"])
        outs, real = [], rk.compare
        rk.compare = lambda q, docs: outs.append(_guard(real, q, docs)) or outs[-1]
        ranking = [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]]
        res = rk.rerank(case["query"], ranking)
        tag = case["qid"]
        assert outs == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [d.docid for d in ranking] == [d for d, _ in case["docs"]], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
    rt.engine.close()


def test_rankr1_reference_cases_on_the_engine(gold):
    """the reference's Rank-R1 ranker on the Qwen2 toy with 64-wide heads (7 query heads on one kv head, q / k / v biases, a LoRA
    adapter merged by the loader): every compare's output, ranking, counters"""
    import os
    import random
    from conftest import GOLD
    from transformers import AutoTokenizer
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    cases, specs, paths = gold
    rt = LlamaRuntime(paths["ckpt_qwen2_hd64"], "cuda", max_tokens=4096, max_seqs=16, accept_model_types=("qwen2",), adapter_dir=paths["adapter_qwen2_hd64"])
    assert rt.model_type == "qwen2" and rt.dims.qkv_bias and rt.dims.head_dim == 64 and rt.generation["eos_token_ids"] == [cases["rankr1_model_eos"]]
    tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, specs["ckpt_qwen2_hd64"]["tokenizer"]))    # (its own directory: see test_rankr1_host.py)
    for case in _by_kind(cases, "rankr1-qwen2"):
        rk = RankR1SetwiseLlmRanker.from_runtime(rt, tok, os.path.join(GOLD, "rankr1_prompt.toml"), num_child=case["num_child"], k=case["k"],
                                                 method=case["method"], num_permutation=case["num_permutation"], max_new_tokens=case["max_new_tokens"])
        outs, real = [], rk.compare
        rk.compare = lambda q, docs: outs.append(_guard(real, q, docs)) or outs[-1]
        random.seed(case["random_seed"])
        res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
        tag = case["qid"]
        assert outs == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
    rt.engine.close()


def test_run_py_setwise_on_a_64_wide_checkpoint(gold, tmp_path):
    """run.py ... setwise once on the toy checkpoint: the run file holds the recorded heapsort ranking of that query on top"""
    import contextlib
    import importlib.util
    import io
    import os
    from conftest import REPO
    cases, _, paths = gold
    case = next(c for c in _by_kind(cases, "setwise-llama") if c["method"] == "heapsort")
    spec = importlib.util.spec_from_file_location("rk_run_llama_hd64_gpu", os.path.join(REPO, "run.py"))
    runmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(runmod)
    (tmp_path / "q.tsv").write_text(f"q1\t{case['query']}\n")
    (tmp_path / "d.tsv").write_text("".join(f"{d}\t{t}\n" for d, _, t in case["input"]))
    (tmp_path / "in.trec").write_text("".join(f"q1 Q0 {d} {r + 1} {s} bm25\n" for r, (d, s, _) in enumerate(case["input"])))
    parser, commands = runmod.build_parser()
    save = tmp_path / "out.trec"
    args = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", paths["ckpt_llama_hd64"], "--run_path", str(tmp_path / "in.trec"),
                                                "--save_path", str(save), "--query_file", str(tmp_path / "q.tsv"), "--doc_file", str(tmp_path / "d.tsv"),
                                                "--hits", str(len(case["input"])), "--passage_length", "512", "--query_length", "64",
                                                "setwise", "--num_child", str(case["num_child"]), "--k", str(case["k"]), "--method", "heapsort"])
    runmod.validate(args)
    with contextlib.redirect_stdout(io.StringIO()):
        runmod.main(args)
    rows = [l.split() for l in save.read_text().splitlines()]
    assert len(rows) == len(case["input"]) and sorted(r[2] for r in rows) == sorted(d for d, _, _ in case["input"])
    assert [r[2] for r in rows] == [d for d, _ in case["result"]]


TOKEN_SEED = 100          # chosen on the CPU with the oracle alone: every prompt has at least one clear step
