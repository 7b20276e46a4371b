"""The Qwen2 family on the HIP engine (q / k / v projection biases in the prefill's rotary kernel and in the cached decode step, 7
query heads per kv head in one pass over the cache) and RankR1SetwiseLlmRanker end to end: prefill and decode step against the fp32
oracle, outlier bias channels against HF's own fp16 error, batch independence, the bias-free path bit for bit, the contract, the
reference's recorded Rank-R1 cases."""
import dataclasses
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
FLOOR = 5e-3              # fp16 noise floor of the toy scale (test_gpu_rerank.py)
BOUND = 4e-3              # x logit scale: what the bias-free Llama prefill and step are held to (test_gpu_llama_listwise.py)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "rankr1_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def toy():
    """toy-qwen2 at seed 929: dims, state, oracle, head - computed once, never modified"""
    from llmrankers import _synth
    from _qwen2_ref import Qwen2Oracle
    dims = _synth.TOY_QWEN2
    state = _synth.synth_state_dict(dims, seed=929)
    return dims, state, Qwen2Oracle(dims, state), np.asarray(state["model.embed_tokens.weight"], dtype=np.float32)


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 4096)
    kw.setdefault("max_seqs", 16)
    return RkLlamaEngine(dims, device=0, **kw).load_state(state.items())


def _all_logits(eng, seqs, vocab):
    return np.concatenate([eng.last_logits(seqs, list(range(v0, v0 + 64))) for v0 in range(0, vocab, 64)], axis=1)


def test_prefill_with_bias_vs_oracle(toy):
    """Check 1: 6 ragged prompts (1, 2, 63, 64, 65, 300 tokens), every vocabulary row, against the fp32 oracle"""
    from llmrankers import _synth
    dims, state, orc, _ = toy
    seqs = [_synth.synth_token_batch(1, n, n, dims.vocab, seed=40 + n)[0] for n in (1, 2, 63, 64, 65, 300)]
    eng = _engine(dims, state)
    got = _all_logits(eng, seqs, dims.vocab)
    eng.close()
    want = orc.last_logits(seqs)
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"max |logit - oracle| = {err:.3e} at scale {scale:.2f} (bound {BOUND * scale:.3e})")
    assert got.shape == want.shape == (6, dims.vocab)
    assert err < BOUND * scale, (err, scale)
    # what the bound is worth: the oracle with any ONE of the three biases dropped is 9 (k) to 50 (v) bounds away
    from _qwen2_ref import Qwen2Oracle
    for m in ("q_proj", "k_proj", "v_proj"):
        less = {k: v for k, v in state.items() if not k.endswith(m + ".bias")}
        off = float(np.abs(Qwen2Oracle(dims, less).last_logits(seqs[3:4]) - want[3:4]).max())
        print(f"oracle without the {m} bias: {off:.2f} away")
        assert off > 5 * BOUND * scale, (m, off)


def test_decode_step_with_bias_at_chunk_boundaries(toy):
    """Check 2: prefixes of one 300-token sequence around the step kernel's 128-key chunks, max_new 1 .. 4, no EOS: the rows the
    last step's head read against the oracle; tokens == the oracle's and == a greedy1 re-prefill loop wherever the oracle margin
    clears the floor (a step's cached key equals a prefill's).  toy-qwen2 has 7 query heads on 1 kv head: R = 1 by the plan's rule;
    the same run with all seven in one pass over the cache (R = 7, option llama_dec_r = 2) gives the same bits."""
    from llmrankers import _synth
    from _llama_gen_stub import oracle_greedy
    dims, state, orc, head = toy
    base = _synth.synth_token_batch(1, 300, 300, dims.vocab, seed=17)[0]
    seqs = [base[:n] for n in (1, 2, 3, 126, 127, 128, 129, 255, 256, 257)]
    eng = _engine(dims, state)
    gen = None
    for max_new in range(1, 5):
        gen, steps = eng.generate(seqs, max_new, [], 0)
        assert steps == max_new and gen.shape == (len(seqs), max_new)
        last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), dims.hidden)
        want = orc.last_logits([list(s) + [int(t) for t in gen[b, :max_new - 1]] for b, s in enumerate(seqs)])
        scale, err = float(np.abs(want).max()), float(np.abs(last @ head.T - want).max())
        print(f"max_new {max_new}: max |logit - oracle| = {err:.3e} at scale {scale:.2f}")
        assert err < BOUND * scale, (max_new, err, scale)
    rows = last.copy()                                             # (of the 4-token run; the greedy1 calls below reuse the buffer)
    checked = 0
    for b, s in enumerate(seqs):
        toks, margins = oracle_greedy(orc, s, 4)
        low = next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
        assert list(gen[b, :low]) == toks[:low], (b, low)
        cur = list(s)
        for t in range(low):
            assert int(eng.greedy1([cur])[0]) == int(gen[b, t]), (b, t)
            cur.append(int(gen[b, t]))
        checked += low
    assert checked >= 20, checked
    # all seven heads of the kv head per workgroup (R = 7) instead of one: the same bits
    eng.set_option("llama_dec_r", 2)
    gen1, _ = eng.generate(seqs, 4, [], 0)
    rows1 = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), dims.hidden)
    eng.close()
    np.testing.assert_array_equal(gen1, gen)
    assert rows1.shape == rows.shape and np.array_equal(rows1.view(np.uint32), rows.view(np.uint32))


def test_outlier_bias_channels_vs_hf_fp16_error(gold, toy):
    """Check 3: 4 channels of every k bias and 2 of every q bias x 40: the engine's max logit error against fp32 on 4 prompts of
    40 - 120 tokens must not exceed HF's own fp16 error there (Qwen2ForCausalLM.half() on the CPU against fp32, recorded by
    tools/make_rankr1_golden.py)"""
    from llmrankers import _synth
    from _qwen2_ref import Qwen2Oracle, with_bias_outliers
    dims, state, _, _ = toy
    rec = gold["outlier"]
    assert (rec["dims"], rec["seed"]) == ("toy-qwen2", 929)
    out = with_bias_outliers(state)
    seqs = _synth.synth_token_batch(4, 40, 120, dims.vocab, seed=rec["prompt_seed"])
    assert [len(s) for s in seqs] == rec["prompt_lens"]
    eng = _engine(dims, out)
    got = _all_logits(eng, seqs, dims.vocab)
    eng.close()
    want = Qwen2Oracle(dims, out).last_logits(seqs)
    errs = np.abs(got - want).max(axis=1)
    print(f"engine max |logit - fp32| per prompt {[f'{e:.4f}' for e in errs]}; HF fp16: {[f'{e:.4f}' for e in rec['hf_fp16_err_per_prompt']]} "
          f"(scale {float(np.abs(want).max()):.2f})")
    assert float(errs.max()) <= rec["hf_fp16_max_err"], (float(errs.max()), rec["hf_fp16_max_err"])


def test_batch_independence(toy):
    """Check 4: a row alone, in a batch of 7 and in the reversed batch: equal tokens where the oracle margins clear the floor,
    bit-equal final rows between the batch and the reversed batch"""
    from _llama_gen_stub import oracle_greedy
    dims, state, orc, _ = toy
    rs = np.random.RandomState(23)
    seqs = [rs.randint(3, dims.vocab - 28, size=n).astype(np.int32) for n in (3, 300, 129, 47, 256, 64, 190)]
    eng = _engine(dims, state)
    batch, _ = eng.generate(seqs, 6, [], 0)
    last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), -1).copy()
    rev, _ = eng.generate(seqs[::-1], 6, [], 0)
    last_rev = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), -1)
    np.testing.assert_array_equal(rev[::-1], batch)
    assert np.array_equal(last_rev[::-1].view(np.uint32), last.view(np.uint32))
    for b, s in enumerate(seqs):
        alone, _ = eng.generate([s], 6, [], 0)
        toks, margins = oracle_greedy(orc, s, 6)
        low = next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
        assert list(alone[0, :low]) == list(batch[b, :low]) == toks[:low], (b, low)
    eng.close()


def test_zero_bias_path_equals_the_bias_free_path_bit_for_bit():
    """Check 5: on the same weights, the switch on with all-zero bias vectors == the switch off (the bias-free kernels, which the
    existing Llama tests hold to their recorded behaviour) - last_logits bits and generate tokens; on toy-llama's shape (2 query
    heads per kv head) and toy-qwen2's (7).  (The step's final rows are not compared bit for bit: the bias path rounds a step's
    queries as the prefill does, the bias-free step as its compiler pleases.)"""
    from llmrankers import _synth
    for name in ("toy-llama", "toy-qwen2"):
        off = dataclasses.replace(_synth.NAMED_DIMS[name], qkv_bias=False)
        on = dataclasses.replace(off, qkv_bias=True)
        state = {k: v for k, v in _synth.synth_state_dict(off, seed=929).items()}
        assert not any(k.endswith(".bias") for k in state)
        zero = dict(state)
        for n, shape, _, _ in _synth.llama_tensor_specs(on):
            if n.endswith(".bias"):
                zero[n] = np.zeros(shape, np.float32)
        seqs = _synth.synth_token_batch(5, 2, 270, off.vocab, seed=9)
        ids = list(range(0, off.vocab, off.vocab // 64))              # 64 vocabulary rows, the most one call takes
        res = []
        for dims, st in ((off, state), (on, zero)):
            eng = _engine(dims, st)
            lg = eng.last_logits(seqs, ids)
            gen, steps = eng.generate(seqs, 5, [], 0)
            eng.close()
            res.append((lg, gen))
        assert np.array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32)), name
        np.testing.assert_array_equal(res[0][1], res[1][1])


def test_contract(toy, ckpt_dirs):
    """Check 6: rk_llama_set_qkv_bias on a T5 engine and after finalize: RK_ERR_STATE; finalize with the switch on and a bias
    missing: RK_ERR_MISSING naming the tensor; with the switch off the bias names are ignored"""
    from conftest import load_state
    from llmrankers._engine import RkEngine, RkError, RkLlamaEngine
    dims, state, orc, _ = toy
    t5dims, t5state = load_state(ckpt_dirs["ckpt_gated_untied"])
    t5 = RkEngine(t5dims, device=0, max_tokens=512, max_seqs=4, max_dec_len=4)
    assert t5.lib.rk_llama_set_qkv_bias(t5.h, 1) == -4
    t5.close()
    eng = _engine(dims, state, max_tokens=512, max_seqs=4)
    assert eng.lib.rk_llama_set_qkv_bias(eng.h, 0) == -4
    assert b"finalize" in eng.lib.rk_last_error(eng.h)
    eng.close()
    missing = "model.layers.1.self_attn.k_proj.bias"
    eng = RkLlamaEngine(dims, device=0, max_tokens=512, max_seqs=4)
    with pytest.raises(RkError) as ex:
        eng.load_state((k, v) for k, v in state.items() if k != missing)
    assert ex.value.code == -5 and missing in str(ex.value)
    eng.close()
    # switch off: the checkpoint's biases are ignored - the engine computes the bias-free model
    import dataclasses as dc
    from oracle.llama_numpy import LlamaOracle
    eng = _engine(dc.replace(dims, qkv_bias=False), state, max_tokens=512, max_seqs=4)
    seqs = [[5, 9, 200, 31, 77]]
    got = eng.last_logits(seqs, list(range(64)))
    eng.close()
    want = LlamaOracle(dims, state).last_logits(seqs)[:, :64]
    assert float(np.abs(got - want).max()) < BOUND * float(np.abs(want).max())


def test_rankr1_golden_cases_on_the_engine(gold, tmp_path):
    """Check 7: the recorded cases through RankR1SetwiseLlmRanker.from_runtime on the real engine, checkpoint and adapter written
    from the recipes (sha256 asserted), the adapter merged by the loader"""
    from transformers import AutoTokenizer
    from llmrankers import _synth
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    assert gold["min_margin"] > FLOOR
    path, adir = str(tmp_path / "toy-qwen2"), str(tmp_path / "adapter")
    _synth.write_checkpoint(path, gold["ckpt"], os.path.join(GOLD, gold["tokenizer"]))
    assert _synth.checkpoint_sha256(path) == gold["ckpt"]["sha256"]
    assert _synth.write_lora_adapter(adir, _synth.NAMED_DIMS[gold["ckpt"]["dims"]], gold["adapter"]) == gold["adapter"]["sha256"]
    with pytest.raises(NotImplementedError):
        LlamaRuntime(path, "cuda")                                  # the default still serves Llama only
    rt = LlamaRuntime(path, "cuda", max_tokens=4096, max_seqs=16, accept_model_types=("qwen2",), adapter_dir=adir)
    assert rt.model_type == "qwen2" and rt.dims.qkv_bias and rt.generation["eos_token_ids"] == [gold["model_eos"]]
    tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, gold["tokenizer"]))    # (its own directory: see test_rankr1_host.py)
    for case in gold["cases"]:
        rk = RankR1SetwiseLlmRanker.from_runtime(rt, tok, os.path.join(GOLD, "rankr1_prompt.toml"), num_child=case["num_child"], k=case["k"],
                                                 method=case["method"], num_permutation=case["num_permutation"],
                                                 max_new_tokens=case["max_new_tokens"])
        outs, real = [], rk.compare
        rk.compare = lambda q, docs: outs.append(real(q, docs)) or outs[-1]
        random.seed(case["random_seed"])
        res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
        tag = case["qid"]
        assert outs == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
    rt.engine.close()
    # the reference's constructor: checkpoint, prompt file, adapter directory and tokenizer by path
    case = gold["cases"][2]
    rk = RankR1SetwiseLlmRanker(path, os.path.join(GOLD, "rankr1_prompt.toml"), lora_name_or_path=adir,
                                tokenizer_name_or_path=os.path.join(GOLD, gold["tokenizer"]), num_child=case["num_child"], k=case["k"],
                                method=case["method"], num_permutation=case["num_permutation"], max_new_tokens=case["max_new_tokens"])
    assert rk.lora_path == adir and rk.llm.model_type == "qwen2"
    random.seed(case["random_seed"])
    res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
    assert [d.docid for d in res] == case["docids"]
    assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"]
    rk.llm.engine.close()
