"""Rank-R1 on the host: the Qwen2 oracle against HF, the Qwen2 configuration round trip, the LoRA merge, and RankR1SetwiseLlmRanker
over an oracle-backed runtime double against the reference's recorded cases (tools/make_rankr1_golden.py)."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLD


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "rankr1_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def r1_ckpt(gold, tmp_path_factory):
    from llmrankers import _synth
    root = tmp_path_factory.mktemp("rankr1_host")
    path, adir = str(root / "toy-qwen2"), str(root / "adapter")
    _synth.write_checkpoint(path, gold["ckpt"], os.path.join(GOLD, gold["tokenizer"]))
    assert _synth.checkpoint_sha256(path) == gold["ckpt"]["sha256"]
    assert _synth.write_lora_adapter(adir, _synth.NAMED_DIMS[gold["ckpt"]["dims"]], gold["adapter"]) == gold["adapter"]["sha256"]
    return path, adir


def ids_sha256(ids):
    return hashlib.sha256(np.asarray(ids, dtype=np.int32).tobytes()).hexdigest()


def test_existing_synthetic_checkpoints_did_not_move(ckpt_dirs):
    """the bias specs only exist for qkv_bias dims: every recorded Llama / T5 recipe still regenerates its sha256 (ckpt_dirs asserts)"""
    from llmrankers import _synth
    assert not any("bias" in n for n, *_ in _synth.llama_tensor_specs(_synth.TOY_LLAMA))
    names = [n for n, *_ in _synth.llama_tensor_specs(_synth.TOY_QWEN2)]
    assert sum(n.endswith("_proj.bias") for n in names) == 3 * _synth.TOY_QWEN2.n_layers
    assert not any(n.endswith("o_proj.bias") for n in names)


def test_qwen2_oracle_vs_hf_fp32():
    import torch
    from transformers import Qwen2Config, Qwen2ForCausalLM
    from llmrankers import _synth
    from _qwen2_ref import Qwen2Oracle
    dims = _synth.TOY_QWEN2
    state = _synth.synth_state_dict(dims, seed=929)
    model = Qwen2ForCausalLM(Qwen2Config(**dims.to_hf_config())).eval()
    res = model.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"lm_head.weight"}     # (tied head)
    orc = Qwen2Oracle(dims, state)
    seqs = [[int(t) for t in s] for s in _synth.synth_token_batch(3, 5, 60, dims.vocab, seed=3)]
    assert len({len(s) for s in seqs}) == 3
    for s in seqs:
        with torch.no_grad():
            want = model(torch.tensor([s])).logits[0, -1].numpy()
        err = float(np.abs(want - orc.last_logits([s])[0]).max())
        print(f"{len(s)} tokens: max |oracle - HF| = {err:.3e}")
        assert err < 1e-4, (len(s), err)
    # the biases matter: the Llama oracle on the same weights is far off
    from oracle.llama_numpy import LlamaOracle
    assert float(np.abs(LlamaOracle(dims, state).last_logits([seqs[0]]) - orc.last_logits([seqs[0]])).max()) > 1.0


def test_from_hf_config_round_trip_and_refusals(tmp_path):
    from llmrankers import _synth
    from llmrankers._runtime import load_runtime
    for dims in (_synth.TOY_QWEN2, _synth.QWEN25_7B):
        cfg = dims.to_hf_config()
        assert cfg["model_type"] == "qwen2" and cfg["architectures"] == ["Qwen2ForCausalLM"]
        assert _synth.LlamaDims.from_hf_config(cfg) == dims
    assert _synth.LlamaDims.from_hf_config(_synth.TOY_LLAMA.to_hf_config()) == _synth.TOY_LLAMA          # Llama as before
    assert not _synth.TOY_LLAMA.qkv_bias and _synth.NAMED_DIMS["toy-qwen2"] is _synth.TOY_QWEN2
    with pytest.raises(NotImplementedError):
        _synth.LlamaDims.from_hf_config({**_synth.TOY_QWEN2.to_hf_config(), "use_sliding_window": True})
    with pytest.raises(NotImplementedError):
        _synth.LlamaDims.from_hf_config({**_synth.TOY_LLAMA.to_hf_config(), "attention_bias": True})
    with open(tmp_path / "config.json", "w") as f:
        json.dump(_synth.TOY_QWEN2.to_hf_config(), f)
    with pytest.raises(NotImplementedError, match="qwen2"):
        load_runtime(str(tmp_path), "cuda")                          # setwise / pairwise / listwise keep refusing Qwen


def _adapter_dir(tmp_path, dims, spec, **cfg_over):
    from llmrankers import _synth
    path = str(tmp_path)
    _synth.write_lora_adapter(path, dims, spec)
    if cfg_over:
        with open(os.path.join(path, "adapter_config.json")) as f:
            cfg = json.load(f)
        cfg.update(cfg_over)
        with open(os.path.join(path, "adapter_config.json"), "w") as f:
            json.dump(cfg, f)
    return path


def test_merge_lora(tmp_path):
    from safetensors.numpy import load_file, save_file
    from llmrankers import _synth
    from llmrankers._runtime import merge_lora
    from _qwen2_ref import host_merge_lora
    dims = _synth.TOY_QWEN2
    state = _synth.synth_state_dict(dims, seed=7)
    spec = {"seed": 5, "r": 4, "lora_alpha": 8, "std": 0.05}
    adapter = _synth.synth_lora_tensors(dims, spec)
    assert len(adapter) == 2 * 7 * dims.n_layers
    for name, rs, scale in (("plain", False, 8 / 4), ("rslora", True, 8 / 2.0)):
        adir = _adapter_dir(tmp_path / name, dims, spec, use_rslora=rs)
        got = dict(merge_lora(iter(state.items()), adir))
        want = host_merge_lora(state, adapter, scale)
        assert list(got) == list(state)
        worst = 0.0
        for k in state:
            if k.endswith("_proj.weight"):
                assert got[k].dtype == np.float32
                worst = max(worst, float(np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)).max()))
                assert float(np.abs(got[k] - state[k]).max()) > 1e-3                   # the adapter changed it
            else:
                assert got[k] is state[k]                                             # biases, norms, embedding: untouched
        print(f"{name}: max |merge - fp64 merge| = {worst:.3e}")
        assert worst < 1e-6
    # a bf16 base weight (raw bits, as iter_checkpoint_tensors hands it on) merges the same
    k = "model.layers.0.self_attn.q_proj.weight"
    bf = (state[k].view(np.uint32) >> 16).astype(np.uint16)
    as32 = (bf.astype(np.uint32) << 16).view(np.float32)
    got = dict(merge_lora(iter([(k2, bf if k2 == k else v) for k2, v in state.items()]), str(tmp_path / "plain")))
    assert float(np.abs(got[k] - host_merge_lora({**state, k: as32}, adapter, 2.0)[k]).max()) < 1e-6
    # an adapter key that matches no checkpoint tensor is an error, not skipped
    dangling = dict(load_file(os.path.join(str(tmp_path / "plain"), "adapter_model.safetensors")))
    for tag in ("lora_A", "lora_B"):
        dangling[f"base_model.model.model.layers.9.self_attn.q_proj.{tag}.weight"] = dangling[f"base_model.model.model.layers.0.self_attn.q_proj.{tag}.weight"]
    adir = _adapter_dir(tmp_path / "dangling", dims, spec)
    save_file(dangling, os.path.join(adir, "adapter_model.safetensors"))
    with pytest.raises(KeyError, match="layers.9"):
        list(merge_lora(iter(state.items()), adir))
    for over in ({"use_dora": True}, {"bias": "all"}, {"modules_to_save": ["lm_head"]}, {"target_modules": ["q_proj", "embed_tokens"]}):
        adir = _adapter_dir(tmp_path / ("bad_" + next(iter(over))), dims, spec, **over)
        with pytest.raises(NotImplementedError):
            list(merge_lora(iter(state.items()), adir))


def _ranker(gold, r1_ckpt, case, prompt_file=None):
    from transformers import AutoTokenizer
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    from _qwen2_ref import OracleQwen2GenRuntime, load_qwen2_state, merged_state
    path, _ = r1_ckpt
    dims, state = load_qwen2_state(path)
    rt = OracleQwen2GenRuntime(dims, merged_state(dims, state, gold["adapter"]))
    assert rt.generation["eos_token_ids"] == [gold["model_eos"]]
    # the tokenizer from its OWN directory: beside a config.json with model_type qwen2 AutoTokenizer builds Qwen's byte-level BPE
    # class over the word-level tokenizer.json and every word falls apart
    tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, gold["tokenizer"]))
    rk = RankR1SetwiseLlmRanker.from_runtime(rt, tok, prompt_file if prompt_file is not None else gold["prompt"],
                                             num_child=case["num_child"], k=case["k"], method=case["method"],
                                             num_permutation=case["num_permutation"], max_new_tokens=case["max_new_tokens"])
    return rk, rt


def _run_case(rk, rt, case):
    """rerank with every compare's prompts and new tokens logged -> (result, [{output, rows}])"""
    from llmrankers.rankers import SearchResult
    log, real_generate, real_compare = [], rt.generate, rk.compare

    def generate(seqs, max_new, eos_ids, pad_id, max_total=0):
        out = real_generate(seqs, max_new, eos_ids, pad_id, max_total)
        log.append((seqs, np.asarray(out)))
        return out

    compares = []

    def compare(query, docs):
        n0 = len(log)
        out = real_compare(query, docs)
        assert len(log) == n0 + 1                                     # all permutations in ONE generate call
        compares.append({"output": out, "seqs": log[n0][0], "new": log[n0][1]})
        return out

    rt.generate, rk.compare = generate, compare
    random.seed(case["random_seed"])
    res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
    return res, compares


def test_ranker_reproduces_the_recorded_cases(gold, r1_ckpt):
    assert gold["min_margin"] > gold["floor"]
    eos = gold["model_eos"]
    seen = {"eos": False, "full": False, "nomatch": False, "moved": False}
    for case in gold["cases"]:
        rk, rt = _ranker(gold, r1_ckpt, case)
        assert rk.CHARACTERS == [f"[{i}]" for i in range(1, 21)]
        res, compares = _run_case(rk, rt, case)
        tag = case["qid"]
        assert [c["output"] for c in compares] == [c["output"] for c in case["compares"]], tag
        for got, want in zip(compares, case["compares"]):
            assert [ids_sha256(s) for s in got["seqs"]] == [r["prompt_sha256"] for r in want["rows"]], tag
            for row, r in zip(got["new"], want["rows"]):
                new = [int(t) for t in row if t >= 0]
                if eos in new:
                    new = new[:new.index(eos) + 1]
                assert new == r["new_ids"], tag
                assert rk.tokenizer.decode(new, skip_special_tokens=True) == r["completion"], tag
                seen["eos"] |= new[-1] == eos and len(new) < case["max_new_tokens"]
                seen["full"] |= new[-1] != eos and len(new) == case["max_new_tokens"]
        seen["nomatch"] |= any(c["output"] == "Unexpected voting." for c in case["compares"])
        seen["moved"] |= case["docids"] != [d for d, _ in case["docs"]]
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
    assert all(seen.values()), seen
    # the recorded prompts are real prompts: three different ones in a 3-permutation compare, no prompt shared between cases
    assert any(len({r["prompt_sha256"] for r in c["rows"]}) == 3 for case in gold["cases"] if case["num_permutation"] == 3
               for c in case["compares"])
    per_case = [{r["prompt_sha256"] for c in case["compares"] for r in c["rows"]} for case in gold["cases"]]
    assert all(not (a & b) for i, a in enumerate(per_case) for b in per_case[i + 1:])
    # rerank_many: one rerank per query, the same results and counters
    case = gold["cases"][0]
    rk, rt = _ranker(gold, r1_ckpt, case)
    from llmrankers.rankers import SearchResult
    random.seed(case["random_seed"])
    out, counters = rk.rerank_many([(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])])
    assert [d.docid for d in out[0]] == case["docids"] and list(counters[0]) == case["counters"]


def test_prompt_tokens_are_what_the_reference_lists(gold, r1_ckpt):
    """one compare, token by token: ChatML markers and role words, the system text, the query, "[n] passage" lines in the shuffled
    order with the labels in order, the closing question, the generation prompt - every piece a vocabulary word (no <unk>)"""
    case = gold["cases"][1]
    rk, rt = _ranker(gold, r1_ckpt, case)
    seen = []
    rt.generate = lambda seqs, *a, **kw: seen.append(seqs) or np.full((len(seqs), 1), gold["model_eos"], np.int32)
    from llmrankers.rankers import SearchResult
    docs = [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]][:4]
    random.seed(5)
    order = [random.sample(list(range(4)), 4) for _ in range(3)]
    random.seed(5)
    assert rk.compare(case["query"], docs) == "Unexpected voting."
    tok = rk.tokenizer
    assert len(seen) == 1 and len(seen[0]) == 3 and len({tuple(s) for s in seen[0]}) == 3
    for perm, ids in zip(order, seen[0]):
        lines = "\n".join(f"[{i + 1}] {docs[d].text}" for i, d in enumerate(perm))
        want = (f"<|im_start|> system {gold['prompt']['prompt_system']} <|im_end|> <|im_start|> user "
                f"{gold['prompt']['prompt_user'].format(query=case['query'], docs=lines)} <|im_end|> <|im_start|> assistant")
        assert tok.unk_token_id not in ids
        assert tok.decode(ids).split() == want.split()
        assert [tok.convert_ids_to_tokens(t) for t in ids if tok.convert_ids_to_tokens(t).startswith("[")] == ["[1]", "[2]", "[3]", "[4]"]


def test_the_adapter_matters(gold, r1_ckpt):
    """the recorded compare the generator names changes its tokens when the adapter is left out"""
    from _llama_gen_stub import oracle_greedy
    from _qwen2_ref import Qwen2Oracle, load_qwen2_state, merged_state
    w = gold["without_adapter"]
    case = gold["cases"][w["case"]]
    row = case["compares"][w["compare"]]["rows"][w["row"]]
    rk, rt = _ranker(gold, r1_ckpt, case)
    _, compares = _run_case(rk, rt, case)
    ids = compares[w["compare"]]["seqs"][w["row"]]
    dims, state = load_qwen2_state(r1_ckpt[0])
    base, _ = oracle_greedy(Qwen2Oracle(dims, state), ids, case["max_new_tokens"], (gold["model_eos"],))
    assert base == w["base_new_ids"] != row["new_ids"]


def test_prompt_file_forms_and_constructor_contract(gold, r1_ckpt):
    from llmrankers.setwise import RankR1SetwiseLlmRanker, SetwiseLlmRanker, load_prompt_file
    assert issubclass(RankR1SetwiseLlmRanker, SetwiseLlmRanker)
    assert load_prompt_file(os.path.join(GOLD, "rankr1_prompt.toml")) == gold["prompt"] == load_prompt_file(gold["prompt"])
    case = gold["cases"][2]
    a, _ = _ranker(gold, r1_ckpt, case, os.path.join(GOLD, "rankr1_prompt.toml"))
    b, _ = _ranker(gold, r1_ckpt, case, gold["prompt"])
    assert a.prompt == b.prompt and a.max_new_tokens == b.max_new_tokens == case["max_new_tokens"]
    with pytest.raises(KeyError):
        load_prompt_file({"prompt_system": "x"})
    with pytest.raises(NotImplementedError, match="only supports 'generation'"):
        RankR1SetwiseLlmRanker("nowhere", gold["prompt"], scoring="likelihood")
    with pytest.raises(NotImplementedError, match="only supports 'generation'"):
        RankR1SetwiseLlmRanker.from_runtime(None, None, gold["prompt"], scoring="likelihood")
    import inspect
    names = list(inspect.signature(RankR1SetwiseLlmRanker.__init__).parameters)[1:]
    assert names == ["model_name_or_path", "prompt_file", "lora_name_or_path", "tokenizer_name_or_path", "num_child", "k", "scoring",
                     "method", "num_permutation", "cache_dir", "verbose", "device", "max_new_tokens"]
    d = {k: p.default for k, p in inspect.signature(RankR1SetwiseLlmRanker.__init__).parameters.items()}
    assert (d["num_child"], d["k"], d["method"], d["num_permutation"], d["max_new_tokens"], d["device"]) == (19, 10, "heapsort", 1, 2048, "cuda")
