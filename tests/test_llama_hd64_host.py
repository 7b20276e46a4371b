"""Host logic for Llama / Qwen2 checkpoints with 64-wide heads, without a GPU: the registered dimensions, the head width a
Llama-3.2-1B-shaped config gives, which widths LlamaRuntime and the rankers accept (the engine behind them is a stub that records
what it is asked to create), and the checkpoint recipes of tests/golden/llama_hd64_ckpts.json."""
import json
import os

import pytest

from conftest import GOLD
from llmrankers import _synth

LLAMA_32_1B_CONFIG = {          # the published config's shape (no "head_dim" entry: hidden_size / num_attention_heads)
    "architectures": ["LlamaForCausalLM"], "model_type": "llama", "vocab_size": 128256, "hidden_size": 2048, "intermediate_size": 8192,
    "num_hidden_layers": 16, "num_attention_heads": 32, "num_key_value_heads": 8, "hidden_act": "silu", "rms_norm_eps": 1e-5,
    "rope_theta": 500000.0, "max_position_embeddings": 131072, "attention_bias": False, "mlp_bias": False, "tie_word_embeddings": True,
    "bos_token_id": 128000, "eos_token_id": [128001, 128008, 128009],
    "rope_scaling": {"factor": 32.0, "high_freq_factor": 4.0, "low_freq_factor": 1.0, "original_max_position_embeddings": 8192, "rope_type": "llama3"},
}


@pytest.fixture(scope="module")
def specs():
    with open(os.path.join(GOLD, "llama_hd64_ckpts.json")) as f:
        return json.load(f)


def test_named_dims_and_the_head_width_of_a_llama_32_1b_config():
    d = _synth.LlamaDims.from_hf_config(LLAMA_32_1B_CONFIG)
    assert d.head_dim == 64 and (d.n_heads, d.n_kv_heads, d.hidden, d.intermediate, d.n_layers, d.vocab) == (32, 8, 2048, 8192, 16, 128256)
    assert d.tied_head and d.rope_scaling == (32.0, 1.0, 4.0, 8192) and d.eos_token_id == 128001
    assert d == _synth.LLAMA_32_1B == _synth.NAMED_DIMS["llama-3.2-1b"]
    assert _synth.LlamaDims.from_hf_config({**LLAMA_32_1B_CONFIG, "head_dim": 64}).head_dim == 64
    t, q = _synth.NAMED_DIMS["tinyllama-1.1b"], _synth.NAMED_DIMS["qwen2.5-0.5b"]
    assert (t.hidden, t.n_heads, t.n_kv_heads, t.head_dim, t.intermediate, t.n_layers, t.vocab, t.rope_theta) == (2048, 32, 4, 64, 5632, 22, 32000, 10000.0)
    assert (q.hidden, q.n_heads, q.n_kv_heads, q.head_dim, q.intermediate, q.n_layers, q.vocab) == (896, 14, 2, 64, 4864, 24, 151936)
    assert q.qkv_bias and q.tied_head and q.rope_theta == 1000000.0
    a, b, c = _synth.NAMED_DIMS["toy-llama-hd64"], _synth.NAMED_DIMS["toy-qwen2-hd64"], _synth.NAMED_DIMS["toy-llama-mha-hd64"]
    assert a == _synth.LlamaDims(**{**_synth.TOY_LLAMA.__dict__, "n_heads": 8, "n_kv_heads": 2, "head_dim": 64})
    assert (b.n_heads, b.n_kv_heads, b.head_dim, b.qkv_bias) == (7, 1, 64, True) and (c.n_heads, c.n_kv_heads, c.head_dim) == (3, 3, 64)
    for dims in (a, b, c, q, _synth.LLAMA_32_1B):
        assert _synth.LlamaDims.from_hf_config(dims.to_hf_config()) == dims


class _StubEngine:
    """RkLlamaEngine's constructor and loader, recording: what LlamaRuntime asks the engine for"""
    made = []

    def __init__(self, dims, device=0, max_tokens=16384, max_seqs=16):
        self.dims, self.loaded = dims, 0
        _StubEngine.made.append(self)

    def load_state(self, tensors):
        self.loaded = sum(1 for _ in tensors)
        return self

    def close(self):
        pass


@pytest.fixture()
def stub_engine(monkeypatch):
    from llmrankers import _runtime
    monkeypatch.setattr(_runtime, "RkLlamaEngine", _StubEngine)
    del _StubEngine.made[:]
    return _StubEngine


def _write(tmp_path, name, dims, tok):
    import shutil
    path = str(tmp_path / name)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dims.to_hf_config(), f)
    from safetensors.numpy import save_file
    import numpy as np
    save_file({"model.norm.weight": np.ones(dims.hidden, np.float32)}, os.path.join(path, "model.safetensors"))
    for fn in os.listdir(os.path.join(GOLD, tok)):
        shutil.copy(os.path.join(GOLD, tok, fn), os.path.join(path, fn))
    return path


def test_runtime_and_rankers_construct_on_64_wide_configs(stub_engine, tmp_path):
    import dataclasses
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.listwise import ListwiseLlmRanker
    from llmrankers.pairwise import PairwiseLlmRanker
    from llmrankers.setwise import RankR1SetwiseLlmRanker, SetwiseLlmRanker
    small = dataclasses.replace(_synth.LLAMA_32_1B, n_layers=1, vocab=256, bos_token_id=1, eos_token_id=2)
    path = _write(tmp_path, "llama64", small, "tok_llama")
    rt = LlamaRuntime(path, "cuda")
    assert rt.dims.head_dim == 64 and rt.engine is stub_engine.made[-1] and rt.engine.dims == small and rt.engine.loaded == 1
    n = len(stub_engine.made)
    SetwiseLlmRanker(path, path, "cuda", num_child=3, k=5, scoring="generation", method="heapsort")
    PairwiseLlmRanker(path, path, "cuda", method="heapsort", batch_size=2, k=3)
    ListwiseLlmRanker(path, path, "cuda", 4, 2)
    assert len(stub_engine.made) == n + 3 and all(e.dims.head_dim == 64 for e in stub_engine.made)
    # Rank-R1 on the Qwen2.5-0.5B shape (tokenizer from its own directory: see test_rankr1_host.py)
    q05 = dataclasses.replace(_synth.QWEN25_05B, n_layers=1, vocab=512, bos_token_id=1, eos_token_id=2)
    qpath = _write(tmp_path, "qwen64", q05, "tok_qwen")
    rk = RankR1SetwiseLlmRanker(qpath, os.path.join(GOLD, "rankr1_prompt.toml"), tokenizer_name_or_path=os.path.join(GOLD, "tok_qwen"))
    assert rk.llm.model_type == "qwen2" and rk.llm.dims.head_dim == 64 and rk.llm.dims.qkv_bias and (rk.llm.dims.n_heads, rk.llm.dims.n_kv_heads) == (14, 2)
    # what stays refused: another head width, and hidden > 4096 (Qwen2.5-14B / Rank-R1-14B) - before an engine is asked for
    n = len(stub_engine.made)
    for name, dims in (("hd96", dataclasses.replace(small, head_dim=96)), ("h5120", dataclasses.replace(small, hidden=5120, n_heads=40, head_dim=128))):
        bad = _write(tmp_path, name, dims, "tok_llama")
        with pytest.raises(NotImplementedError, match="head_dim 64 or 128") as ei:
            LlamaRuntime(bad, "cuda")
        assert "hidden <= 4096" in str(ei.value)
        for build in (lambda: SetwiseLlmRanker(bad, bad, "cuda"), lambda: PairwiseLlmRanker(bad, bad, "cuda", method="heapsort"),
                      lambda: ListwiseLlmRanker(bad, bad, "cuda", 4, 2),
                      lambda: RankR1SetwiseLlmRanker(bad, os.path.join(GOLD, "rankr1_prompt.toml"), tokenizer_name_or_path=os.path.join(GOLD, "tok_qwen"))):
            with pytest.raises(NotImplementedError):
                build()
    assert len(stub_engine.made) == n


def test_recipes_sha256(specs, tmp_path):
    assert {"ckpt_llama_hd64", "ckpt_qwen2_hd64"} <= set(specs)
    for name, spec in specs.items():
        if name.startswith("adapter"):
            assert _synth.write_lora_adapter(str(tmp_path / name), _synth.TOY_QWEN2_HD64, spec) == spec["sha256"]
            continue
        assert _synth.NAMED_DIMS[spec["dims"]].head_dim == 64
        path = str(tmp_path / name)
        _synth.write_checkpoint(path, spec, os.path.join(GOLD, spec["tokenizer"]))
        assert _synth.checkpoint_sha256(path) == spec["sha256"], name


def test_recorded_reference_cases_on_the_oracle(specs, tmp_path):
    """the reference's recorded setwise / pairwise / listwise cases (tests/golden/llama_hd64_cases.json) through the build's rankers
    on the numpy oracle: every compare in order, rankings, counters - the fixture and the host logic agree before a GPU is involved"""
    import random
    from safetensors.numpy import load_file
    from transformers import AutoTokenizer
    from _llama_gen_stub import OracleLlamaGenRuntime
    from _stub import OracleLlamaRuntime
    from llmrankers._runtime import read_config, read_generation_settings
    from llmrankers.listwise import ListwiseLlmRanker
    from llmrankers.pairwise import PairwiseLlmRanker
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import SetwiseLlmRanker
    with open(os.path.join(GOLD, "llama_hd64_cases.json")) as f:
        cases = json.load(f)
    assert all(c["min_margin"] >= cases["keep"] == 4 * cases["floor"] for c in cases["cases"])
    assert {c["kind"] for c in cases["cases"]} == {"setwise-llama", "pairwise-llama", "listwise-llama", "rankr1-qwen2"}
    dims = _synth.TOY_LLAMA_HD64

    def ckpt(name):
        path = str(tmp_path / name)
        _synth.write_checkpoint(path, specs[name], os.path.join(GOLD, specs[name]["tokenizer"]))
        return path, load_file(os.path.join(path, "model.safetensors"))

    path, state = ckpt("ckpt_llama_hd64")
    rt, tok = OracleLlamaRuntime(dims, state), AutoTokenizer.from_pretrained(path)
    n = 0
    for case in cases["cases"]:
        if case["kind"] == "setwise-llama":
            rk = SetwiseLlmRanker.from_runtime(rt, tok, num_child=case["num_child"], k=case["k"], scoring=case["scoring"], method=case["method"],
                                               num_permutation=case["num_permutation"])
            rk.batch_independent_compares = False
            ids_of = lambda docs: [d.docid for d in docs]
        elif case["kind"] == "pairwise-llama":
            rk, ids_of = PairwiseLlmRanker.from_runtime(rt, tok, method=case["method"], batch_size=2, k=case["k"]), list
        else:
            continue
        log, orig = [], rk.compare
        rk.compare = lambda q, d, _o=orig, _l=log, _i=ids_of: (_l.append([_i(d)]), _l[-1].append(_o(q, d)))[1] or _l[-1][1]
        ranking = [SearchResult(docid=d, score=s, text=t) for d, s, t in case["input"]]
        random.seed(929)
        res = rk.rerank(case["query"], ranking)
        assert log == case["compares"], (case["kind"], case["method"])
        assert [[r.docid, r.score] for r in res] == case["result"] and [r.docid for r in ranking] == case["caller_list_after"]
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"]
        n += 1
    assert n >= 8
    path, state = ckpt("ckpt_llama_hd64_listwise")
    rt = OracleLlamaGenRuntime(dims, state, generation=read_generation_settings(path, read_config(path)))
    tok = AutoTokenizer.from_pretrained(path)
    tok.use_default_system_prompt = False
    for case in (c for c in cases["cases"] if c["kind"] == "listwise-llama"):
        rk = ListwiseLlmRanker.from_runtime(rt, tok, window_size=case["window_size"], step_size=case["step_size"], scoring=case["scoring"],
                                            num_repeat=case["num_repeat"])
        outs, real = [], rk.compare
        rk.compare = lambda q, docs: outs.append(real(q, docs)) or outs[-1]
        res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
        assert outs == [c["output"] for c in case["compares"]], case["qid"]
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"]
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"]
