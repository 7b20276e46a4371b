"""Host logic of the Qwen3 family (q / k head RMSNorm), without a GPU: the fp32 oracle against HF's recorded Qwen3ForCausalLM logits
and greedy tokens, the published configs' dims and every refusal, what the engine binding and the rankers are asked for (stubs
record the calls), what the GPU test's bound is worth on its own seed and prompts, and the recorded Rank-R1 cases on the oracle."""
import dataclasses
import json
import os
import random
import shutil

import numpy as np
import pytest

from conftest import GOLD, REPO
from llmrankers import _synth

FLOOR, BOUND = 5e-3, 4e-3               # tests/test_gpu_rankr1.py


def _published(hidden, inter, layers, heads, tied):
    """the published config's shape of Qwen/Qwen3-0.6B, -4B, -8B (head_dim is given; the q width heads x 128 need not equal hidden)"""
    return {"architectures": ["Qwen3ForCausalLM"], "model_type": "qwen3", "attention_bias": False, "attention_dropout": 0.0,
            "bos_token_id": 151643, "eos_token_id": 151645, "head_dim": 128, "hidden_act": "silu", "hidden_size": hidden,
            "initializer_range": 0.02, "intermediate_size": inter, "max_position_embeddings": 40960, "max_window_layers": layers,
            "num_attention_heads": heads, "num_hidden_layers": layers, "num_key_value_heads": 8, "rms_norm_eps": 1e-06, "rope_scaling": None,
            "rope_theta": 1000000, "sliding_window": None, "tie_word_embeddings": tied, "torch_dtype": "bfloat16", "use_cache": True,
            "use_sliding_window": False, "vocab_size": 151936}


QWEN3_06B_CONFIG = _published(1024, 3072, 28, 16, True)
QWEN3_4B_CONFIG = _published(2560, 9728, 36, 32, True)
QWEN3_8B_CONFIG = _published(4096, 12288, 36, 32, False)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "qwen3_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def toy(gold):
    from _qwen3_ref import Qwen3Oracle
    rec = gold["logits"]
    dims = _synth.NAMED_DIMS[rec["dims"]]
    state = _synth.synth_state_dict(dims, seed=rec["seed"], gain=rec["gain"])
    return dims, state, Qwen3Oracle(dims, state)


def test_qwen3_oracle_vs_hf_fp32(gold, toy):
    """tests/_qwen3_ref.py: Qwen3Oracle against HF's Qwen3ForCausalLM (fp32, tools/make_qwen3_golden.py), the tolerance
    tests/test_oracle_golden.py holds the Llama oracle to; HF's greedy tokens where its margins clear the floor"""
    from _llama_gen_stub import oracle_greedy
    dims, state, orc = toy
    assert dims is _synth.TOY_QWEN3 and dims.qk_norm
    assert sum(k.endswith("_norm.weight") for k in state) == 2 * dims.n_layers and state["model.layers.1.self_attn.k_norm.weight"].shape == (128,)
    rec = gold["logits"]
    seqs = [_synth.synth_token_batch(1, n, n, dims.vocab, seed=s)[0] for n, s in rec["prompts"]]
    want = np.asarray(rec["last_logits"], dtype=np.float32)
    got = orc.last_logits(seqs)
    assert got.shape == want.shape == (3, dims.vocab)
    assert np.abs(got - want).max() < 2e-4 * max(1.0, np.abs(want).max())
    # the norm is not a no-op at this seed: the plain Llama oracle on the same weights is far away
    from oracle.llama_numpy import LlamaOracle
    assert np.abs(LlamaOracle(dims, state).last_logits(seqs) - want).max() > 50 * 2e-4 * np.abs(want).max()
    g = gold["greedy"]
    assert (g["dims"], g["seed"], g["gain"]) == (rec["dims"], rec["seed"], rec["gain"])
    base = _synth.synth_token_batch(1, 300, 300, dims.vocab, seed=g["base_seed"])[0]
    compared = 0
    for n, toks, margins in zip(g["prefix_lens"], g["tokens"], g["margins"]):
        mine, my_margins = oracle_greedy(orc, base[:n], g["max_new"])
        low = next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
        assert mine[:low] == toks[:low], n
        np.testing.assert_allclose(my_margins[:low], margins[:low], atol=2e-3)
        compared += next((i for i, m in enumerate(my_margins) if m <= FLOOR), len(my_margins))
    # the GPU test's "at least 20 tokens compared" is cleared by the oracle alone
    assert compared >= 20 and compared == g["compared"]


def test_what_the_gpu_bound_is_worth(gold, toy):
    """the GPU test's seed and its six prefill prompts: the oracle with q_norm alone, or k_norm alone, left out is more than
    5 x BOUND x scale away - an engine that skipped either norm could not pass"""
    from _qwen3_ref import Qwen3Oracle
    dims, state, orc = toy
    seqs = [_synth.synth_token_batch(1, n, n, dims.vocab, seed=40 + n)[0] for n in (1, 2, 63, 64, 65, 300)]
    want = orc.last_logits(seqs)
    scale = float(np.abs(want).max())
    for m in ("q_norm", "k_norm"):
        less = {k: v for k, v in state.items() if not k.endswith(m + ".weight")}
        assert len(less) == len(state) - dims.n_layers
        off = float(np.abs(Qwen3Oracle(dims, less).last_logits(seqs) - want).max())
        print(f"oracle without {m}: {off:.2f} away = {off / (BOUND * scale):.1f} bounds")
        assert off > 5 * BOUND * scale, (m, off, scale)


def test_published_configs_parse_and_round_trip():
    a, b, c = (_synth.LlamaDims.from_hf_config(x) for x in (QWEN3_06B_CONFIG, QWEN3_4B_CONFIG, QWEN3_8B_CONFIG))
    assert b == _synth.QWEN3_4B == _synth.NAMED_DIMS["qwen3-4b"] and c == _synth.QWEN3_8B == _synth.NAMED_DIMS["qwen3-8b"]
    assert (a.hidden, a.n_heads, a.n_kv_heads, a.head_dim, a.intermediate, a.n_layers, a.tied_head) == (1024, 16, 8, 128, 3072, 28, True)
    assert b.n_heads * b.head_dim == 4096 and b.hidden == 2560 and b.tied_head and not c.tied_head and c.hidden == 4096
    for d in (a, b, c, _synth.TOY_QWEN3):
        assert d.qk_norm and not d.qkv_bias and not d.mistral and d.sliding_window == 0 and d.rope_scaling is None
        assert d.rope_theta == 1e6 and d.eps == 1e-6
        cfg = d.to_hf_config()
        assert cfg["model_type"] == "qwen3" and cfg["architectures"] == ["Qwen3ForCausalLM"] and cfg["head_dim"] == 128
        assert cfg["attention_bias"] is False and set(cfg["layer_types"]) == {"full_attention"}
        assert _synth.LlamaDims.from_hf_config(json.loads(json.dumps(cfg))) == d
    t = _synth.NAMED_DIMS["toy-qwen3"]
    assert t is _synth.TOY_QWEN3
    assert (t.vocab, t.hidden, t.n_heads, t.n_kv_heads, t.head_dim, t.intermediate, t.n_layers, t.tied_head, t.eps, t.rope_theta) == \
        (512, 256, 4, 2, 128, 512, 2, True, 1e-6, 1e6)
    # the new field is a default at the end: every other family's dims and tensor list are what they were
    assert [f.name for f in dataclasses.fields(_synth.LlamaDims)][-1] == "qk_norm"
    for name in ("toy-llama", "toy-qwen2", "toy-mistral", "toy-llama-hd64"):
        d = _synth.NAMED_DIMS[name]
        assert not d.qk_norm and not any("_norm.weight" in n for n, *_ in _synth.llama_tensor_specs(d))
        assert not _synth.LlamaDims.from_hf_config(d.to_hf_config()).qk_norm
    names = [n for n, *_ in _synth.llama_tensor_specs(_synth.TOY_QWEN3)]
    plain = [n for n, *_ in _synth.llama_tensor_specs(dataclasses.replace(_synth.TOY_QWEN3, qk_norm=False))]
    assert [n for n in names if "_norm.weight" not in n] == plain and len(names) == len(plain) + 4
    assert all(shape == (128,) and is_norm for n, shape, _, is_norm in _synth.llama_tensor_specs(_synth.TOY_QWEN3) if "_norm.weight" in n)


def test_refused_configs():
    ok = QWEN3_4B_CONFIG
    with pytest.raises(NotImplementedError, match="bias-free"):
        _synth.LlamaDims.from_hf_config({**ok, "attention_bias": True})
    with pytest.raises(NotImplementedError, match="use_sliding_window"):
        _synth.LlamaDims.from_hf_config({**ok, "use_sliding_window": True, "sliding_window": 4096})
    with pytest.raises(NotImplementedError, match="layer_types"):
        _synth.LlamaDims.from_hf_config({**ok, "layer_types": ["full_attention"] * 35 + ["sliding_attention"]})
    assert _synth.LlamaDims.from_hf_config({**ok, "layer_types": ["full_attention"] * 36}) == _synth.QWEN3_4B
    for scaling in ({"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}, {"type": "linear", "factor": 2.0}):
        with pytest.raises(NotImplementedError, match="rope scaling"):
            _synth.LlamaDims.from_hf_config({**ok, "rope_scaling": scaling})
    with pytest.raises(NotImplementedError):
        dataclasses.replace(_synth.TOY_QWEN3, qkv_bias=True).to_hf_config()
    with pytest.raises(NotImplementedError):
        dataclasses.replace(_synth.TOY_QWEN3, sliding_window=8, mistral=True).to_hf_config()


class _StubLib:
    """every rk_* entry returns RK_OK and is recorded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


def test_the_engine_binding_switches_the_head_norm_on(monkeypatch):
    from llmrankers import _engine
    header = open(os.path.join(REPO, "include", "rk_engine.h")).read()
    assert "int rk_llama_set_qk_norm(rk_engine* e, int on);" in header
    # appended behind out_n_cu, and the drafting step's g1 / live appended behind them: earlier callers' layout stays
    assert "out_heads_per_wg, out_n_cu;\n  const float* qk_norm; float qk_eps;\n  int g1; const int32_t* live;\n} rk_debug_attn_call;" in header
    assert [n for n, _ in _engine.RkDebugAttnCall._fields_][-5:] == ["out_n_cu", "qk_norm", "qk_eps", "g1", "live"]
    for dims in (_synth.TOY_QWEN3, _synth.QWEN3_8B, _synth.TOY_QWEN2, _synth.TOY_LLAMA, _synth.TOY_MISTRAL):
        lib = _StubLib()
        monkeypatch.setattr(_engine, "load_library", lambda lib=lib: lib)
        _engine.RkLlamaEngine(dims, device=0, max_tokens=64, max_seqs=2)
        names = [n for n, _ in lib.calls]
        assert names[0] == "rk_llama_create"
        assert [a[1] for n, a in lib.calls if n == "rk_llama_set_qk_norm"] == ([1] if dims.qk_norm else []), dims
        assert ("rk_llama_set_qkv_bias" in names) == dims.qkv_bias


class _StubEngine:
    made = []

    def __init__(self, dims, device=0, max_tokens=16384, max_seqs=16):
        self.dims, self.loaded = dims, 0
        _StubEngine.made.append(self)

    def load_state(self, tensors):
        self.loaded = sum(1 for _ in tensors)
        return self

    def close(self):
        pass


def _write(tmp_path, name, cfg, tok="tok_qwen"):
    from safetensors.numpy import save_file
    path = str(tmp_path / name)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({"model.norm.weight": np.ones(cfg["hidden_size"], np.float32)}, os.path.join(path, "model.safetensors"))
    for fn in os.listdir(os.path.join(GOLD, tok)):
        shutil.copy(os.path.join(GOLD, tok, fn), os.path.join(path, fn))
    return path


def test_who_accepts_a_qwen3_checkpoint(monkeypatch, tmp_path):
    """RankR1SetwiseLlmRanker and R1ListwiseLlmRanker (vLLM-served in the reference: any chat model) load it and the engine is asked
    for the head norm; the reference's setwise / pairwise / listwise rankers refuse it as they refuse every non-Llama decoder; what
    stays refused is refused before an engine is asked for"""
    from llmrankers import _runtime
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.listwise import ListwiseLlmRanker, R1ListwiseLlmRanker
    from llmrankers.pairwise import PairwiseLlmRanker
    from llmrankers.setwise import RankR1SetwiseLlmRanker, SetwiseLlmRanker
    from test_mistral_host import PROMPT
    monkeypatch.setattr(_runtime, "RkLlamaEngine", _StubEngine)
    del _StubEngine.made[:]
    tokdir, r1 = os.path.join(GOLD, "tok_qwen"), os.path.join(GOLD, "rankr1_prompt.toml")
    path = str(tmp_path / "toy-qwen3")
    _synth.write_checkpoint(path, {"dims": "toy-qwen3", "seed": 5}, tokdir)
    for build in (lambda: SetwiseLlmRanker(path, path, "cuda"), lambda: PairwiseLlmRanker(path, path, "cuda", method="heapsort"),
                  lambda: ListwiseLlmRanker(path, path, "cuda", 4, 2), lambda: LlamaRuntime(path, "cuda")):
        with pytest.raises(NotImplementedError, match="qwen3"):
            build()
    assert not _StubEngine.made
    a = RankR1SetwiseLlmRanker(path, r1, tokenizer_name_or_path=tokdir)
    b = R1ListwiseLlmRanker(path, tokdir, PROMPT, 4, 2)
    n_tensors = sum(1 for _ in _synth.llama_tensor_specs(_synth.TOY_QWEN3))
    for rk in (a, b):
        assert rk.llm.model_type == rk.model_type == "qwen3" and rk.llm.dims == _synth.TOY_QWEN3
        assert rk.llm.engine.dims.qk_norm and rk.llm.engine.loaded == n_tensors            # the four norm weights reach the engine
    # the prompt format is what it was: "[n] text" lines joined by a newline
    from llmrankers.rankers import SearchResult
    _, messages, _ = a._compare_prompts("q", [SearchResult("d1", None, "ocean river"), SearchResult("d2", None, "solar policy")], random.Random(0))
    assert messages[0][1]["content"].split("\n")[1:3] in (["[1] ocean river", "[2] solar policy"], ["[1] solar policy", "[2] ocean river"])
    # the published shapes construct too (stub engine: no weights are read beyond the file's)
    for i, cfg in enumerate((QWEN3_06B_CONFIG, QWEN3_4B_CONFIG, QWEN3_8B_CONFIG)):
        rt = LlamaRuntime(_write(tmp_path, f"pub{i}", cfg), "cuda", accept_model_types=("qwen3",))
        assert rt.engine.dims.qk_norm and rt.engine.dims.n_heads * rt.engine.dims.head_dim == cfg["num_attention_heads"] * 128
    # ---- refused, nothing created ----
    n = len(_StubEngine.made)
    big = _write(tmp_path, "h5120", {**QWEN3_8B_CONFIG, "hidden_size": 5120, "num_attention_heads": 40, "intermediate_size": 17408})   # Qwen3-14B
    with pytest.raises(NotImplementedError, match="head_dim 64 or 128") as ei:
        RankR1SetwiseLlmRanker(big, r1, tokenizer_name_or_path=tokdir)
    assert "hidden <= 4096" in str(ei.value)
    moe = _write(tmp_path, "moe", {**QWEN3_8B_CONFIG, "model_type": "qwen3_moe", "architectures": ["Qwen3MoeForCausalLM"], "num_experts": 128})
    with pytest.raises(NotImplementedError, match="qwen3_moe"):
        RankR1SetwiseLlmRanker(moe, r1, tokenizer_name_or_path=tokdir)
    for name, extra, msg in (("bias", {"attention_bias": True}, "bias-free"), ("win", {"use_sliding_window": True, "sliding_window": 4096}, "use_sliding_window"),
                             ("lt", {"layer_types": ["sliding_attention"] * 36}, "layer_types"),
                             ("yarn", {"rope_scaling": {"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}}, "rope scaling")):
        bad = _write(tmp_path, name, {**QWEN3_8B_CONFIG, **extra})
        for build in (lambda: RankR1SetwiseLlmRanker(bad, r1, tokenizer_name_or_path=tokdir), lambda: R1ListwiseLlmRanker(bad, tokdir, PROMPT, 4, 2)):
            with pytest.raises(NotImplementedError, match=msg):
                build()
    # the head norm with 64-wide heads: no such checkpoint, no such kernel (rk_engine_finalize refuses it too: tests/test_gpu_qwen3.py)
    hd64 = _write(tmp_path, "hd64", {**QWEN3_06B_CONFIG, "head_dim": 64})
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        RankR1SetwiseLlmRanker(hd64, r1, tokenizer_name_or_path=tokdir)
    assert len(_StubEngine.made) == n


def test_lora_on_a_head_norm_is_refused(tmp_path):
    """the norms are no LoRA targets: an adapter that names one hits merge_lora's refusal, as for every other non-projection tensor"""
    from safetensors.numpy import save_file
    from llmrankers._runtime import merge_lora
    adir = str(tmp_path / "adapter")
    spec = {"seed": 3, "r": 2, "lora_alpha": 4, "std": 0.05, "targets": ["q_proj"]}
    _synth.write_lora_adapter(adir, _synth.TOY_QWEN3, spec)
    state = _synth.synth_state_dict(_synth.TOY_QWEN3, seed=5)
    assert len(dict(merge_lora(iter(state.items()), adir))) == len(state)                 # a projection adapter merges as before
    from safetensors.numpy import load_file
    sd = load_file(os.path.join(adir, "adapter_model.safetensors"))
    sd["base_model.model.model.layers.0.self_attn.q_norm.lora_A.weight"] = np.zeros((2, 128), np.float32)
    sd["base_model.model.model.layers.0.self_attn.q_norm.lora_B.weight"] = np.zeros((128, 2), np.float32)
    save_file(sd, os.path.join(adir, "adapter_model.safetensors"))
    with pytest.raises(NotImplementedError, match="q_norm.*not one of the projections"):
        dict(merge_lora(iter(state.items()), adir))


def test_recorded_rankr1_cases_on_the_oracle(gold, tmp_path):
    """the recorded cases (HF's greedy generate under the build's RankR1SetwiseLlmRanker) through the same ranker on the numpy
    oracle: every compare's label and tokens, rankings, counters - fixture, oracle and host logic agree before a GPU is involved"""
    from safetensors.numpy import load_file
    from transformers import AutoTokenizer
    from _qwen3_ref import OracleQwen3GenRuntime
    from llmrankers._runtime import read_config, read_generation_settings
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    assert gold["min_margin"] > FLOOR == gold["floor"] and gold["bound"] == BOUND
    path = str(tmp_path / "toy-qwen3")
    _synth.write_checkpoint(path, gold["ckpt"], os.path.join(GOLD, gold["tokenizer"]))
    assert _synth.checkpoint_sha256(path) == gold["ckpt"]["sha256"]
    cfg = read_config(path)
    dims = _synth.LlamaDims.from_hf_config(cfg)
    assert dims == _synth.TOY_QWEN3
    rt = OracleQwen3GenRuntime(dims, load_file(os.path.join(path, "model.safetensors")), generation=read_generation_settings(path, cfg))
    assert rt.generation["eos_token_ids"] == [gold["model_eos"]]
    tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, gold["tokenizer"]))
    moved = False
    for case in gold["cases"]:
        rk = RankR1SetwiseLlmRanker.from_runtime(rt, tok, os.path.join(GOLD, gold["prompt_file"]), num_child=case["num_child"], k=case["k"],
                                                 method=case["method"], num_permutation=case["num_permutation"],
                                                 max_new_tokens=case["max_new_tokens"])
        outs, real = [], rk.compare
        rk.compare = lambda q, docs: outs.append(real(q, docs)) or outs[-1]
        random.seed(case["random_seed"])
        res = rk.rerank(case["query"], [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]])
        assert outs == [c["output"] for c in case["compares"]], case["qid"]
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"]
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"]
        assert case["counters"][2] == sum(len(r["new_ids"]) for c in case["compares"] for r in c["rows"])
        moved |= case["docids"] != [d for d, _ in case["docs"]]
    assert moved


def test_honest_orders_pass_the_kernel_judges():
    """tests/_qwen3_ref.py's judges on the GPU test's own fixtures with the honest fp32 orders standing in for the kernel (per-lane
    chains + butterfly, one chain, pairwise; rsqrt one ulp up and down; the rotation fused and not): all within HALF of C_ROWS - the
    constant tests/_rows_ref.py derived for rmsnorm and rope carries over to their composition - and a kernel that skipped the norm,
    took q's weights for k, or normed over the wrong half fails by orders of magnitude"""
    import _qwen3_ref as Q
    worst = 0.0
    for H, n_kv in ((4, 2), (7, 1), (3, 3)):
        p = Q.build_qkn(1100 + H, 5, H, n_kv, zero_head=(2, 1))
        for order in ("lanes", "chain", "pairwise"):
            for nudge in (0, 1, -1):
                worst = max(worst, Q.qkn_miss(p, Q.A.f16_sat(Q.qkn_emulated(p, order, nudge))))
        want, touched = Q.qkn_expected(p)
        assert not want[2, 128:256].any() and not np.isnan(want).any()        # the all-zero head: zeros, not NaN
        assert touched[:, :(H + n_kv) * 128].all() and not touched[:, (H + n_kv) * 128:].any()
        # mutants
        plain = Q.R.problem("rope", rows=p.rows, H=H, n_kv=n_kv, hd=128, ld=p.ld, max_pos=p.max_pos, pos=p.pos, cos=p.cos, sin=p.sin, bias=None, qkv=p.qkv)
        assert Q.qkn_miss(p, Q.A.f16_sat(Q.R.rope_emulated(plain)["out"])) > 100 * Q.R.C_ROWS            # no norm at all
        swapped = Q.SimpleNamespace(**{**p.__dict__, "w": np.concatenate([p.w[128:], p.w[:128]])})
        assert Q.qkn_miss(p, Q.A.f16_sat(Q.qkn_emulated(swapped))) > 100 * Q.R.C_ROWS                     # k normed with q's weight
        half = p.qkv.copy()
        half[:, 64:128] = 0                                                                                 # head 0's sum over one half only
        halfp = Q.SimpleNamespace(**{**p.__dict__, "qkv": half})
        got = Q.qkn_emulated(halfp)
        got[:, 64:128] = Q.qkn_emulated(p)[:, 64:128] * np.sqrt(2.0)
        assert Q.qkn_miss(p, Q.A.f16_sat(got)) > 100 * Q.R.C_ROWS
    print(f"honest orders: worst (error - half ulp) / E = {worst:.3f}")
    assert worst <= Q.R.C_ROWS / 2
    # the step's judge: the chain emulation of its own pieces passes, the un-normed step does not
    s = Q.build_qkn_step(5, 4, 2, [0, 1, 127, 128, 129, 300], 512)
    got = np.zeros((6, 512), np.float16)
    for it in Q.qkn_step_items(s, emul=True):
        got[it["out_rows"], it["out_col"]:it["out_col"] + 128] = Q.A.f16_sat(Q.A.emulate_item(it))
    assert Q.qkn_step_judge(s, got, "chain emulation") <= Q.A.C / 2
    with pytest.raises(AssertionError):
        Q.qkn_step_judge(s, Q.A.emulated(s)[:, :512], "the step without the norm")
