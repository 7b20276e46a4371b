"""Host logic of the Mistral family and the R1 listwise ranker, without a GPU: the config round trip, what the engine binding is
asked for (a stub library records the calls), which rankers accept a `mistral` checkpoint, R1ListwiseLlmRanker on a scripted
runtime, the CLI leg, the fp32 oracle with the window mask against HF's MistralForCausalLM, and the generated code of the windowed
kernels."""
import contextlib
import dataclasses
import importlib.util
import io
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLD, REPO
from llmrankers import _synth

ZEPHYR_CONFIG = {               # the published config's shape of castorini/rank_zephyr_7b_v1_full (no "head_dim" entry)
    "architectures": ["MistralForCausalLM"], "model_type": "mistral", "vocab_size": 32000, "hidden_size": 4096, "intermediate_size": 14336,
    "num_hidden_layers": 32, "num_attention_heads": 32, "num_key_value_heads": 8, "hidden_act": "silu", "rms_norm_eps": 1e-5,
    "rope_theta": 10000.0, "max_position_embeddings": 32768, "sliding_window": 4096, "tie_word_embeddings": False,
    "bos_token_id": 1, "eos_token_id": 2,
}
PROMPT = {"prompt_system": "you rank documents for a query", "prompt_user": "query {query}\nrank the {num} documents\n{docs}\nanswer with the order",
          "pattern": r"((?:\[[0-9]+\]\s*)+)"}


def test_config_round_trip():
    d = _synth.LlamaDims.from_hf_config(ZEPHYR_CONFIG)
    assert d == _synth.MISTRAL_7B == _synth.NAMED_DIMS["mistral-7b"]
    assert d.head_dim == 128 and d.sliding_window == 4096 and d.mistral and not d.qkv_bias and d.rope_scaling is None
    bare = {k: v for k, v in ZEPHYR_CONFIG.items() if k != "sliding_window"}
    for cfg in ({**ZEPHYR_CONFIG, "sliding_window": None, "head_dim": None}, bare):          # Mistral-7B-v0.2 / v0.3: no window
        n = _synth.LlamaDims.from_hf_config(cfg)
        assert n.sliding_window == 0 and n.mistral and n.head_dim == 128 and n == dataclasses.replace(d, sliding_window=0)
        out = n.to_hf_config()
        assert out["model_type"] == "mistral" and out["sliding_window"] is None and _synth.LlamaDims.from_hf_config(out) == n
    for name in ("mistral-7b", "toy-mistral", "toy-mistral-hd64"):
        dims = _synth.NAMED_DIMS[name]
        cfg = dims.to_hf_config()
        assert cfg["architectures"] == ["MistralForCausalLM"] and cfg["sliding_window"] == dims.sliding_window > 0
        assert _synth.LlamaDims.from_hf_config(cfg) == dims
        assert _synth.LlamaDims.from_hf_config(json.loads(json.dumps(cfg))) == dims
    a, b = _synth.NAMED_DIMS["toy-mistral"], _synth.NAMED_DIMS["toy-mistral-hd64"]
    assert dataclasses.replace(a, sliding_window=0, mistral=False) == _synth.TOY_LLAMA
    assert dataclasses.replace(b, sliding_window=0, mistral=False) == _synth.TOY_LLAMA_HD64
    # the new fields are defaults: a Llama config gives the dims it always gave, and a window outside Mistral is nobody's
    assert _synth.TOY_LLAMA.sliding_window == 0 and not _synth.TOY_LLAMA.mistral
    assert _synth.LlamaDims.from_hf_config({**_synth.TOY_LLAMA.to_hf_config(), "sliding_window": 8}) == _synth.TOY_LLAMA
    with pytest.raises(NotImplementedError):
        dataclasses.replace(_synth.TOY_LLAMA, sliding_window=8).to_hf_config()
    with pytest.raises(NotImplementedError, match="use_sliding_window"):                 # Qwen2's stays refused
        _synth.LlamaDims.from_hf_config({**_synth.TOY_QWEN2.to_hf_config(), "use_sliding_window": True, "sliding_window": 8})
    from llmrankers.listwise import permutation_order
    assert permutation_order('None', 5) == [0, 1, 2, 3, 4]


class _StubLib:
    """every rk_* entry returns RK_OK and is recorded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


def test_the_engine_binding_sets_the_window_only_when_there_is_one(monkeypatch):
    from llmrankers import _engine
    assert "rk_llama_set_sliding_window" in _engine.API if hasattr(_engine, "API") else True
    header = open(os.path.join(REPO, "include", "rk_engine.h")).read()
    assert "int rk_llama_set_sliding_window(rk_engine* e, int window);" in header
    for dims, want in ((_synth.TOY_MISTRAL, [64]), (dataclasses.replace(_synth.TOY_MISTRAL, sliding_window=5), [5]),
                       (dataclasses.replace(_synth.TOY_MISTRAL, sliding_window=0), []), (_synth.TOY_LLAMA, []), (_synth.TOY_QWEN2, [])):
        lib = _StubLib()
        monkeypatch.setattr(_engine, "load_library", lambda lib=lib: lib)
        _engine.RkLlamaEngine(dims, device=0, max_tokens=64, max_seqs=2)
        names = [n for n, _ in lib.calls]
        assert names[0] == "rk_llama_create"
        assert [a[1] for n, a in lib.calls if n == "rk_llama_set_sliding_window"] == want, dims
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


def _write(tmp_path, name, dims, tok):
    from safetensors.numpy import save_file
    path = str(tmp_path / name)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dims.to_hf_config(), f)
    save_file({"model.norm.weight": np.ones(dims.hidden, np.float32)}, os.path.join(path, "model.safetensors"))
    for fn in os.listdir(os.path.join(GOLD, tok)):
        shutil.copy(os.path.join(GOLD, tok, fn), os.path.join(path, fn))
    return path


def test_who_accepts_a_mistral_checkpoint(monkeypatch, tmp_path):
    """the reference's setwise / pairwise / listwise rankers refuse everything but llama and t5, ours too; the two vLLM-served
    rankers take any chat model: RankR1SetwiseLlmRanker and R1ListwiseLlmRanker load it, with its window"""
    from llmrankers import _runtime
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.listwise import ListwiseLlmRanker, R1ListwiseLlmRanker
    from llmrankers.pairwise import PairwiseLlmRanker
    from llmrankers.setwise import RankR1SetwiseLlmRanker, SetwiseLlmRanker
    monkeypatch.setattr(_runtime, "RkLlamaEngine", _StubEngine)
    del _StubEngine.made[:]
    dims = dataclasses.replace(_synth.TOY_MISTRAL, sliding_window=40, vocab=512)
    path = _write(tmp_path, "mistral", dims, "tok_llama")
    tokdir = os.path.join(GOLD, "tok_qwen")
    for build in (lambda: SetwiseLlmRanker(path, path, "cuda"), lambda: PairwiseLlmRanker(path, path, "cuda", method="heapsort"),
                  lambda: ListwiseLlmRanker(path, path, "cuda", 4, 2), lambda: LlamaRuntime(path, "cuda")):
        with pytest.raises(NotImplementedError, match="mistral"):
            build()
    assert not _StubEngine.made
    rt = LlamaRuntime(path, "cuda", accept_model_types=("mistral",))
    assert rt.model_type == "mistral" and rt.dims == dims and rt.engine.dims.sliding_window == 40
    a = RankR1SetwiseLlmRanker(path, os.path.join(GOLD, "rankr1_prompt.toml"), tokenizer_name_or_path=tokdir)
    b = R1ListwiseLlmRanker(path, tokdir, PROMPT, 4, 2)
    for rk in (a, b):
        assert rk.llm.model_type == "mistral" and rk.llm.engine.dims.sliding_window == 40 and rk.llm.engine.loaded == 1
    assert issubclass(R1ListwiseLlmRanker, ListwiseLlmRanker) and R1ListwiseLlmRanker.CHARACTERS == [f"[{i}]" for i in range(1, 21)]
    assert (b.window_size, b.step_size, b.num_repeat, b.max_new_tokens, b.lora_path, b.prompt["pattern"]) == (4, 2, 1, 2048, None, PROMPT["pattern"])
    import inspect
    assert list(inspect.signature(R1ListwiseLlmRanker.__init__).parameters)[1:] == [
        "model_name_or_path", "tokenizer_name_or_path", "prompt", "window_size", "step_size", "lora_path", "scoring", "num_repeat", "cache_dir",
        "device", "max_new_tokens"]
    for other in (_synth.TOY_LLAMA, dataclasses.replace(_synth.TOY_QWEN2, vocab=512)):         # ... and the families it took before
        p2 = _write(tmp_path, "other%d" % other.n_heads, other, "tok_llama")
        assert R1ListwiseLlmRanker(p2, tokdir, PROMPT, 4, 2).llm.dims == other
    t5 = str(tmp_path / "t5")
    os.makedirs(t5)
    with open(os.path.join(t5, "config.json"), "w") as f:
        json.dump(_synth.TOY_GATED_UNTIED.to_hf_config(), f)
    with pytest.raises(NotImplementedError):
        R1ListwiseLlmRanker(t5, tokdir, PROMPT, 4, 2)


# ---- R1ListwiseLlmRanker on a scripted runtime ------------------------------------------------------------------------------------
class _Scripted:
    """`generate` answers a prompt by the script: the text for the FIRST passage label order it finds is looked up by the prompt's
    passage words"""
    model_type = "mistral"

    def __init__(self, tok, answer, eos=2, pad=0):
        self.tok, self.answer, self.calls = tok, answer, []
        self.generation = {"eos_token_ids": [eos], "pad_token_id": pad, "max_new_tokens": None, "max_length": None, "do_sample": False}

    def generate(self, seqs, max_new, eos_ids, pad_id, max_total=0):
        self.calls.append((len(seqs), max_new, list(eos_ids), pad_id))
        rows = [self.answer(self.tok.decode(s)) for s in seqs]
        out = np.full((len(seqs), max_new), -1, dtype=np.int32)
        steps = max(len(r) for r in rows)
        for b, r in enumerate(rows):
            assert len(r) <= max_new
            out[b, :len(r)] = r
            out[b, len(r):steps] = pad_id
        return out


@pytest.fixture(scope="module")
def tok():
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(os.path.join(GOLD, "tok_qwen"))


def _docs(words):
    from llmrankers.rankers import SearchResult
    return [SearchResult(docid=f"d{i}", score=None, text=w) for i, w in enumerate(words)]


def test_r1_listwise_compare_counters_and_the_pattern(tok):
    from llmrankers.listwise import R1ListwiseLlmRanker
    eos = 2
    say = lambda text, end=True: tok.encode(text, add_special_tokens=False) + ([eos] if end else [])
    script = {"first": say("[2] > [1] > [3]"), "upper": say("[3] [1]"), "none": say("ranking"), "limit": say("[1] [2] [3] [1] [2] [3] [1] [2]", end=False),
              "junk": say("[2] [1]") + [0, 0, 0]}
    state = {"key": "first"}
    rt = _Scripted(tok, lambda prompt: script[state["key"]], eos=eos)
    rk = R1ListwiseLlmRanker.from_runtime(rt, tok, PROMPT, window_size=3, step_size=1, max_new_tokens=8)
    docs = _docs(["ranking", "query", "document"])
    ids = rk._chat_ids("relevant", docs)
    text = tok.decode(ids)
    assert "[1] ranking" in text and "[2] query" in text and "[3] document" in text and "assistant" in text.split("answer with the order")[-1]
    assert rk._chat_messages("q", docs)[0] == {"role": "system", "content": PROMPT["prompt_system"]}
    assert rk._chat_messages("q", docs)[1]["content"] == PROMPT["prompt_user"].format(query="q", num=3, docs="[1] ranking\n[2] query\n[3] document")
    assert rk.compare("relevant", docs) == "[2] [1] [3]"                       # group 1, stripped ('>' is not in this vocabulary)
    assert (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens) == (1, len(ids), len(script["first"]))   # the EOS counts
    assert rt.calls[-1] == (1, 8, [eos], 0)
    state["key"] = "none"
    assert rk.compare("relevant", docs) == 'None'
    state["key"] = "limit"                                                      # no EOS: the row ran to the limit
    assert rk.compare("relevant", docs) == "[1] [2] [3] [1] [2] [3] [1] [2]"
    state["key"] = "junk"                                                       # whatever follows the EOS that ended the row is not part of it
    assert rk.compare("relevant", docs) == "[2] [1]"
    want = len(script["first"]) + len(script["none"]) + 8 + 3
    assert (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens) == (4, 4 * len(ids), want)
    # the search runs on completion.lower()
    rk.prompt = {**PROMPT, "pattern": r"(ranking)"}
    rk.tokenizer = type("Upper", (), {"decode": lambda self, ids, skip_special_tokens=True: "RANKING", "apply_chat_template": tok.apply_chat_template})()
    assert rk.compare("relevant", docs) == "ranking"


def test_r1_listwise_window_walk_and_rerank_many(tok):
    """the inherited walk: windows from the bottom, a permutation re-orders its window, 'None' leaves it; rerank_many == one by one,
    in ONE generate call per step"""
    from llmrankers.listwise import R1ListwiseLlmRanker
    vocab_words = [w for w in ("ranking", "query", "document", "relevant", "think", "answer", "label", "most", "first", "then") if tok.encode(w, add_special_tokens=False) not in ([], [tok.unk_token_id]) and len(tok.encode(w, add_special_tokens=False)) == 1]
    assert len(vocab_words) >= 6
    eos = 2

    def answer(prompt):
        """reverse the window when its first passage is vocab_words[0]-ish, say nothing useful when it holds vocab_words[1] first"""
        lines = re.findall(r"\[(\d+)\] (\S+)", prompt)                         # (the word-level tokenizer decodes line breaks away)
        first = lines[0][1]
        if first == vocab_words[1]:
            return tok.encode("ranking", add_special_tokens=False) + [eos]
        order = " ".join(f"[{i}]" for i in range(len(lines), 0, -1))
        return tok.encode(order, add_special_tokens=False) + [eos]

    def fresh():
        rt = _Scripted(tok, answer, eos=eos)
        return R1ListwiseLlmRanker.from_runtime(rt, tok, PROMPT, window_size=3, step_size=2, num_repeat=1, max_new_tokens=8), rt

    items = [("relevant", _docs(vocab_words[:5])), ("query", _docs(vocab_words[1:6])), ("think", _docs(vocab_words[:3]))]
    solo = []
    for q, ranking in items:
        rk, rt = fresh()
        before = [d.docid for d in ranking]
        res = rk.rerank(q, ranking)
        assert [d.docid for d in ranking] == before and [d.score for d in res] == [-i for i in range(len(res))]
        assert sorted(d.docid for d in res) == sorted(before)
        assert rk.total_compare == len(rt.calls) == (2 if len(ranking) == 5 else 1)
        solo.append(([d.docid for d in res], (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens)))
    # 5 documents, windows [2:5] then [0:3]: both reversed by the script -> d0..d4 becomes [d4, d1, d0, d3, d2] unless a window says 'None'
    assert solo[0][0] == ["d4", "d1", "d0", "d3", "d2"]
    assert solo[2][0] == ["d2", "d1", "d0"]
    assert solo[1][0] != ["d0", "d1", "d2", "d3", "d4"] and solo[1][0][:3] == ["d0", "d1", "d4"]   # its top window starts with vocab_words[1]: 'None'
    rk, rt = fresh()
    results, counters = rk.rerank_many(items)
    assert [[d.docid for d in r] for r in results] == [s[0] for s in solo]
    assert [tuple(c) for c in counters] == [s[1] for s in solo]
    assert [c[0] for c in rt.calls] == [3, 2]                                  # the pending windows of all live queries per step


@pytest.fixture(scope="module")
def runmod():
    spec = importlib.util.spec_from_file_location("rk_run_r1_listwise", os.path.join(REPO, "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_builds_the_r1_listwise_ranker(runmod, monkeypatch):
    import llmrankers.listwise as lw
    made = {}

    class Stub:
        def __init__(self, **kw):
            made.update(kw, cls=type(self).__name__)

    class R1(Stub):
        pass

    class Plain(Stub):
        pass

    monkeypatch.setattr(lw, "R1ListwiseLlmRanker", R1)
    monkeypatch.setattr(lw, "ListwiseLlmRanker", Plain)
    parser, commands = runmod.build_parser()
    a = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "m", "--prompt_file", "p.toml", "--lora_path_or_name", "l", "--max_new_tokens", "77",
                                             "listwise", "--window_size", "20", "--step_size", "10", "--num_repeat", "2"])
    runmod.validate(a)
    assert isinstance(runmod.build_ranker(a), R1)
    assert (made["cls"], made["model_name_or_path"], made["tokenizer_name_or_path"], made["prompt"], made["lora_path"], made["max_new_tokens"],
            made["window_size"], made["step_size"], made["num_repeat"], made["device"]) == ("R1", "m", None, "p.toml", "l", 77, 20, 10, 2, "cuda")
    made.clear()                                                               # without --prompt_file nothing changes
    c = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "m", "listwise"])
    assert isinstance(runmod.build_ranker(c), Plain)
    assert sorted(made) == sorted(["cls", "model_name_or_path", "tokenizer_name_or_path", "device", "cache_dir", "window_size", "step_size", "scoring", "num_repeat"])


# ---- the reference's recorded cases (tools/make_r1_listwise_golden.py) on the oracle -------------------------------------------------
@pytest.fixture(scope="module")
def r1_gold(tmp_path_factory):
    """the recorded cases; the checkpoint and the adapter written from their recipes, sha256 asserted - once"""
    with open(os.path.join(GOLD, "r1_listwise_cases.json")) as f:
        gold = json.load(f)
    root = tmp_path_factory.mktemp("r1_listwise_gold")
    ckpt, adir = str(root / "ckpt"), str(root / "adapter")
    _synth.write_checkpoint(ckpt, gold["ckpt"], os.path.join(GOLD, gold["tokenizer"]))
    assert _synth.checkpoint_sha256(ckpt) == gold["ckpt"]["sha256"]
    assert _synth.write_lora_adapter(adir, _synth.NAMED_DIMS[gold["ckpt"]["dims"]], gold["adapter"]) == gold["adapter"]["sha256"]
    return gold, ckpt, adir


from _r1_listwise_gold import check_r1_case, run_r1_case   # noqa: E402


def test_recorded_r1_listwise_cases_on_the_oracle(r1_gold):
    """the reference's R1ListwiseLlmRanker cases through the build's ranker on the fp32 oracle with the window mask: prompt sha256s,
    new ids, completions, returned strings, rankings, scores, counters; rerank_many == one by one; and what the fixture must show"""
    from transformers import AutoTokenizer
    from _mistral_ref import OracleMistralGenRuntime
    from _qwen2_ref import merged_state
    from conftest import load_state
    from llmrankers._runtime import read_config, read_generation_settings
    from llmrankers.listwise import R1ListwiseLlmRanker
    from llmrankers.rankers import SearchResult
    gold, ckpt, _ = r1_gold
    dims = _synth.LlamaDims.from_hf_config(read_config(ckpt))
    W = gold["sliding_window"]
    assert dims == _synth.NAMED_DIMS["toy-mistral"] and dims.sliding_window == W > 0 and gold["min_margin"] > gold["floor"] == 5e-3
    from safetensors.numpy import load_file
    merged = merged_state(dims, load_file(os.path.join(ckpt, "model.safetensors")), gold["adapter"])
    rt = OracleMistralGenRuntime(dims, merged, generation=read_generation_settings(ckpt, read_config(ckpt)))
    assert rt.generation["eos_token_ids"] == [gold["model_eos"]]
    tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, gold["tokenizer"]))
    rows = [(case, c) for case in gold["cases"] for c in case["compares"]]
    eos = gold["model_eos"]
    assert any(c["prompt_len"] > W for _, c in rows)                                                         # a prompt longer than the window
    assert any(c["prompt_len"] <= W < c["prompt_len"] + len(c["new_ids"]) - 1 for _, c in rows)               # a decode that crosses it
    assert any(c["new_ids"][-1] == eos and len(c["new_ids"]) < case["max_new_tokens"] for case, c in rows)   # stops at EOS
    assert any(c["new_ids"][-1] != eos and len(c["new_ids"]) == case["max_new_tokens"] for case, c in rows)  # runs to the limit
    assert any(c["output"] == 'None' for _, c in rows) and any(case["docids"] != [d for d, _ in case["docs"]] for case in gold["cases"])
    assert all(min(c["margin"]) > gold["floor"] and len(c["margin"]) == len(c["new_ids"]) for _, c in rows)   # no step is excluded anywhere
    make = lambda case: R1ListwiseLlmRanker.from_runtime(rt, tok, gold["prompt"], window_size=case["window_size"], step_size=case["step_size"],
                                                         num_repeat=case["num_repeat"], max_new_tokens=case["max_new_tokens"])
    for case in gold["cases"]:
        rk = make(case)
        res, log = run_r1_case(rk, rt, case)
        check_r1_case(rk, res, log, case)
    same = [c for c in gold["cases"] if (c["window_size"], c["max_new_tokens"]) == (gold["cases"][0]["window_size"], gold["cases"][0]["max_new_tokens"])]
    rk = make(gold["cases"][0])
    items = [(c["query"], [SearchResult(docid=d, score=None, text=t) for d, t in c["docs"]]) for c in same + [gold["cases"][0]]]
    with contextlib.redirect_stdout(io.StringIO()):
        results, counters = rk.rerank_many(items)
    for c, r, n in zip(same + [gold["cases"][0]], results, counters):
        if (c["step_size"], c["num_repeat"]) == (gold["cases"][0]["step_size"], gold["cases"][0]["num_repeat"]):
            assert [d.docid for d in r] == c["docids"] and list(n) == c["counters"]
    # the fixture can see the feature: the recorded compare comes out otherwise under the plain Llama mask
    from _llama_gen_stub import oracle_greedy
    from oracle.llama_numpy import LlamaOracle
    w = gold["without_window"]
    case = gold["cases"][w["case"]]
    rk = make(case)
    _, log = run_r1_case(rk, rt, case)
    assert log[w["compare"]]["new_ids"] == case["compares"][w["compare"]]["new_ids"] != w["windowless_new_ids"]


# ---- the oracle against HF -----------------------------------------------------------------------------------------------------------
def test_mistral_oracle_vs_hf_fp32_at_a_toy_window():
    """MistralForCausalLM (fp32, CPU, eager attention) with sliding_window = 8 on 30 tokens: every position's logits; positions 0 .. 7
    are the window-less model's and position 8 is the first that is not"""
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    from _mistral_ref import MistralOracle
    from oracle.llama_numpy import LlamaOracle
    dims = dataclasses.replace(_synth.TOY_MISTRAL_HD64, sliding_window=8)
    state = _synth.synth_state_dict(dims, seed=929)
    cfg = transformers.MistralConfig(**{k: v for k, v in dims.to_hf_config().items() if k not in ("architectures", "model_type")})
    cfg._attn_implementation = "eager"
    model = transformers.MistralForCausalLM(cfg).eval()
    missing = model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in state.items()}, strict=False)
    assert not [k for k in missing.missing_keys if "rotary" not in k] and not missing.unexpected_keys
    ids = _synth.synth_token_batch(1, 30, 30, dims.vocab, seed=3)[0]
    with torch.no_grad():
        want = model(torch.tensor([list(map(int, ids))])).logits[0].numpy()
    orc = MistralOracle(dims, state)
    got = orc.hidden_states(ids) @ np.asarray(state["lm_head.weight"], np.float32).T
    assert np.abs(got - want).max() < 2e-4 * np.abs(want).max()
    plain = LlamaOracle(dims, state).hidden_states(ids) @ np.asarray(state["lm_head.weight"], np.float32).T
    assert np.abs(got[:8] - plain[:8]).max() < 1e-5 * np.abs(want).max()
    assert np.abs(got[8] - plain[8]).max() > 1e-3 * np.abs(want).max()
    assert np.array_equal(MistralOracle(dataclasses.replace(dims, sliding_window=0), state).hidden_states(ids), LlamaOracle(dims, state).hidden_states(ids))


# ---- generated code of the windowed kernels --------------------------------------------------------------------------------------------
def test_windowed_kernels_isa(tmp_path_factory):
    """the windowed entries keep what the plain kernels are held to (tests/test_isa_guards.py, tests/test_llama_listwise_host.py): the
    LDS-DMA prefill kernel spills nothing, fits two workgroups per CU, issues the prologue's chunk and the loop's next chunk only, and
    no compiler-placed vmcnt wait sits between its chunk bodies (four: diagonal / below x lower mask or none); the step and merge
    kernels of every (D, R, BIAS) have no scratch and wait on nobody"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_win") / "rk.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value", "-w",
                    os.path.join(REPO, "llm-rankers_amd", "csrc", "rk_engine.hip"), "-o", str(out)], check=True, timeout=600)
    lines = out.read_text().split("\n")

    def body(mangled):                       # (a name, or a prefix that ends in the template arguments: exactly one kernel)
        starts = [i for i, l in enumerate(lines) if re.match(re.escape(mangled) + r"\w*:", l)]
        assert len(starts) == 1, (mangled, [lines[i] for i in starts])
        start = starts[0]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        return lines[start:end + 1], "\n".join(lines[end:end + 400])

    for nw in (4, 8):
        code, meta = body(f"_Z22attn_causal_dma_kernelILi{nw}ELb1E")
        assert not any("scratch_" in l for l in code) and re.search(r"ScratchSize: 0\b", meta)
        assert int(re.search(r"NumVgprs: (\d+)", meta).group(1)) <= 256
        assert sum("global_load_lds_dwordx4" in l for l in code) == 2 * 32 // nw
        assert sum("v_mfma_f32_32x32x16_f16" in l for l in code) == 4 * 32
        first = next(i for i, l in enumerate(code) if "v_mfma" in l)
        last = max(i for i, l in enumerate(code) if "v_mfma" in l)
        for i in range(first, last):
            if "vmcnt" in code[i].split(";")[0]:
                assert "ASMSTART" in code[i - 1], f"compiler-placed vmcnt wait between the chunk bodies: {code[i].strip()}"
    code, meta = body("_Z23attn_causal_tile_kernelILi64ELb1E")
    assert not any("scratch_" in l for l in code) and re.search(r"ScratchSize: 0\b", meta)
    for d in (128, 64):
        for r in (1, 2, 4, 8) + ((7,) if d == 128 else ()):
            for bias in (0, 1):
                code, meta = body(f"_Z26attn_dec_cached_win_kernelILi{d}ELi{r}ELb{bias}EEv16LlamaDecAttnArgs")
                assert not any("scratch_" in l for l in code) and re.search(r"ScratchSize: 0\b", meta), (d, r, bias)
                assert not any("s_sleep" in l or "buffer_wbl2" in l for l in code)
        code, meta = body(f"_Z27attn_dec_combine_win_kernelILi{d}EEv16LlamaDecAttnArgs")
        assert not any("scratch_" in l for l in code) and re.search(r"ScratchSize: 0\b", meta), d
