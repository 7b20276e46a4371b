"""Listwise ranker on a Llama checkpoint, host logic on the CPU: the reference's recorded cases (tests/golden/
llama_listwise_cases.json, written by tools/make_llama_listwise_golden.py) replayed over the numpy oracle behind the incremental
decoder's interface, the generation settings read from the checkpoint, the chat-template rule, what `likelihood` raises, the
lockstep form - and the compile-time guard on the cached decode attention kernel (no GPU: hipcc cross-compiles)."""
import copy
import hashlib
import json
import logging
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _llama_gen_stub import OracleLlamaGenRuntime
from conftest import GOLD, REPO

ERRORS = {"AttributeError": AttributeError, "ValueError": ValueError, "UnboundLocalError": UnboundLocalError,
          "NotImplementedError": NotImplementedError}


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "llama_listwise_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ckpt(gold, tmp_path_factory):
    """the fixture's toy checkpoint, regenerated from its recipe and checked against the recorded sha256"""
    from llmrankers import _synth
    from safetensors.numpy import load_file
    from transformers import AutoTokenizer
    path = str(tmp_path_factory.mktemp("llama_listwise") / "toy-llama")
    spec = gold["ckpt"]
    _synth.write_checkpoint(path, spec, os.path.join(GOLD, gold["tokenizer"]))
    assert _synth.checkpoint_sha256(path) == spec["sha256"], "regenerated weights differ from the golden recipe"
    dims = _synth.NAMED_DIMS[spec["dims"]]
    tok = AutoTokenizer.from_pretrained(path)
    tok.use_default_system_prompt = False
    return path, dims, load_file(os.path.join(path, "model.safetensors")), tok


def _ranking(case):
    from llmrankers.rankers import SearchResult
    return [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]]


def _ranker(rt, tok, case, **kw):
    from llmrankers.listwise import ListwiseLlmRanker
    return ListwiseLlmRanker.from_runtime(rt, tok, window_size=case["window_size"], step_size=case["step_size"],
                                          scoring=kw.get("scoring", case["scoring"]), num_repeat=case["num_repeat"])


def _sha(ids):
    return hashlib.sha256(np.asarray(ids, dtype=np.int32).tobytes()).hexdigest()


def test_fixture_covers_what_it_should(gold):
    comps = [c for case in gold["cases"] for c in case["compares"]]
    assert gold["min_margin"] > gold["floor"] == 5e-3
    assert min(m for c in comps for m in c["margin"]) == gold["min_margin"]
    assert any(c["new_ids"][-1] == gold["model_eos"] for c in comps)                       # an EOS stop ...
    assert any(len(c["new_ids"]) == gold["max_new"] and c["new_ids"][-1] != gold["model_eos"] for c in comps)   # ... and a full run
    for case in gold["cases"]:
        if case["compares"]:                                                               # every shape re-orders a window
            assert [d for d, _ in case["docs"]] != case["docids"], case["qid"]


def test_golden_cases_on_the_oracle(gold, ckpt):
    _, dims, state, tok = ckpt
    from llmrankers.listwise import ListwiseLlmRanker
    rt = OracleLlamaGenRuntime(dims, state)
    assert rt.generation["eos_token_ids"] == [gold["model_eos"]] and tok.eos_token_id != gold["model_eos"]   # the MODEL's EOS
    for case in gold["cases"]:
        rk = _ranker(rt, tok, case)
        seen, prompts = [], []
        real = rk.compare
        rk.compare = lambda q, docs: seen.append(real(q, docs)) or seen[-1]
        real_ids = ListwiseLlmRanker._chat_ids
        rk._chat_ids = lambda q, docs: prompts.append(real_ids(rk, q, docs)) or prompts[-1]
        ranking = _ranking(case)
        before = [d.docid for d in ranking]
        res = rk.rerank(case["query"], ranking)
        tag = case["qid"]
        assert [len(p) for p in prompts] == [c["prompt_len"] for c in case["compares"]], tag
        assert [_sha(p) for p in prompts] == [c["prompt_sha256"] for c in case["compares"]], tag
        assert seen == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [d.docid for d in ranking] == before, tag                       # the caller's list keeps its order
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag


def test_rerank_many_equals_one_at_a_time(gold, ckpt):
    _, dims, state, tok = ckpt
    rt = OracleLlamaGenRuntime(dims, state)
    base = next(c for c in gold["cases"] if c["window_size"] == 3 and c["step_size"] == 1)
    rk = _ranker(rt, tok, base)
    items = [(c["query"], _ranking(c)) for c in gold["cases"]]
    want, wcount = [], []
    for q, r in copy.deepcopy(items):
        want.append([(d.docid, d.score) for d in rk.rerank(q, r)])
        wcount.append((rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens))
    rt.calls.clear()
    got, counters = rk.rerank_many(items)
    assert [[(d.docid, d.score) for d in res] for res in got] == want
    assert counters == wcount
    assert max(rt.calls) > 1                                              # windows of several queries shared a call


def test_likelihood_raises_what_the_reference_raises(gold, ckpt):
    _, dims, state, tok = ckpt
    case = gold["cases"][0]
    rk = _ranker(OracleLlamaGenRuntime(dims, state), tok, case, scoring="likelihood")
    with pytest.raises(ERRORS[gold["likelihood_raises"]]):
        rk.compare(case["query"], _ranking(case)[:3])


def test_generation_settings_from_the_checkpoint(tmp_path, caplog):
    from llmrankers._runtime import generation_plan, read_generation_settings

    def settings(cfg, gc=None):
        d = tmp_path / f"c{len(os.listdir(tmp_path))}"
        d.mkdir()
        if gc is not None:
            (d / "generation_config.json").write_text(json.dumps(gc))
        return read_generation_settings(str(d), cfg)

    class RT:
        def __init__(self, g):
            self.generation = g

    s = settings({"eos_token_id": 2})
    assert s["eos_token_ids"] == [2] and s["pad_token_id"] == 2 and not s["do_sample"]
    assert generation_plan(RT(s), [700, 30]) == {"max_new": 20, "max_total": 0, "eos_ids": [2], "pad_id": 2}   # transformers >= 5
    s = settings({"eos_token_id": 2}, {"eos_token_id": [128001, 128009], "pad_token_id": 0, "max_new_tokens": 7})
    assert generation_plan(RT(s), [5]) == {"max_new": 7, "max_total": 0, "eos_ids": [128001, 128009], "pad_id": 0}
    s = settings({"eos_token_id": 2}, {"max_length": 4096, "max_new_tokens": 9})                                # HF's order
    assert generation_plan(RT(s), [5])["max_new"] == 9 and generation_plan(RT(s), [5])["max_total"] == 0
    s = settings({"eos_token_id": 2, "pad_token_id": 1}, {"max_length": 4096})
    assert generation_plan(RT(s), [700, 30]) == {"max_new": 4096 - 30, "max_total": 4096, "eos_ids": [2], "pad_id": 1}
    with pytest.raises(ValueError, match="max_length"):
        generation_plan(RT(s), [30, 4096])
    rt = RT(settings({"eos_token_id": 2}, {"do_sample": True, "temperature": 0.6}))
    with caplog.at_level(logging.WARNING, logger="llmrankers"):
        generation_plan(rt, [5])
        generation_plan(rt, [5])
    assert sum("greedily" in r.getMessage() for r in caplog.records) == 1                                        # ONE warning


def test_prompt_that_reaches_max_length_raises_what_hf_raises(gold, ckpt):
    _, dims, state, tok = ckpt
    case = gold["cases"][0]
    rt = OracleLlamaGenRuntime(dims, state, generation={"eos_token_ids": [2], "pad_token_id": 2, "max_new_tokens": None,
                                                        "max_length": 16, "do_sample": False})
    with pytest.raises(ERRORS[gold["prompt_reaches_max_length_raises"]]):
        _ranker(rt, tok, case).compare(case["query"], _ranking(case)[:3])


def test_max_length_ends_a_row_and_counts_like_hf(gold, ckpt):
    """max_length counts prompt + new tokens: the completion counter (which includes the prompt) never passes it"""
    _, dims, state, tok = ckpt
    case = gold["cases"][0]
    plen = case["compares"][0]["prompt_len"]
    rt = OracleLlamaGenRuntime(dims, state, generation={"eos_token_ids": [], "pad_token_id": 0, "max_new_tokens": None,
                                                        "max_length": plen + 3, "do_sample": False})
    rk = _ranker(rt, tok, case)
    docs = _ranking(case)[-case["window_size"]:]
    rk.compare(case["query"], docs)
    assert rk.total_prompt_tokens == plen and rk.total_completion_tokens == plen + 3


def test_vicuna_template_rule(gold, ckpt, monkeypatch):
    """the vicuna-v1.5 chat template is installed when 'v1.5' is in the model path (the reference's test), shared with setwise"""
    path, dims, state, _ = ckpt
    from llmrankers import _runtime, listwise, setwise
    monkeypatch.setattr(_runtime, "load_runtime", lambda p, device, cache_dir=None: OracleLlamaGenRuntime(dims, state))
    plain = listwise.ListwiseLlmRanker(path, None, "cuda", 3, 1)
    assert plain.tokenizer.chat_template != setwise.VICUNA_TEMPLATE and plain.tokenizer.use_default_system_prompt is False
    v15 = os.path.join(os.path.dirname(path), "toy-vicuna-v1.5")
    shutil.copytree(path, v15)
    rk = listwise.ListwiseLlmRanker(v15, None, "cuda", 3, 1)
    assert rk.tokenizer.chat_template == setwise.VICUNA_TEMPLATE
    case = gold["cases"][0]
    ids = rk._chat_ids(case["query"], _ranking(case)[:3])
    assert "ASSISTANT:" in rk.tokenizer.decode(ids) or len(ids) > 0


def test_cached_decode_attention_kernel_has_no_scratch(tmp_path_factory):
    """attn_dec_cached_kernel<D, R> keeps D / 8 K / V pieces (16 at D = 128, 8 at D = 64), the rotated queries and the
    accumulators of up to 8 query heads in registers: no spills (scratch), in every instantiation, and the merge kernel neither"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_llama_dec") / "rk.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value", "-w",
                    os.path.join(REPO, "llm-rankers_amd", "csrc", "rk_engine.hip"), "-o", str(out)], check=True, timeout=600)
    lines = out.read_text().split("\n")

    def body(mangled):
        start = next(i for i, l in enumerate(lines) if l.startswith(mangled + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        return lines[start:end + 1], "\n".join(lines[end:end + 400])
    for d, loads in ((128, 16), (64, 8)):                                     # a wave issues D / 16 K and D / 16 V loads
        for r in (1, 2, 4, 8):
            code, meta = body(f"_Z22attn_dec_cached_kernelILi{d}ELi{r}ELb0EEv16LlamaDecAttnArgs")
            assert not any("scratch_" in l for l in code), f"D = {d}, R = {r}: the cached decode attention kernel spills"
            assert re.search(r"ScratchSize: 0\b", meta), (d, r)
            assert sum("global_load_dwordx4" in l for l in code) >= loads      # K / V pieces straight to registers, 16 B per lane
            assert not any("s_sleep" in l or "buffer_wbl2" in l for l in code)   # nobody waits on another workgroup
        code, meta = body(f"_Z23attn_dec_combine_kernelILi{d}EEv16LlamaDecAttnArgs")
        assert not any("scratch_" in l for l in code) and re.search(r"ScratchSize: 0\b", meta), d
