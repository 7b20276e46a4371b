"""Listwise ranker host logic on the CPU: the reference's recorded cases (tests/golden/listwise_cases.json, written by
tools/make_listwise_golden.py) replayed over the numpy oracle, permutation parsing, prompt truncation, the generation length and
the lockstep form.  No GPU: the oracle stands in for the engine (`generate` = the oracle's greedy continuation)."""
import copy
import json
import os

import numpy as np
import pytest

from _stub import OracleRuntime
from conftest import GOLD


class GenerateRuntime(OracleRuntime):
    """OracleRuntime with the engine runtime's `generate` (T5Runtime.generate has greedy's result and -1 convention)"""

    def __init__(self, dims, state):
        super().__init__(dims, state)
        self.calls = []

    def generate(self, seqs, dec_prefix, max_new, eos_id=1, pad_id=0):
        self.calls.append(len(seqs))
        return self.greedy(seqs, dec_prefix, max_new, eos_id, pad_id)

    def score(self, seqs, dec_prefix, out_ids):
        self.calls.append(len(seqs))
        return super().score(seqs, dec_prefix, out_ids)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "listwise_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def listwise_ckpt(gold, tmp_path_factory):
    """the fixture's toy checkpoint, regenerated from its recipe and checked against the recorded sha256"""
    from llmrankers import _synth
    from safetensors.numpy import load_file
    from transformers import T5Tokenizer
    path = str(tmp_path_factory.mktemp("listwise") / "ckpt")
    spec = gold["ckpt"]
    _synth.write_checkpoint(path, spec, os.path.join(GOLD, gold["tokenizer"]))
    assert _synth.checkpoint_sha256(path) == spec["sha256"], "regenerated listwise weights differ from the golden recipe"
    dims = _synth.NAMED_DIMS[spec["dims"]]
    return path, dims, load_file(os.path.join(path, "model.safetensors")), T5Tokenizer.from_pretrained(path)


def _ranking(case):
    from llmrankers.rankers import SearchResult
    return [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]]


def _ranker(rt, tok, case, max_new):
    from llmrankers.listwise import ListwiseLlmRanker
    return ListwiseLlmRanker.from_runtime(rt, tok, window_size=case["window_size"], step_size=case["step_size"],
                                          scoring=case["scoring"], num_repeat=case["num_repeat"], max_new=max_new)


def test_golden_cases_on_the_oracle(gold, listwise_ckpt):
    _, dims, state, tok = listwise_ckpt
    rt = GenerateRuntime(dims, state)
    assert {c["scoring"] for c in gold["cases"]} == {"generation", "likelihood"}
    for case in gold["cases"]:
        rk = _ranker(rt, tok, case, gold["max_new"])
        seen = []
        real = rk.compare
        rk.compare = lambda q, docs: seen.append(real(q, docs)) or seen[-1]
        ranking = _ranking(case)
        before = [d.docid for d in ranking]
        res = rk.rerank(case["query"], ranking)
        tag = (case["scoring"], case["qid"])
        assert seen == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [d.docid for d in ranking] == before, tag                       # the caller's list keeps its order
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag


def test_golden_generations_token_for_token(gold, listwise_ckpt):
    """every recorded generation: prompt length and the generated ids (start token included, cut at the row's EOS)"""
    _, dims, state, tok = listwise_ckpt
    from llmrankers.listwise import ListwiseLlmRanker
    rt = GenerateRuntime(dims, state)
    for case in gold["cases"]:
        if case["scoring"] != "generation":
            continue
        rk = _ranker(rt, tok, case, gold["max_new"])
        prompts = []
        real = ListwiseLlmRanker._compare_windows

        def spy(self, queries, doc_lists):
            prompts.extend(self._truncated_ids([self._permutation_prompt(q, d) for q, d in zip(queries, doc_lists)]))
            return real(self, queries, doc_lists)
        rk._compare_windows = spy.__get__(rk)
        rk.rerank(case["query"], _ranking(case))
        assert [len(p) for p in prompts] == [c["prompt_len"] for c in case["compares"]]
        for p, c in zip(prompts, case["compares"]):
            new = [int(t) for t in rt.greedy([p], [0], gold["max_new"], 1, 0)[0] if t >= 0]
            assert [0] + new == c["output_ids"]
    stops = [c["output_ids"][-1] == 1 for case in gold["cases"] for c in case["compares"] if "output_ids" in c]
    assert any(stops) and not all(stops)                                      # an EOS stop and a full-length run


@pytest.mark.parametrize("text,n,want", [
    ("", 3, [0, 1, 2]),
    ("no digits here", 3, [0, 1, 2]),
    ("[2] > [2] > [1]", 3, [1, 0, 2]),
    ("[3] > [9] > [0] > [1]", 3, [2, 0, 1]),
    ("[12] > [2] > [10]", 12, [11, 1, 9, 0, 2, 3, 4, 5, 6, 7, 8, 10]),
    ("605 'Yes'0505", 6, [0, 1, 2, 3, 4, 5]),
    ("2a3", 4, [1, 2, 0, 3]),
])
def test_permutation_parsing(text, n, want):
    from llmrankers.listwise import permutation_order
    assert permutation_order(text, n) == want


def test_prompt_truncation(listwise_ckpt):
    """`generation` prompts are tokenised with truncation at model_max_length, like the reference's tokenizer call"""
    path, dims, state, _ = listwise_ckpt
    from transformers import T5Tokenizer
    from llmrankers.listwise import ListwiseLlmRanker
    from llmrankers.rankers import SearchResult
    tok = T5Tokenizer.from_pretrained(path, model_max_length=40)
    rk = ListwiseLlmRanker.from_runtime(GenerateRuntime(dims, state), tok, window_size=3, step_size=1, max_new=4)
    docs = [SearchResult(f"d{i}", None, "ocean river carbon energy solar policy " * (i + 1)) for i in range(3)]
    text = rk._permutation_prompt("water", docs)
    ids = rk._truncated_ids([text])[0]
    assert ids == list(tok(text, truncation=True)["input_ids"]) and len(ids) == 40
    assert len(tok(text)["input_ids"]) > 40


def test_max_new_matches_hf_generate(listwise_ckpt, tmp_path):
    """the resolved generation length is what the reference's bare `generate(input_ids)` produces for the checkpoint"""
    import torch
    from transformers import T5ForConditionalGeneration
    from llmrankers import _synth
    from llmrankers.listwise import resolve_max_new
    from conftest import REPO
    with open(os.path.join(GOLD, "ckpts.json")) as f:
        spec = json.load(f)["ckpt_gated_untied"]           # (random weights: no early EOS from this prompt)
    path = str(tmp_path / "ck")
    _synth.write_checkpoint(path, spec, os.path.join(GOLD, "tok"))
    model = T5ForConditionalGeneration.from_pretrained(path, torch_dtype=torch.float32).eval()
    out = model.generate(torch.tensor([[5, 6, 7, 8, 9, 1]]))[0].tolist()
    assert 1 not in out[1:]
    assert len(out) == 1 + resolve_max_new(path)
    with open(os.path.join(path, "generation_config.json"), "w") as f:
        json.dump({"decoder_start_token_id": 0, "eos_token_id": 1, "pad_token_id": 0, "max_new_tokens": 7}, f)
    assert resolve_max_new(path) == 7


def test_rerank_many_equals_one_at_a_time(gold, listwise_ckpt):
    _, dims, state, tok = listwise_ckpt
    for scoring in ("generation", "likelihood"):
        cases = [c for c in gold["cases"] if c["scoring"] == scoring and c["window_size"] == 3 and c["step_size"] == 1]
        rt = GenerateRuntime(dims, state)
        rk = _ranker(rt, tok, {**cases[0], "num_repeat": 1}, gold["max_new"])
        items = [(c["query"], _ranking(c)) for c in gold["cases"] if c["scoring"] == scoring]
        want, wcount = [], []
        for q, r in copy.deepcopy(items):
            want.append([(d.docid, d.score) for d in rk.rerank(q, r)])
            wcount.append((rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens))
        rt.calls.clear()
        before = [[d.docid for d in r] for _, r in items]
        got, counters = rk.rerank_many(items)
        assert [[(d.docid, d.score) for d in res] for res in got] == want
        assert counters == wcount
        assert [[d.docid for d in r] for _, r in items] == before
        assert max(rt.calls) > 1                                              # windows of several queries shared a call


def test_llama_runtime_is_refused(listwise_ckpt):
    from llmrankers.listwise import ListwiseLlmRanker

    class Llama:
        model_type = "llama"
    with pytest.raises(NotImplementedError, match="Llama"):
        ListwiseLlmRanker.from_runtime(Llama(), listwise_ckpt[3])


def test_listwise_cli_kind(tmp_path):
    from llmrankers._batching import default_queries_per_call
    assert default_queries_per_call("listwise", 100) > 1


def test_run_py_listwise_with_openai_key_is_refused():
    import importlib.util
    from conftest import REPO
    spec = importlib.util.spec_from_file_location("rk_run_lw", os.path.join(REPO, "run.py"))
    runmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(runmod)
    parser, commands = runmod.build_parser()
    args = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "x", "--run_path", "r", "--save_path", "s",
                                                "--openai_key", "k", "listwise", "--window_size", "4"])
    with pytest.raises(NotImplementedError, match="OpenAI"):
        runmod.build_ranker(args)
