#!/usr/bin/env python
"""Generate tests/golden/tok_r1list/ and r1_listwise_cases.json - runs ONLY where the reference and transformers are installed.

Runs the reference's R1ListwiseLlmRanker (ielab/llm-rankers, Rank-R1/run_listwise.py; imported read-only, `pyserini`, `vllm`,
`openai`, `tiktoken`, `toml` and `huggingface_hub` provided as stand-in modules) over a `toy-mistral` checkpoint - its SMALL
sliding_window left in the config - and a seeded rank-4 LoRA adapter.  The stand-in `vllm.LLM.chat` runs HF's MistralForCausalLM on
the CPU in fp32, greedily, with the adapter merged into the weights and the tokenizer's own chat template, and returns objects with
`prompt_token_ids`, `outputs[0].token_ids` (the EOS that ended a row included, as vLLM keeps it) and `.text` - so the reference's
own compare and its inherited rerank (the window walk, receive_permutation) run.  Recorded per case: the settings, every compare
(sha256 of the prompt ids, the new ids, the completion, the fp32 oracle's top-1 / top-2 margin of every step, the string returned),
the final docids and scores and the three counters.

tok_r1list is a word-level tokenizer built here with the `tokenizers` library (tok_qwen has no `>`): the word list of the other
generators, single tokens for [1] .. [20], `>` and the numbers 1 .. 20, the ChatML markers and the role words, and a ChatML chat template written for
this fixture.  The prompt settings are this fixture's own.

Seeds and head-row boosts are searched until: every recorded step's margin clears FLOOR - on the fp32 merged weights AND on their
fp16 rounding, which is what the engine holds -; one prompt is longer than the window; one decode crosses from inside the window to
beyond it; one completion stops at EOS, one runs to the limit, one does not match the pattern ('None'), one case re-orders its
documents; and running one recorded compare WITHOUT the window (the plain Llama mask) changes its tokens.  Conditions fail, never
relax.

Usage:  python tools/make_r1_listwise_golden.py --reference <checkout of ielab/llm-rankers> [--seeds 60]
"""
import argparse
import contextlib
import hashlib
import importlib.util
import io
import json
import os
import re
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO, os.path.join(REPO, "tests")]
from llmrankers import _synth                                     # noqa: E402
from oracle.llama_numpy import LlamaOracle                        # noqa: E402
from _mistral_ref import MistralOracle                            # noqa: E402
from _qwen2_ref import host_merge_lora                            # noqa: E402
from _llama_gen_stub import oracle_greedy                         # noqa: E402

FLOOR = 5e-3                                  # the fp16 noise floor of the toy scale (tests/test_gpu_rerank.py: MARGIN_FLOOR)
DIMS = "toy-mistral"
WORDS = ("ocean river carbon energy solar policy market health vaccine protein neural network language model search query "
         "passage ranking climate water forest city history music science data system study result method patient school "
         "price trade law court food soil").split()
PROMPT_WORDS = ("system user assistant you rank documents for a the by relevance to answer with identifiers in order most relevant first").split()
SPECIALS = ["<|endoftext|>", "<|im_start|>", "<|im_end|>"]     # ids 0, 1, 2: pad, (unused) bos, eos = the toy config's ids
LABELS = [f"[{i + 1}]" for i in range(20)]
CHAT_TEMPLATE = ("{% for message in messages %}{{ '<|im_start|>' + message['role'] + '\n' + message['content'] + '<|im_end|>' + '\n' }}"
                 "{% endfor %}{% if add_generation_prompt %}{{ '<|im_start|>assistant\n' }}{% endif %}")
PROMPT = {"prompt_system": "you rank documents for a query by relevance",
          "prompt_user": "query {query}\nrank the {num} documents\n{docs}\nanswer with the identifiers in order , the most relevant first",
          "pattern": r"(\[[0-9]+\](?: > \[[0-9]+\])*)"}
ADAPTER = {"seed": 4343, "r": 4, "lora_alpha": 8, "std": 0.05, "targets": list(_synth.LORA_TARGETS)}
# (window_size, step_size, num_repeat, n_docs, max_new_tokens)
CASES = [(3, 1, 1, 6, 12), (5, 2, 1, 9, 16), (4, 2, 2, 7, 10), (6, 3, 1, 10, 20), (3, 2, 1, 5, 8)]
RECIPES = [(3.0, 2.0), (2.5, 2.0), (3.5, 2.5), (3.0, 2.5), (4.0, 3.0), (2.0, 1.5)]   # (boost of the [1] .. [6] and `>` rows, boost of the EOS row)


def ids_sha256(ids):
    return hashlib.sha256(np.asarray(ids, dtype=np.int32).tobytes()).hexdigest()


def make_tokenizer(path):
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    vocab = {}
    for w in SPECIALS + ["<unk>"] + LABELS + [">"] + PROMPT_WORDS + WORDS + list(".,?:") + [str(n) for n in range(1, 21)]:
        vocab.setdefault(w, len(vocab))
    assert len(vocab) <= _synth.NAMED_DIMS[DIMS].vocab, len(vocab)
    tk = Tokenizer(models.WordLevel(vocab=vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tok = PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="<unk>", pad_token="<|endoftext|>", eos_token="<|im_end|>",
                                  additional_special_tokens=["<|im_start|>"], chat_template=CHAT_TEMPLATE)
    tok.save_pretrained(path)
    return vocab


class StandInLLM:
    """vllm.LLM for the reference's R1 listwise ranker: HF MistralForCausalLM (the config's sliding_window as it is), CPU fp32, greedy"""
    merged = None            # name -> fp32 array: the adapter-merged weights a lora_request selects
    log = None               # every chat() call appends one entry

    def __init__(self, model, tokenizer=None, enable_lora=False, max_lora_rank=32, **kw):
        import torch
        from transformers import AutoModelForCausalLM, AutoTokenizer
        self.tok = AutoTokenizer.from_pretrained(tokenizer or model)
        load = lambda: AutoModelForCausalLM.from_pretrained(model, torch_dtype=torch.float32, attn_implementation="eager").eval()
        self.base = load()
        assert type(self.base).__name__ == "MistralForCausalLM" and self.base.config.sliding_window == _synth.NAMED_DIMS[DIMS].sliding_window
        self.lora = None
        if enable_lora:
            self.lora = load()
            missing = self.lora.load_state_dict({k: torch.tensor(v) for k, v in StandInLLM.merged.items()}, strict=False)
            assert not missing.unexpected_keys and not [k for k in missing.missing_keys if "rotary" not in k], missing
        cfg = self.base.config
        self.eos = cfg.eos_token_id if isinstance(cfg.eos_token_id, list) else [cfg.eos_token_id]

    def chat(self, messages, sampling_params=None, use_tqdm=False, lora_request=None):
        import torch
        model = self.lora if lora_request is not None else self.base
        ids = self.tok.apply_chat_template(messages, add_generation_prompt=True, tokenize=True)
        ids = [int(t) for t in (ids["input_ids"] if hasattr(ids, "keys") else ids)]
        with torch.no_grad():
            full = model.generate(torch.tensor([ids]), do_sample=False, max_new_tokens=sampling_params.max_tokens,
                                  eos_token_id=self.eos, pad_token_id=0)[0].tolist()
        new = full[len(ids):]
        text = self.tok.decode(new, skip_special_tokens=True)
        StandInLLM.log.append({"prompt_ids": ids, "new_ids": new, "completion": text})
        return [types.SimpleNamespace(prompt_token_ids=ids, outputs=[types.SimpleNamespace(token_ids=new, text=text)])]


def import_reference_run_listwise(ref):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("tiktoken")
    mod("openai", OpenAI=object)
    import tomli

    def toml_load(path):
        with open(path, "rb") as f:
            return tomli.load(f)
    mod("toml", load=toml_load)
    mod("pyserini")
    mod("pyserini.search")
    mod("pyserini.search.lucene", LuceneSearcher=object)
    mod("pyserini.search._base", get_topics=lambda *a, **kw: {})
    mod("vllm", LLM=StandInLLM, SamplingParams=lambda temperature=0.0, max_tokens=16: types.SimpleNamespace(temperature=temperature, max_tokens=max_tokens))
    mod("vllm.lora")
    mod("vllm.lora.request", LoRARequest=lambda name, n, path: types.SimpleNamespace(name=name, path=path))
    hub = sys.modules.get("huggingface_hub")
    if hub is None or not hasattr(hub, "snapshot_download"):
        mod("huggingface_hub", snapshot_download=lambda *a, **kw: (_ for _ in ()).throw(RuntimeError("offline")))
    for k in [k for k in sys.modules if k == "llmrankers" or k.startswith("llmrankers.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref] + [p for p in sys.path if p != os.path.join(REPO, "llm-rankers_amd")]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            import llmrankers.rankers as ref_rankers
            spec = importlib.util.spec_from_file_location("ref_run_listwise", os.path.join(ref, "Rank-R1", "run_listwise.py"))
            run_listwise = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(run_listwise)
    finally:
        sys.path[:] = saved
    assert sys.modules["llmrankers.listwise"].__file__.startswith(os.path.abspath(ref))
    for k in [k for k in sys.modules if k == "llmrankers" or k.startswith("llmrankers.")]:
        del sys.modules[k]                                           # (our package again for whoever imports next)
    return ref_rankers, run_listwise


def make_queries(rs):
    out = []
    for qi, (w, s, rep, n, max_new) in enumerate(CASES):
        query = " ".join(rs.choice(WORDS, size=3))
        docs = [(f"d{qi}_{i}", " ".join(rs.choice(WORDS, size=int(rs.randint(5, 12))))) for i in range(n)]
        out.append({"qid": f"q{qi}", "query": query, "docs": docs, "window_size": w, "step_size": s, "num_repeat": rep, "max_new_tokens": max_new})
    return out


def run_case(ref_rankers, run_listwise, ckpt, adapter_dir, q, tok_dir):
    with contextlib.redirect_stdout(io.StringIO()):
        ranker = run_listwise.R1ListwiseLlmRanker(ckpt, tok_dir, PROMPT, q["window_size"], q["step_size"], lora_path=adapter_dir,
                                                  num_repeat=q["num_repeat"])
    ranker.sampling_params.max_tokens = q["max_new_tokens"]        # the reference hard-codes 2 048; the toy cases are short
    compares, StandInLLM.log = [], []
    orig = ranker.compare

    def compare(query, docs):
        out = orig(query, docs)
        compares.append({"output": out, **StandInLLM.log[-1]})
        return out

    ranker.compare = compare
    ranking = [ref_rankers.SearchResult(docid=d, score=None, text=t) for d, t in q["docs"]]
    with contextlib.redirect_stdout(io.StringIO()):
        res = ranker.rerank(q["query"], ranking)
    assert len(compares) == len(StandInLLM.log) == ranker.total_compare
    return {**q, "compares": compares, "docids": [d.docid for d in res], "scores": [d.score for d in res],
            "counters": [ranker.total_compare, ranker.total_prompt_tokens, ranker.total_completion_tokens]}


def check_prompts(cases, vocab):
    """every prompt holds the ChatML markers, the three role words, the labels [1] .. [n] of its window in order, no unknown token"""
    unk, start, end = vocab["<unk>"], vocab["<|im_start|>"], vocab["<|im_end|>"]
    roles = [vocab[w] for w in ("system", "user", "assistant")]
    label_ids = {vocab[l]: l for l in LABELS}
    for case in cases:
        for c in case["compares"]:
            ids = c["prompt_ids"]
            assert unk not in ids, "unknown token in a prompt"
            assert ids.count(start) == 3 and ids.count(end) == 2 and ids[-2:] == [start, roles[2]], ids
            assert [ids[i + 1] for i, t in enumerate(ids[:-1]) if t == start] == roles, "role words"
            labels = [label_ids[t] for t in ids[ids.index(roles[1]):] if t in label_ids]
            assert labels == LABELS[:min(case["window_size"], len(case["docs"]))], labels


def fp16_state(state):
    return {k: (v.astype(np.float16).astype(np.float32) if v.ndim == 2 else v) for k, v in state.items()}


def add_margins(cases, dims, merged, eos):
    """fp32 oracle (with the window) on the merged weights: the margin of every recorded step, whose arg-max must be the recorded
    token; the same tokens must come out of the fp16-rounded merged weights, each step clear of FLOOR there too -> smallest margin"""
    orc, orc16 = MistralOracle(dims, merged), MistralOracle(dims, fp16_state(merged))
    worst = np.inf
    for case in cases:
        for c in case["compares"]:
            toks, margins = oracle_greedy(orc, c["prompt_ids"], case["max_new_tokens"], (eos,))
            toks16, margins16 = oracle_greedy(orc16, c["prompt_ids"], case["max_new_tokens"], (eos,))
            if toks != c["new_ids"] or toks16 != toks:
                return -1.0
            c["margin"] = margins
            worst = min(worst, min(margins), min(margins16))
            if worst <= FLOOR:
                return worst
    return float(worst)


def window_matters(cases, dims, merged, eos):
    """first recorded compare whose tokens change when the window is left out (the plain Llama mask on the same weights)"""
    orc = LlamaOracle(dims, merged)
    for ci, case in enumerate(cases):
        for ki, c in enumerate(case["compares"]):
            toks, _ = oracle_greedy(orc, c["prompt_ids"], case["max_new_tokens"], (eos,))
            if toks != c["new_ids"]:
                return {"case": ci, "compare": ki, "windowless_new_ids": toks}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (ielab/llm-rankers), read-only")
    ap.add_argument("--seeds", type=int, default=60)
    ap.add_argument("--first-seed", type=int, default=601)
    args = ap.parse_args()
    import torch
    torch.set_num_threads(8)
    os.environ.setdefault("HF_HUB_OFFLINE", "1")
    tok_dir = os.path.join(GOLD, "tok_r1list")
    vocab = make_tokenizer(tok_dir)
    ref_rankers, run_listwise = import_reference_run_listwise(os.path.abspath(args.reference))
    queries = make_queries(np.random.RandomState(79))
    dims = _synth.NAMED_DIMS[DIMS]
    W, eos = dims.sliding_window, vocab["<|im_end|>"]
    assert eos == dims.eos_token_id and dims.mistral and W > 0
    from safetensors.numpy import load_file
    for seed in range(args.first_seed, args.first_seed + args.seeds):
        for boost, boost_eos in RECIPES:
            spec = {"dims": DIMS, "seed": seed, "gain": 2.0, "boost_ids": [vocab[f"[{i}]"] for i in range(1, 7)] + [vocab[">"]], "boost": boost,
                    "boost2_ids": [eos], "boost2": boost_eos, "tokenizer": "tok_r1list"}
            with tempfile.TemporaryDirectory() as tmp:
                ckpt, adir = os.path.join(tmp, DIMS), os.path.join(tmp, "adapter")
                _synth.write_checkpoint(ckpt, spec, tok_dir)
                spec["sha256"] = _synth.checkpoint_sha256(ckpt)
                adapter = dict(ADAPTER)
                adapter["sha256"] = _synth.write_lora_adapter(adir, dims, adapter)
                base = load_file(os.path.join(ckpt, "model.safetensors"))
                merged = host_merge_lora(base, _synth.synth_lora_tensors(dims, adapter), adapter["lora_alpha"] / adapter["r"])
                StandInLLM.merged = merged
                cases = [run_case(ref_rankers, run_listwise, ckpt, adir, q, tok_dir) for q in queries]
            rows = [(case, c) for case in cases for c in case["compares"]]
            check_prompts(cases, vocab)
            stops = any(c["new_ids"][-1] == eos and len(c["new_ids"]) < case["max_new_tokens"] for case, c in rows)
            full = any(c["new_ids"][-1] != eos and len(c["new_ids"]) == case["max_new_tokens"] for case, c in rows)
            nomatch = any(c["output"] == 'None' for _, c in rows)
            matched = sum(c["output"] != 'None' for _, c in rows)
            moved = any(case["docids"] != [d for d, _ in case["docs"]] for case in cases)
            longer = any(len(c["prompt_ids"]) > W for _, c in rows)
            crosses = any(len(c["prompt_ids"]) <= W < len(c["prompt_ids"]) + len(c["new_ids"]) - 1 for _, c in rows)
            for _, c in rows:
                m = re.search(PROMPT["pattern"], c["completion"].lower(), re.DOTALL)
                assert c["output"] == (m.group(1).strip() if m else 'None')
            print(f"seed {seed} boost {boost}/{boost_eos}: {len(rows)} compares ({matched} match), EOS stop {stops}, full length {full}, no match "
                  f"{nomatch}, re-orders {moved}, prompt > W {longer}, decode crosses W {crosses}; prompt lengths "
                  f"{sorted({len(c['prompt_ids']) for _, c in rows})}", flush=True)
            if not (stops and full and nomatch and moved and longer and crosses):
                continue
            worst = add_margins(cases, dims, merged, eos)
            print(f"    min margin {worst:.4f}", flush=True)
            if not worst > FLOOR:
                continue
            without = window_matters(cases, dims, merged, eos)
            print(f"    window left out changes: {without and (without['case'], without['compare'])}", flush=True)
            if without is None:
                continue
            for case in cases:
                for c in case["compares"]:
                    c["prompt_len"], c["prompt_sha256"] = len(c["prompt_ids"]), ids_sha256(c["prompt_ids"])
                    del c["prompt_ids"]
            out = {"about": "tools/make_r1_listwise_golden.py: the reference's R1ListwiseLlmRanker (Rank-R1/run_listwise.py) over a stand-in vllm (HF "
                            "MistralForCausalLM with its sliding_window, CPU fp32, adapter merged) on the checkpoint and adapter below",
                   "ckpt": spec, "adapter": adapter, "tokenizer": "tok_r1list", "prompt": PROMPT, "model_eos": eos, "sliding_window": W, "floor": FLOOR,
                   "min_margin": worst, "without_window": without, "cases": cases}
            with open(os.path.join(GOLD, "r1_listwise_cases.json"), "w") as f:
                json.dump(out, f, indent=None, separators=(",", ":"))
            print("wrote", os.path.join(GOLD, "r1_listwise_cases.json"))
            return
    raise SystemExit("no recipe / seed qualified")


if __name__ == "__main__":
    main()
