#!/usr/bin/env python
"""Generate tests/golden/tok_qwen/, rankr1_prompt.toml and rankr1_cases.json - runs ONLY where the reference and transformers are
installed.

Runs the reference's RankR1SetwiseLlmRanker (ielab/llm-rankers, llmrankers/setwise.py; imported read-only, `vllm`, `openai`,
`tiktoken`, `toml` and `huggingface_hub` provided as stand-in modules) over a `toy-qwen2` checkpoint and a seeded rank-4 LoRA
adapter.  The stand-in `vllm.LLM.chat` runs HF's Qwen2ForCausalLM on the CPU in fp32, greedily, with the adapter merged into the
weights and the tokenizer's own chat template, and returns objects with `prompt_token_ids`, `outputs[0].token_ids` (the EOS that
ended a row included, as vLLM keeps it) and `.text` - so the reference's own compare / rerank code runs: its shuffles, regex, vote
and sort drivers.  Recorded per case: the settings, every compare (sha256 of each prompt's ids, the new ids, the completion, the
fp32 oracle's top-1 / top-2 margin of every step, the label returned), the final docids and scores and the three counters; plus
HF's own fp16 error on the outlier-bias model of tests/test_gpu_rankr1.py.

tok_qwen is a word-level tokenizer built here with the `tokenizers` library: the word list of the other generators, single tokens
for [1] .. [20], the think / answer tags, the ChatML markers and the role words, and a ChatML chat template written for this
fixture.  The prompt settings are this fixture's own (simpler than the published ones; the pattern still captures a [n] label).

Seeds and head-row boosts are searched until every recorded step's margin clears FLOOR - on the fp32 merged weights AND on their
fp16 rounding, which is what the engine holds - one completion stops at EOS, one runs to the limit, one does not match the
pattern, one case re-orders its documents and leaving the adapter out changes a recorded compare.  Conditions fail, never relax.

Usage:  python tools/make_rankr1_golden.py --reference <checkout of ielab/llm-rankers> [--seeds 40]
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO, os.path.join(REPO, "tests")]
from llmrankers import _synth                                     # noqa: E402
from _qwen2_ref import Qwen2Oracle, host_merge_lora, with_bias_outliers   # noqa: E402
from _llama_gen_stub import oracle_greedy                         # noqa: E402

FLOOR = 5e-3                                  # the fp16 noise floor of the toy scale (tests/test_gpu_rerank.py: MARGIN_FLOOR)
WORDS = ("ocean river carbon energy solar policy market health vaccine protein neural network language model search query "
         "passage ranking climate water forest city history music science data system study result method patient school "
         "price trade law court food soil").split()
PROMPT_WORDS = ("system user assistant you rank documents for a the which document is most relevant to think first then answer "
                "with label of in <think> </think> <answer> </answer>").split()
SPECIALS = ["<|endoftext|>", "<|im_start|>", "<|im_end|>"]     # ids 0, 1, 2: pad, (unused) bos, eos = the toy config's ids
LABELS = [f"[{i + 1}]" for i in range(20)]
CHAT_TEMPLATE = ("{% for message in messages %}{{ '<|im_start|>' + message['role'] + '\n' + message['content'] + '<|im_end|>' + '\n' }}"
                 "{% endfor %}{% if add_generation_prompt %}{{ '<|im_start|>assistant\n' }}{% endif %}")
PROMPT = {"prompt_system": "you rank documents for a query . think first then answer with the label of the most relevant document in <think> </think> <answer> </answer>",
          "prompt_user": "query {query}\n{docs}\nwhich document is the most relevant to the query",
          "pattern": r"(\[[0-9]+\])"}
ADAPTER = {"seed": 4242, "r": 4, "lora_alpha": 8, "std": 0.05, "targets": list(_synth.LORA_TARGETS)}
# (num_child, k, method, num_permutation, n_docs, max_new_tokens, python random seed)
CASES = [(3, 3, "heapsort", 1, 8, 16, 11), (5, 2, "heapsort", 3, 10, 12, 12), (3, 2, "bubblesort", 1, 6, 24, 13),
         (5, 3, "bubblesort", 3, 7, 10, 14), (3, 4, "heapsort", 3, 9, 8, 15)]
RECIPES = [(3.0, 2.0), (2.5, 2.0), (3.5, 2.5), (3.0, 2.5), (4.0, 3.0), (2.0, 1.5)]   # (boost of the [1] .. [5] rows, boost of the EOS row)


def ids_sha256(ids):
    return hashlib.sha256(np.asarray(ids, dtype=np.int32).tobytes()).hexdigest()


def make_tokenizer(path):
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    vocab = {}
    for w in SPECIALS + ["<unk>"] + LABELS + PROMPT_WORDS + WORDS + list(".,?:"):
        vocab.setdefault(w, len(vocab))
    assert len(vocab) <= 512, len(vocab)
    tk = Tokenizer(models.WordLevel(vocab=vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tok = PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="<unk>", pad_token="<|endoftext|>", eos_token="<|im_end|>",
                                  additional_special_tokens=["<|im_start|>"], chat_template=CHAT_TEMPLATE)
    tok.save_pretrained(path)
    return vocab


def write_prompt_toml(path):
    with open(path, "w") as f:
        f.write("# Rank-R1 prompt settings of the test fixture (tools/make_rankr1_golden.py)\n")
        for k, v in PROMPT.items():
            f.write(f"{k} = '{v}'\n" if k == "pattern" else f"{k} = {json.dumps(v)}\n")   # (pattern: a literal string, the backslashes stay)


class StandInLLM:
    """vllm.LLM for the reference's RankR1 ranker: HF Qwen2ForCausalLM, CPU fp32, greedy"""
    merged = None            # name -> fp32 array: the adapter-merged weights a lora_request selects
    log = None               # every chat() call appends one entry per conversation

    def __init__(self, model, tokenizer=None, enable_lora=False, max_lora_rank=32, **kw):
        import torch
        from transformers import AutoModelForCausalLM, AutoTokenizer
        self.tok = AutoTokenizer.from_pretrained(tokenizer or model)
        self.base = AutoModelForCausalLM.from_pretrained(model, torch_dtype=torch.float32).eval()
        self.lora = None
        if enable_lora:
            self.lora = AutoModelForCausalLM.from_pretrained(model, torch_dtype=torch.float32).eval()
            missing = self.lora.load_state_dict({k: torch.tensor(v) for k, v in StandInLLM.merged.items()}, strict=False)
            assert not missing.unexpected_keys and set(missing.missing_keys) <= {"lm_head.weight"}, missing
            self.lora.tie_weights()
        cfg = self.base.config
        self.eos = cfg.eos_token_id if isinstance(cfg.eos_token_id, list) else [cfg.eos_token_id]

    def chat(self, conversations, sampling_params=None, use_tqdm=False, lora_request=None):
        import torch
        model = self.lora if lora_request is not None else self.base
        outs = []
        for messages in conversations:
            ids = self.tok.apply_chat_template(messages, add_generation_prompt=True, tokenize=True)
            ids = [int(t) for t in (ids["input_ids"] if hasattr(ids, "keys") else ids)]
            with torch.no_grad():
                full = model.generate(torch.tensor([ids]), do_sample=False, max_new_tokens=sampling_params.max_tokens,
                                      eos_token_id=self.eos, pad_token_id=0)[0].tolist()
            new = full[len(ids):]
            text = self.tok.decode(new, skip_special_tokens=True)
            StandInLLM.log.append({"prompt_ids": ids, "new_ids": new, "completion": text})
            outs.append(types.SimpleNamespace(prompt_token_ids=ids, outputs=[types.SimpleNamespace(token_ids=new, text=text)]))
        return outs


def import_reference_setwise(ref):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    for m in ("openai", "tiktoken"):
        sys.modules.setdefault(m, types.ModuleType(m))
    import tomli

    def toml_load(path):
        with open(path, "rb") as f:
            return tomli.load(f)
    mod("toml", load=toml_load)
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
            import llmrankers.setwise as ref_setwise
    finally:
        sys.path[:] = saved
    assert ref_setwise.__file__.startswith(os.path.abspath(ref)), ref_setwise.__file__
    for k in [k for k in sys.modules if k == "llmrankers" or k.startswith("llmrankers.")]:
        del sys.modules[k]                                           # (our package again for whoever imports next)
    return ref_rankers, ref_setwise


def make_queries(rs):
    out = []
    for qi, (c, k, method, perm, n, max_new, seed) in enumerate(CASES):
        query = " ".join(rs.choice(WORDS, size=3))
        docs = [(f"d{qi}_{i}", " ".join(rs.choice(WORDS, size=int(rs.randint(5, 12))))) for i in range(n)]
        out.append({"qid": f"q{qi}", "query": query, "docs": docs, "num_child": c, "k": k, "method": method, "num_permutation": perm,
                    "max_new_tokens": max_new, "random_seed": seed})
    return out


def run_case(ref_rankers, ref_setwise, ckpt, adapter_dir, prompt_path, q, tok_dir):
    # the tokenizer comes from its OWN directory: next to a config.json with model_type qwen2, AutoTokenizer would re-read the
    # word-level tokenizer.json as Qwen's byte-level BPE and turn every word into <unk>-like single letters
    with contextlib.redirect_stdout(io.StringIO()):
        ranker = ref_setwise.RankR1SetwiseLlmRanker(ckpt, prompt_path, lora_name_or_path=adapter_dir, tokenizer_name_or_path=tok_dir,
                                                    num_child=q["num_child"], k=q["k"],
                                                    method=q["method"], num_permutation=q["num_permutation"])
    ranker.sampling_params.max_tokens = q["max_new_tokens"]        # the reference hard-codes 2 048; the toy cases are short
    compares, StandInLLM.log = [], []
    orig = ranker.compare

    def compare(query, docs):
        n0 = len(StandInLLM.log)
        out = orig(query, docs)
        compares.append({"output": out, "rows": StandInLLM.log[n0:]})
        return out

    ranker.compare = compare
    ranking = [ref_rankers.SearchResult(docid=d, score=None, text=t) for d, t in q["docs"]]
    ref_setwise.random.seed(q["random_seed"])
    with contextlib.redirect_stdout(io.StringIO()):
        res = ranker.rerank(q["query"], ranking)
    return {**q, "compares": compares, "docids": [d.docid for d in res], "scores": [d.score for d in res],
            "counters": [ranker.total_compare, ranker.total_prompt_tokens, ranker.total_completion_tokens]}


def check_prompts(cases, vocab):
    """The tokenizer did its work, or the fixture is worthless: every prompt holds the ChatML markers, the three role words, the
    labels [1] .. [n] of its window in order, no unknown token; the permutations of a compare are different prompts."""
    unk, start, end = vocab["<unk>"], vocab["<|im_start|>"], vocab["<|im_end|>"]
    roles = [vocab[w] for w in ("system", "user", "assistant")]
    label_ids = {vocab[l]: l for l in LABELS}
    distinct3 = False
    for case in cases:
        for c in case["compares"]:
            for row in c["rows"]:
                ids = row["prompt_ids"]
                assert unk not in ids, "unknown token in a prompt"
                assert ids.count(start) == 3 and ids.count(end) == 2 and ids[-2:] == [start, roles[2]], ids
                assert [ids[i + 1] for i, t in enumerate(ids[:-1]) if t == start] == roles, "role words"
                user = ids[ids.index(roles[1]):]
                labels = [label_ids[t] for t in user if t in label_ids]
                assert labels and labels == LABELS[:len(labels)], labels
            hashes = {ids_sha256(r["prompt_ids"]) for r in c["rows"]}
            distinct3 |= case["num_permutation"] == 3 and len(hashes) == 3
    assert distinct3, "no num_permutation = 3 compare with three distinct prompts"
    everything = [ids_sha256(r["prompt_ids"]) for case in cases for c in case["compares"] for r in c["rows"]]
    assert len(set(everything)) > len(everything) // 2, "prompts repeat across compares"


def fp16_state(state):
    return {k: (v.astype(np.float16).astype(np.float32) if v.ndim == 2 else v) for k, v in state.items()}


def add_margins(cases, dims, merged, eos):
    """fp32 oracle on the merged weights: the margin of every recorded step (its arg-max must be the recorded token); the same
    tokens must come out of the fp16-rounded merged weights (the engine's), each step clear of FLOOR there too -> smallest margin"""
    orc, orc16 = Qwen2Oracle(dims, merged), Qwen2Oracle(dims, fp16_state(merged))
    worst = np.inf
    for case in cases:
        for c in case["compares"]:
            for row in c["rows"]:
                toks, margins = oracle_greedy(orc, row["prompt_ids"], case["max_new_tokens"], (eos,))
                if toks != row["new_ids"]:
                    return -1.0
                toks16, margins16 = oracle_greedy(orc16, row["prompt_ids"], case["max_new_tokens"], (eos,))
                if toks16 != toks:
                    return -1.0
                row["margin"] = margins
                worst = min(worst, min(margins), min(margins16))
                if worst <= FLOOR:
                    return worst
    return float(worst)


def adapter_matters(cases, dims, base, eos):
    """first recorded compare whose tokens change when the adapter is left out (oracle on the base weights)"""
    orc = Qwen2Oracle(dims, base)
    for ci, case in enumerate(cases):
        for ki, c in enumerate(case["compares"]):
            for ri, row in enumerate(c["rows"]):
                toks, _ = oracle_greedy(orc, row["prompt_ids"], case["max_new_tokens"], (eos,))
                if toks != row["new_ids"]:
                    return {"case": ci, "compare": ki, "row": ri, "base_new_ids": toks}
    return None


def hf_fp16_error(tmp, tok_dir):
    """Check 3 of tests/test_gpu_rankr1.py: toy-qwen2 at seed 929 with outlier bias channels, 4 prompts of 40-120 tokens: HF's
    Qwen2ForCausalLM.half() on the CPU against fp32, max |logit difference| at the last position"""
    import torch
    from safetensors.numpy import save_file
    from transformers import AutoModelForCausalLM
    dims = _synth.TOY_QWEN2
    path = os.path.join(tmp, "outlier")
    _synth.write_checkpoint(path, {"dims": "toy-qwen2", "seed": 929}, tok_dir)
    state = with_bias_outliers(_synth.synth_state_dict(dims, seed=929))
    save_file({k: np.ascontiguousarray(v) for k, v in state.items()}, os.path.join(path, "model.safetensors"))
    seqs = _synth.synth_token_batch(4, 40, 120, dims.vocab, seed=31)
    m32 = AutoModelForCausalLM.from_pretrained(path, torch_dtype=torch.float32).eval()
    m16 = AutoModelForCausalLM.from_pretrained(path, torch_dtype=torch.float16).eval()
    errs, scale = [], 0.0
    orc = Qwen2Oracle(dims, state)
    for s in seqs:
        with torch.no_grad():
            a = m32(torch.tensor([s.tolist()])).logits[0, -1].numpy()
            b = m16(torch.tensor([s.tolist()])).logits[0, -1].float().numpy()
        assert float(np.abs(a - orc.last_logits([s])[0]).max()) < 1e-3 * float(np.abs(a).max())
        errs.append(float(np.abs(a - b).max()))
        scale = max(scale, float(np.abs(a).max()))
    return {"dims": "toy-qwen2", "seed": 929, "prompt_seed": 31, "prompt_lens": [len(s) for s in seqs], "hf_fp16_max_err": max(errs),
            "hf_fp16_err_per_prompt": errs, "logit_scale": scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (ielab/llm-rankers), read-only")
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--first-seed", type=int, default=501)
    args = ap.parse_args()
    import torch
    torch.set_num_threads(8)
    os.environ.setdefault("HF_HUB_OFFLINE", "1")
    tok_dir = os.path.join(GOLD, "tok_qwen")
    vocab = make_tokenizer(tok_dir)
    prompt_path = os.path.join(GOLD, "rankr1_prompt.toml")
    write_prompt_toml(prompt_path)
    ref_rankers, ref_setwise = import_reference_setwise(os.path.abspath(args.reference))
    queries = make_queries(np.random.RandomState(78))
    dims = _synth.NAMED_DIMS["toy-qwen2"]
    eos = vocab["<|im_end|>"]
    assert eos == dims.eos_token_id
    from safetensors.numpy import load_file
    for seed in range(args.first_seed, args.first_seed + args.seeds):
        for boost, boost_eos in RECIPES:
            spec = {"dims": "toy-qwen2", "seed": seed, "gain": 2.0, "boost_ids": [vocab[f"[{i}]"] for i in range(1, 6)], "boost": boost,
                    "boost2_ids": [eos], "boost2": boost_eos, "tokenizer": "tok_qwen"}
            with tempfile.TemporaryDirectory() as tmp:
                ckpt, adir = os.path.join(tmp, "toy-qwen2"), os.path.join(tmp, "adapter")
                _synth.write_checkpoint(ckpt, spec, tok_dir)
                spec["sha256"] = _synth.checkpoint_sha256(ckpt)
                adapter = dict(ADAPTER)
                adapter["sha256"] = _synth.write_lora_adapter(adir, dims, adapter)
                base = load_file(os.path.join(ckpt, "model.safetensors"))
                merged = host_merge_lora(base, _synth.synth_lora_tensors(dims, adapter), adapter["lora_alpha"] / adapter["r"])
                StandInLLM.merged = merged
                cases = [run_case(ref_rankers, ref_setwise, ckpt, adir, prompt_path, q, tok_dir) for q in queries]
                rows = [(case, r) for case in cases for c in case["compares"] for r in c["rows"]]
                check_prompts(cases, vocab)
                stops = any(r["new_ids"][-1] == eos and len(r["new_ids"]) < case["max_new_tokens"] for case, r in rows)
                full = any(r["new_ids"][-1] != eos and len(r["new_ids"]) == case["max_new_tokens"] for case, r in rows)
                import re
                nomatch = any(re.search(PROMPT["pattern"], r["completion"].lower(), re.DOTALL) is None for _, r in rows)
                matched = sum(re.search(PROMPT["pattern"], r["completion"].lower(), re.DOTALL) is not None for _, r in rows)
                moved = any(case["docids"] != [d for d, _ in case["docs"]] for case in cases)
                print(f"seed {seed} boost {boost}/{boost_eos}: {len(rows)} generations ({matched} match), EOS stop {stops}, full length {full}, "
                      f"no match {nomatch}, re-orders {moved}", flush=True)
                if not (stops and full and nomatch and moved):
                    continue
                worst = add_margins(cases, dims, merged, eos)
                print(f"    min margin {worst:.4f}", flush=True)
                if not worst > FLOOR:
                    continue
                without = adapter_matters(cases, dims, base, eos)
                print(f"    adapter left out changes: {without and (without['case'], without['compare'], without['row'])}", flush=True)
                if without is None:
                    continue
                outlier = hf_fp16_error(tmp, tok_dir)
            for case in cases:
                for c in case["compares"]:
                    for r in c["rows"]:
                        r["prompt_len"], r["prompt_sha256"] = len(r["prompt_ids"]), ids_sha256(r["prompt_ids"])
                        del r["prompt_ids"]
            out = {"about": "tools/make_rankr1_golden.py: the reference's RankR1SetwiseLlmRanker over a stand-in vllm (HF Qwen2ForCausalLM, CPU fp32, "
                            "adapter merged) on the checkpoint and adapter below",
                   "ckpt": spec, "adapter": adapter, "tokenizer": "tok_qwen", "prompt": PROMPT, "model_eos": eos, "floor": FLOOR,
                   "min_margin": worst, "without_adapter": without, "outlier": outlier, "cases": cases}
            with open(os.path.join(GOLD, "rankr1_cases.json"), "w") as f:
                json.dump(out, f, indent=None, separators=(",", ":"))
            print("wrote", os.path.join(GOLD, "rankr1_cases.json"))
            return
    raise SystemExit("no recipe / seed qualified")


if __name__ == "__main__":
    main()
