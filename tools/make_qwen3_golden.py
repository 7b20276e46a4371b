#!/usr/bin/env python
"""Generate tests/golden/qwen3_cases.json - runs ONLY where transformers (with Qwen3ForCausalLM) and torch are installed; CPU only.

Everything is recorded from HF's Qwen3ForCausalLM on `toy-qwen3` checkpoints written from their recipes:
  logits   fp32 last-position logits of three prompts (the pin of tests/_qwen3_ref.py: Qwen3Oracle);
  outlier  HF's own fp16-against-fp32 logit error with outlier norm weights (4 channels of every q_norm / k_norm weight x 20, as real
           checkpoints have): what the engine's error on the same model is held to;
  greedy   greedy continuations (4 new tokens) of the prefixes tests/test_gpu_qwen3.py decodes, with the top-1 / top-2 margin of every
           step.  The toy seed is searched until the margins clear FLOOR on at least MIN_COMPARED tokens and until leaving out q_norm
           alone, or k_norm alone, moves the logits of the GPU test's six prefill prompts by more than 5 x BOUND x scale - the conditions
           tests/test_qwen3_host.py asserts (the search asks for 6: a seed that is not on the edge);
  cases    the build's RankR1SetwiseLlmRanker over a runtime double whose `generate` is HF's greedy generate (fp32), on a checkpoint
           with boosted label and EOS rows and the tokenizer / prompt file of the Rank-R1 fixture: every compare (sha256 of each
           prompt's ids, the new ids, the margin of every step on the fp32 oracle, the label), the ranking, the counters.  Seeds are
           searched until every recorded step clears FLOOR, a completion matches the pattern and a case re-orders its documents.
Conditions fail, never relax.

Usage:  python tools/make_qwen3_golden.py [--seeds 40]
"""
import argparse
import hashlib
import json
import os
import random
import re
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO, os.path.join(REPO, "tests")]
from llmrankers import _synth                                     # noqa: E402
from _qwen3_ref import Qwen3Oracle, with_norm_outliers            # noqa: E402
from _llama_gen_stub import oracle_greedy                         # noqa: E402

FLOOR, BOUND = 5e-3, 4e-3                     # tests/test_gpu_rankr1.py
MIN_COMPARED = 20
TOY_GAIN = 2.0                                # hot weights (as the recorded checkpoints'): q / k heads whose rms is not 1, so the norm matters
LOGIT_PROMPTS = ((5, 71), (64, 72), (130, 73))                 # (length, synth_token_batch seed)
PREFILL_LENS = (1, 2, 63, 64, 65, 300)                          # tests/test_gpu_qwen3.py: prompt n has seed 40 + n
GREEDY_BASE_SEED, GREEDY_PREFIXES, GREEDY_NEW = 17, (1, 2, 3, 126, 127, 128, 129, 255, 256, 257), 4
WORDS = ("ocean river carbon energy solar policy market health vaccine protein neural network language model search query "
         "passage ranking climate water forest city history music science data system study result method patient school "
         "price trade law court food soil").split()
# (num_child, k, method, num_permutation, n_docs, max_new_tokens, python random seed)
CASES = [(3, 3, "heapsort", 1, 7, 12, 21), (4, 2, "bubblesort", 3, 6, 10, 22), (3, 2, "heapsort", 3, 8, 8, 23)]
RECIPES = [(3.0, 2.0), (2.5, 2.0), (3.5, 2.5), (3.0, 2.5), (4.0, 3.0), (2.0, 1.5)]   # (boost of the [1] .. [5] rows, boost of the EOS row)


def ids_sha256(ids):
    return hashlib.sha256(np.asarray(ids, dtype=np.int32).tobytes()).hexdigest()


def hf_model(path, dtype):
    import torch
    from transformers import AutoModelForCausalLM
    m = AutoModelForCausalLM.from_pretrained(path, torch_dtype=dtype).eval()
    assert type(m).__name__ == "Qwen3ForCausalLM", type(m).__name__
    return m


def hf_last(model, ids):
    import torch
    with torch.no_grad():
        return model(torch.tensor([[int(t) for t in ids]])).logits[0, -1].float().numpy()


def write_state(path, dims_name, state, tok_dir=None):
    from safetensors.numpy import save_file
    _synth.write_checkpoint(path, {"dims": dims_name, "seed": 1}, tok_dir)
    save_file({k: np.ascontiguousarray(v) for k, v in state.items()}, os.path.join(path, "model.safetensors"))


def toy_seed(first, n):
    """first seed whose oracle clears the tests' own conditions -> (seed, compared tokens, drop distances in bounds)"""
    dims = _synth.TOY_QWEN3
    base = _synth.synth_token_batch(1, 300, 300, dims.vocab, seed=GREEDY_BASE_SEED)[0]
    probe = [_synth.synth_token_batch(1, n_, n_, dims.vocab, seed=40 + n_)[0] for n_ in PREFILL_LENS]
    for seed in range(first, first + n):
        state = _synth.synth_state_dict(dims, seed=seed, gain=TOY_GAIN)
        orc = Qwen3Oracle(dims, state)
        want = orc.last_logits(probe)
        scale = float(np.abs(want).max())
        drops = []
        for m in ("q_norm", "k_norm"):
            less = {k: v for k, v in state.items() if not k.endswith(m + ".weight")}
            drops.append(float(np.abs(Qwen3Oracle(dims, less).last_logits(probe) - want).max()) / (BOUND * scale))
        compared = 0
        for n_ in GREEDY_PREFIXES:
            _, margins = oracle_greedy(orc, base[:n_], GREEDY_NEW)
            compared += next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
        print(f"toy seed {seed}: {compared} tokens clear the floor, without q_norm / k_norm {drops[0]:.1f} / {drops[1]:.1f} bounds away", flush=True)
        if compared >= MIN_COMPARED and min(drops) > 6.0:        # (the test asks for 5: a seed that is not on the edge)
            return seed, compared, drops
    raise SystemExit("no toy seed qualified")


def record_toy(tmp, seed):
    import torch
    dims = _synth.TOY_QWEN3
    state = _synth.synth_state_dict(dims, seed=seed, gain=TOY_GAIN)
    path = os.path.join(tmp, "toy")
    write_state(path, "toy-qwen3", state)
    m32 = hf_model(path, torch.float32)
    orc = Qwen3Oracle(dims, state)
    seqs = [_synth.synth_token_batch(1, n, n, dims.vocab, seed=s)[0] for n, s in LOGIT_PROMPTS]
    rows = [hf_last(m32, s) for s in seqs]
    for s, r in zip(seqs, rows):
        assert float(np.abs(orc.last_logits([s])[0] - r).max()) < 2e-4 * max(1.0, float(np.abs(r).max()))
    logits = {"dims": "toy-qwen3", "seed": seed, "gain": TOY_GAIN, "prompts": [list(p) for p in LOGIT_PROMPTS], "last_logits": [[float(v) for v in r] for r in rows]}
    base = _synth.synth_token_batch(1, 300, 300, dims.vocab, seed=GREEDY_BASE_SEED)[0]
    toks, margins = [], []
    for n in GREEDY_PREFIXES:
        cur, t, mg = [int(x) for x in base[:n]], [], []
        for _ in range(GREEDY_NEW):
            lg = hf_last(m32, cur)
            s = np.sort(lg)
            t.append(int(np.argmax(lg)))
            mg.append(float(s[-1] - s[-2]))
            cur.append(t[-1])
        toks.append(t)
        margins.append(mg)
    greedy = {"dims": "toy-qwen3", "seed": seed, "gain": TOY_GAIN, "base_seed": GREEDY_BASE_SEED, "prefix_lens": list(GREEDY_PREFIXES), "max_new": GREEDY_NEW,
              "tokens": toks, "margins": margins}
    # outlier norm weights: HF fp16 against HF fp32
    out_state = with_norm_outliers(state)
    opath = os.path.join(tmp, "outlier")
    write_state(opath, "toy-qwen3", out_state)
    o32, o16 = hf_model(opath, torch.float32), hf_model(opath, torch.float16)
    oorc = Qwen3Oracle(dims, out_state)
    oseqs = _synth.synth_token_batch(4, 40, 120, dims.vocab, seed=31)
    errs, scale = [], 0.0
    for s in oseqs:
        a, b = hf_last(o32, s), hf_last(o16, s)
        assert float(np.abs(a - oorc.last_logits([s])[0]).max()) < 1e-3 * float(np.abs(a).max())
        errs.append(float(np.abs(a - b).max()))
        scale = max(scale, float(np.abs(a).max()))
    outlier = {"dims": "toy-qwen3", "seed": seed, "gain": TOY_GAIN, "prompt_seed": 31, "prompt_lens": [len(s) for s in oseqs], "hf_fp16_max_err": max(errs),
               "hf_fp16_err_per_prompt": errs, "logit_scale": scale}
    return logits, greedy, outlier


class HFGenRuntime:
    """LlamaRuntime's `generate` on HF's greedy generate (fp32, CPU), with the -1 convention; every prompt is logged"""
    model_type = "qwen3"

    def __init__(self, path):
        import torch
        from llmrankers._runtime import read_config, read_generation_settings
        self.config = read_config(path)
        self.dims = _synth.LlamaDims.from_hf_config(self.config)
        self.generation = read_generation_settings(path, self.config)
        self.model = hf_model(path, torch.float32)
        self.log = []

    def generate(self, seqs, max_new, eos_ids, pad_id, max_total=0):
        import torch
        out = np.full((len(seqs), max_new), pad_id, dtype=np.int32)
        steps = 0
        for b, s in enumerate(seqs):
            ids = [int(t) for t in s]
            with torch.no_grad():
                full = self.model.generate(torch.tensor([ids]), do_sample=False, max_new_tokens=max_new, eos_token_id=list(eos_ids),
                                           pad_token_id=int(pad_id))[0].tolist()
            new = full[len(ids):]
            self.log.append({"prompt_ids": ids, "new_ids": new})
            out[b, :len(new)] = new
            steps = max(steps, len(new))
        out[:, steps:] = -1
        return out


def make_queries(rs):
    out = []
    for qi, (c, k, method, perm, n, max_new, seed) in enumerate(CASES):
        query = " ".join(rs.choice(WORDS, size=3))
        docs = [(f"d{qi}_{i}", " ".join(rs.choice(WORDS, size=int(rs.randint(5, 12))))) for i in range(n)]
        out.append({"qid": f"q{qi}", "query": query, "docs": docs, "num_child": c, "k": k, "method": method, "num_permutation": perm,
                    "max_new_tokens": max_new, "random_seed": seed})
    return out


def run_case(rt, tok, prompt_path, q):
    from llmrankers.rankers import SearchResult
    from llmrankers.setwise import RankR1SetwiseLlmRanker
    rk = RankR1SetwiseLlmRanker.from_runtime(rt, tok, prompt_path, num_child=q["num_child"], k=q["k"], method=q["method"],
                                             num_permutation=q["num_permutation"], max_new_tokens=q["max_new_tokens"])
    compares, real = [], rk.compare

    def compare(query, docs):
        n0 = len(rt.log)
        out = real(query, docs)
        compares.append({"output": out, "rows": [dict(r, completion=tok.decode(r["new_ids"], skip_special_tokens=True)) for r in rt.log[n0:]]})
        return out

    rk.compare = compare
    random.seed(q["random_seed"])
    res = rk.rerank(q["query"], [SearchResult(docid=d, score=None, text=t) for d, t in q["docs"]])
    return {**q, "compares": compares, "docids": [d.docid for d in res], "scores": [d.score for d in res],
            "counters": [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens]}


def add_margins(cases, dims, state, eos):
    """fp32 oracle: the margin of every recorded step (its arg-max must be HF's token) -> the smallest"""
    orc, worst = Qwen3Oracle(dims, state), np.inf
    for case in cases:
        for c in case["compares"]:
            for row in c["rows"]:
                toks, margins = oracle_greedy(orc, row["prompt_ids"], case["max_new_tokens"], (eos,))
                if toks != row["new_ids"]:
                    return -1.0
                row["margin"] = margins
                worst = min(worst, min(margins))
                if worst <= FLOOR:
                    return float(worst)
    return float(worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--first-seed", type=int, default=701)
    ap.add_argument("--first-toy-seed", type=int, default=929)
    args = ap.parse_args()
    import torch
    from safetensors.numpy import load_file
    from transformers import AutoTokenizer
    torch.set_num_threads(8)
    os.environ.setdefault("HF_HUB_OFFLINE", "1")
    tok_dir, prompt_path = os.path.join(GOLD, "tok_qwen"), os.path.join(GOLD, "rankr1_prompt.toml")
    tok = AutoTokenizer.from_pretrained(tok_dir)                    # (its own directory: see tests/test_rankr1_host.py)
    vocab = tok.get_vocab()
    dims = _synth.TOY_QWEN3
    eos = vocab["<|im_end|>"]
    assert eos == dims.eos_token_id
    seed, compared, drops = toy_seed(args.first_toy_seed, args.seeds)
    with tempfile.TemporaryDirectory() as tmp:
        logits, greedy, outlier = record_toy(tmp, seed)
    greedy["compared"], logits["without_norm_in_bounds"] = compared, {"q_norm": drops[0], "k_norm": drops[1]}
    with open(prompt_path, "rb") as f:
        import tomli
        pattern = tomli.load(f)["pattern"]
    queries = make_queries(np.random.RandomState(83))
    for ck_seed in range(args.first_seed, args.first_seed + args.seeds):
        for boost, boost_eos in RECIPES:
            spec = {"dims": "toy-qwen3", "seed": ck_seed, "gain": 2.0, "boost_ids": [vocab[f"[{i}]"] for i in range(1, 6)], "boost": boost,
                    "boost2_ids": [eos], "boost2": boost_eos, "tokenizer": "tok_qwen"}
            with tempfile.TemporaryDirectory() as tmp:
                ckpt = os.path.join(tmp, "toy-qwen3")
                _synth.write_checkpoint(ckpt, spec, tok_dir)
                spec["sha256"] = _synth.checkpoint_sha256(ckpt)
                state = load_file(os.path.join(ckpt, "model.safetensors"))
                rt = HFGenRuntime(ckpt)
                assert rt.dims == dims and rt.generation["eos_token_ids"] == [eos]
                cases = [run_case(rt, tok, prompt_path, q) for q in queries]
            rows = [(case, r) for case in cases for c in case["compares"] for r in c["rows"]]
            matched = sum(re.search(pattern, r["completion"].lower(), re.DOTALL) is not None for _, r in rows)
            stops = any(r["new_ids"][-1] == eos and len(r["new_ids"]) < case["max_new_tokens"] for case, r in rows)
            moved = any(case["docids"] != [d for d, _ in case["docs"]] for case in cases)
            print(f"seed {ck_seed} boost {boost}/{boost_eos}: {len(rows)} generations ({matched} match), EOS stop {stops}, re-orders {moved}", flush=True)
            if not (matched and matched < len(rows) and stops and moved):
                continue
            worst = add_margins(cases, dims, state, eos)
            print(f"    min margin {worst:.4f}", flush=True)
            if not worst > FLOOR:
                continue
            for case in cases:
                for c in case["compares"]:
                    for r in c["rows"]:
                        r["prompt_len"], r["prompt_sha256"] = len(r["prompt_ids"]), ids_sha256(r["prompt_ids"])
                        del r["prompt_ids"]
            out = {"about": "tools/make_qwen3_golden.py: HF Qwen3ForCausalLM (CPU) on toy-qwen3 checkpoints; cases: the build's "
                            "RankR1SetwiseLlmRanker over HF's greedy generate (fp32)",
                   "floor": FLOOR, "bound": BOUND, "logits": logits, "greedy": greedy, "outlier": outlier,
                   "ckpt": spec, "tokenizer": "tok_qwen", "prompt_file": "rankr1_prompt.toml", "model_eos": eos, "min_margin": worst, "cases": cases}
            with open(os.path.join(GOLD, "qwen3_cases.json"), "w") as f:
                json.dump(out, f, indent=None, separators=(",", ":"))
            print("wrote", os.path.join(GOLD, "qwen3_cases.json"))
            return
    raise SystemExit("no recipe / seed qualified")


if __name__ == "__main__":
    main()
