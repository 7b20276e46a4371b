#!/usr/bin/env python
"""Generate tests/golden/llama_listwise_cases.json - runs ONLY where the reference and transformers are installed.

Runs the reference's ListwiseLlmRanker (ielab/llm-rankers, llmrankers/listwise.py, Llama branch; imported read-only as
tools/make_listwise_golden.py does, `openai` / `tiktoken` stubbed) on the CPU in fp32 over a `toy-llama` checkpoint with
tests/golden/tok_llama, and records per case the settings, every compare (prompt length and sha256 of the prompt ids, the new
ids, the output string, the fp32 oracle's top-1 / top-2 margin of every step), the final docids and scores, the three counters,
what `scoring='likelihood'` raises and what a prompt longer than the checkpoint's `max_length` raises.

With transformers 5 the reference's `apply_chat_template(..., return_tensors="pt")` returns a BatchEncoding and its
`input_ids.shape` fails: the ranker's tokenizer is wrapped to pass `return_dict=False` (the shim next to `batch_encode_plus`'s).

In tok_llama a digit is two tokens ([6, 188 + d]) and brackets are unknown-token pairs, so the head rows of the word-start
piece and of the digits 1-5 and the MODEL's EOS row (2; the tokenizer's EOS is 1) are boosted; recipe and seed are searched until
every recorded step's margin clears FLOOR, one row stops at EOS, one runs the full length and every (window, step, repeat)
shape with compares re-orders a window.  The recipe and its sha256 live in the fixture.

Usage:  python tools/make_llama_listwise_golden.py --reference <checkout of ielab/llm-rankers> [--seeds 40]
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
from llmrankers import _synth                 # noqa: E402
from oracle.llama_numpy import LlamaOracle    # noqa: E402

FLOOR = 5e-3                                  # the fp16 noise floor of the toy scale (tests/test_gpu_rerank.py: MARGIN_FLOOR)
MODEL_EOS = 2                                 # LlamaConfig's eos_token_id of the toy checkpoint (the tokenizer's EOS is 1)
WORD_START, DIGIT0 = 6, 188                   # tok_llama: a digit d is the pieces [6, 188 + d]
WORDS = ("ocean river carbon energy solar policy market health vaccine protein neural network language model search query "
         "passage ranking climate water forest city history music science data system study result method patient school "
         "price trade law court food soil").split()
CASES = [(3, 1, 1, 6), (4, 2, 2, 8), (3, 2, 1, 6), (6, 2, 1, 4)]   # (window, step, repeats, passages): make_listwise_golden.py's
RECIPES = [(5.0, 3.5), (4.0, 3.0), (5.0, 3.0), (6.0, 4.0), (4.5, 3.5)]   # (boost of [6, 189..193], boost of the EOS row)


def ids_sha256(ids):
    return hashlib.sha256(np.asarray(ids, dtype=np.int32).tobytes()).hexdigest()


def import_reference_listwise(ref):
    for m in ("openai", "tiktoken"):
        sys.modules.setdefault(m, types.ModuleType(m))
    for k in [k for k in sys.modules if k == "llmrankers" or k.startswith("llmrankers.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref] + [p for p in sys.path if p != os.path.join(REPO, "llm-rankers_amd")]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            import llmrankers.rankers as ref_rankers
            import llmrankers.listwise as ref_listwise
    finally:
        sys.path[:] = saved
    assert ref_listwise.__file__.startswith(os.path.abspath(ref)), ref_listwise.__file__
    return ref_rankers, ref_listwise


def make_queries(rs):
    out = []
    for qi, (w, s, r, n) in enumerate(CASES):
        query = " ".join(rs.choice(WORDS, size=3))
        docs = [(f"d{qi}_{i}", " ".join(rs.choice(WORDS, size=int(rs.randint(6, 18))))) for i in range(n)]
        out.append({"qid": f"q{qi}", "query": query, "window_size": w, "step_size": s, "num_repeat": r, "docs": docs})
    return out


def make_ranker(ref_listwise, ckpt, q, scoring):
    with contextlib.redirect_stdout(io.StringIO()):
        ranker = ref_listwise.ListwiseLlmRanker(ckpt, None, "cpu", q["window_size"], q["step_size"], scoring=scoring,
                                                num_repeat=q["num_repeat"])
    real = ranker.tokenizer.apply_chat_template
    ranker.tokenizer.apply_chat_template = lambda *a, **kw: real(*a, **{**kw, "return_dict": False})   # transformers >= 5
    ranker.total_compare = ranker.total_prompt_tokens = ranker.total_completion_tokens = 0   # (rerank() sets them; compare() alone needs them)
    return ranker


def step_margins(oracle, prompt, new):
    """fp32 oracle: top-1 minus top-2 logit at every greedy step of the recorded continuation; the oracle's own arg-max must
    be the recorded token"""
    out = []
    for t in range(len(new)):
        lg = oracle.last_logits([list(prompt) + list(new[:t])])[0]
        assert int(np.argmax(lg)) == new[t], "the oracle's greedy loop left the reference's generation"
        s = np.sort(lg)
        out.append(float(s[-1] - s[-2]))
    return out


def run_case(ref_rankers, ref_listwise, ckpt, q, oracle):
    ranker = make_ranker(ref_listwise, ckpt, q, "generation")
    compares = []
    real_generate = ranker.llm.generate

    def generate(input_ids, *a, **kw):
        out = real_generate(input_ids, *a, **kw)
        ids = [int(t) for t in input_ids[0]]
        new = [int(t) for t in out[0]][len(ids):]
        compares.append({"prompt_len": len(ids), "prompt_sha256": ids_sha256(ids), "new_ids": new, "margin": step_margins(oracle, ids, new)})
        return out

    ranker.llm.generate = generate
    ranking = [ref_rankers.SearchResult(docid=d, score=None, text=t) for d, t in q["docs"]]
    before = [d.docid for d in ranking]
    orig_compare = ranker.compare

    def compare(query, docs):
        n0 = len(compares)
        out = orig_compare(query, docs)
        compares[n0]["output"] = out
        return out

    ranker.compare = compare
    with contextlib.redirect_stdout(io.StringIO()):
        res = ranker.rerank(q["query"], ranking)
    assert [d.docid for d in ranking] == before                  # the caller's list is not re-ordered
    return {"scoring": "generation", "qid": q["qid"], "query": q["query"], "docs": q["docs"], "window_size": q["window_size"],
            "step_size": q["step_size"], "num_repeat": q["num_repeat"], "compares": compares,
            "docids": [d.docid for d in res], "scores": [d.score for d in res],
            "counters": [ranker.total_compare, ranker.total_prompt_tokens, ranker.total_completion_tokens]}


def raised_by(fn):
    try:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            fn()
    except Exception as exc:                                       # noqa: BLE001 - the type is what gets recorded
        return type(exc).__name__
    return None


def reorders(case):
    """a compare of the case changed its window's order (the digits it named are not 1..k in order)"""
    import re
    for c in case["compares"]:
        named = [int(w) for w in re.sub(r"[^0-9]", " ", c["output"]).split()]
        named = [k for k in named if 1 <= k <= case["window_size"]]
        if named and named[0] != 1:
            return True
    return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (ielab/llm-rankers), read-only")
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--first-seed", type=int, default=301)
    args = ap.parse_args()
    import torch
    torch.set_num_threads(8)
    os.environ.setdefault("HF_HUB_OFFLINE", "1")
    ref_rankers, ref_listwise = import_reference_listwise(os.path.abspath(args.reference))
    queries = make_queries(np.random.RandomState(77))
    tok_dir = os.path.join(GOLD, "tok_llama")
    from safetensors.numpy import load_file
    for seed in range(args.first_seed, args.first_seed + args.seeds):
        for boost, boost_eos in RECIPES:
            spec = {"dims": "toy-llama", "seed": seed, "gain": 2.0, "boost_ids": [WORD_START] + [DIGIT0 + d for d in range(1, 6)],
                    "boost": boost, "boost2_ids": [MODEL_EOS], "boost2": boost_eos, "tokenizer": "tok_llama"}
            with tempfile.TemporaryDirectory() as tmp:
                ckpt = os.path.join(tmp, "toy-llama")
                _synth.write_checkpoint(ckpt, spec, tok_dir)
                spec["sha256"] = _synth.checkpoint_sha256(ckpt)
                dims = _synth.NAMED_DIMS[spec["dims"]]
                oracle = LlamaOracle(dims, load_file(os.path.join(ckpt, "model.safetensors")))
                cases = [run_case(ref_rankers, ref_listwise, ckpt, q, oracle) for q in queries]
                comps = [c for case in cases for c in case["compares"]]
                steps = [m for c in comps for m in c["margin"]]
                worst = min(steps) if steps else 0.0
                stops = any(c["new_ids"] and c["new_ids"][-1] == MODEL_EOS for c in comps)
                full = any(len(c["new_ids"]) == 20 and c["new_ids"][-1] != MODEL_EOS for c in comps)
                moved = all(reorders(case) for case in cases if case["compares"])
                print(f"seed {seed} boost {boost}/{boost_eos}: {len(comps)} generations, min margin {worst:.4f}, EOS stop {stops}, "
                      f"full length {full}, every shape re-orders {moved}", flush=True)
                if not (worst > FLOOR and stops and full and moved):
                    continue
                q0 = queries[0]
                docs0 = [ref_rankers.SearchResult(docid=d, score=None, text=t) for d, t in q0["docs"]][:3]
                likelihood = raised_by(lambda: make_ranker(ref_listwise, ckpt, q0, "likelihood").compare(q0["query"], docs0))
                with open(os.path.join(ckpt, "generation_config.json"), "w") as f:
                    json.dump({"max_length": 16, "eos_token_id": MODEL_EOS}, f)
                too_long = raised_by(lambda: make_ranker(ref_listwise, ckpt, q0, "generation").compare(q0["query"], docs0))
            out = {"about": "tools/make_llama_listwise_golden.py: the reference's ListwiseLlmRanker (Llama branch), CPU fp32, on the checkpoint below",
                   "ckpt": spec, "tokenizer": "tok_llama", "max_new": 20, "model_eos": MODEL_EOS, "floor": FLOOR, "min_margin": worst,
                   "likelihood_raises": likelihood, "prompt_reaches_max_length_raises": too_long, "cases": cases}
            with open(os.path.join(GOLD, "llama_listwise_cases.json"), "w") as f:
                json.dump(out, f, indent=None, separators=(",", ":"))
            print("wrote", os.path.join(GOLD, "llama_listwise_cases.json"), "likelihood:", likelihood, "max_length:", too_long)
            return
    raise SystemExit("no recipe / seed qualified")


if __name__ == "__main__":
    main()
