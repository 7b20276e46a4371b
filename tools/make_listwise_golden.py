#!/usr/bin/env python
"""Generate tests/golden/listwise_cases.json - runs ONLY where the reference and transformers are installed.

Runs the reference's ListwiseLlmRanker (ielab/llm-rankers, llmrankers/listwise.py; imported read-only the way
tools/make_goldens.py imports pointwise / setwise, with `openai` and `tiktoken` stubbed) on the CPU in fp32 over a toy T5
checkpoint, and records per case the settings, every compare (prompt length, generated ids, output string), the final docids
and scores and the three counters.

The checkpoint is `toy-gated-untied` with the digit tokens and EOS boosted in the head, so that generations are permutation-like
digit strings of varying length.  Its recipe and sha256 live in the fixture itself (not in ckpts.json, whose entries every suite
builds).  The seed is searched so that every greedy step of every recorded compare has a top-1 / top-2 logit margin above
FLOOR, measured with the fp32 oracle as tools/annotate_margins.py does (for `likelihood`: the smallest gap between neighbours of
the window's sorted label logits - the whole order is the output); the margins are recorded.

Usage:  python tools/make_listwise_golden.py --reference <checkout of ielab/llm-rankers> [--seeds 40]
"""
import argparse
import contextlib
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
from oracle.t5_numpy import T5Oracle          # noqa: E402

FLOOR = 5e-3                                  # the fp16 noise floor of the toy scale (tests/test_gpu_rerank.py: MARGIN_FLOOR)
DIGITS = list(range(185, 195))                # '0' .. '9' of tests/golden/tok
EOS = 1
WORDS = ("ocean river carbon energy solar policy market health vaccine protein neural network language model search query "
         "passage ranking climate water forest city history music science data system study result method patient school "
         "price trade law court food soil").split()
# (window, step, repeats, passages): the CLI default, the README's shape with two repeats, a walk that never reaches position 0
# ((n - w) % s != 0), and a window wider than the list
CASES = [(3, 1, 1, 6), (4, 2, 2, 8), (3, 2, 1, 6), (6, 2, 1, 4)]


def import_reference_listwise(ref):
    for m in ("openai", "tiktoken"):
        sys.modules.setdefault(m, types.ModuleType(m))
    from transformers import T5Tokenizer
    if not hasattr(T5Tokenizer, "batch_encode_plus"):
        T5Tokenizer.batch_encode_plus = lambda self, texts, **kw: self(texts, **kw)
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


def run_case(ref_rankers, ref_listwise, ckpt, q, scoring, oracle):
    with contextlib.redirect_stdout(io.StringIO()):
        ranker = ref_listwise.ListwiseLlmRanker(ckpt, None, "cpu", q["window_size"], q["step_size"], scoring=scoring,
                                                num_repeat=q["num_repeat"])
    compares = []
    llm = ranker.llm
    real_generate = llm.generate

    def generate(input_ids, *a, **kw):
        out = real_generate(input_ids, *a, **kw)
        ids = [int(t) for t in input_ids[0]]
        gen = [int(t) for t in out[0]]
        compares.append({"prompt_len": len(ids), "output_ids": gen, "margin": step_margins(oracle, ids, gen)})
        return out

    llm.generate = generate
    ranking = [ref_rankers.SearchResult(docid=d, score=None, text=t) for d, t in q["docs"]]
    before = [d.docid for d in ranking]
    orig_compare = ranker.compare

    def compare(query, docs):
        n0 = len(compares)
        out = orig_compare(query, docs)
        if scoring == "likelihood":
            ids = ranker.tokenizer(label_prompt(query, docs, ranker.CHARACTERS)).input_ids
            lg = oracle.score_last([ids], [int(t) for t in ranker.decoder_input_ids[0]],
                                   [int(t) for t in ranker.target_token_ids[:len(docs)]])[0]
            srt = np.sort(lg)
            compares.append({"prompt_len": len(ids), "margin": float(np.min(np.diff(srt))) if len(docs) > 1 else None})
        compares[n0]["output"] = out
        return out

    ranker.compare = compare
    with contextlib.redirect_stdout(io.StringIO()):
        res = ranker.rerank(q["query"], ranking)
    assert [d.docid for d in ranking] == before                  # the caller's list is not re-ordered
    return {"scoring": scoring, "qid": q["qid"], "query": q["query"], "docs": q["docs"], "window_size": q["window_size"],
            "step_size": q["step_size"], "num_repeat": q["num_repeat"], "compares": compares,
            "docids": [d.docid for d in res], "scores": [d.score for d in res],
            "counters": [ranker.total_compare, ranker.total_prompt_tokens, ranker.total_completion_tokens]}


def label_prompt(query, docs, chars):
    passages = "\n\n".join(f'Passage {chars[i]}: "{doc.text}"' for i, doc in enumerate(docs))
    return (f'Given a query "{query}", which of the following passages is the most relevant one to the query?\n\n' + passages
            + '\n\nOutput only the passage label of the most relevant passage:')


def step_margins(oracle, ids, gen):
    """fp32 oracle: top-1 minus top-2 logit at every greedy step of the recorded continuation (start token first)"""
    enc = oracle.encode(ids)
    out = []
    for t in range(1, len(gen)):
        lg = np.sort(oracle.decode(enc, gen[:t])[-1])
        out.append(float(lg[-1] - lg[-2]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (ielab/llm-rankers), read-only")
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--first-seed", type=int, default=100)
    args = ap.parse_args()
    import torch
    torch.set_num_threads(8)
    ref_rankers, ref_listwise = import_reference_listwise(os.path.abspath(args.reference))
    queries = make_queries(np.random.RandomState(77))
    tok_dir = os.path.join(GOLD, "tok")
    for seed in range(args.first_seed, args.first_seed + args.seeds):
        spec = {"dims": "toy-gated-untied", "seed": seed, "gain": 1.0, "boost_ids": DIGITS, "boost": 5.0,
                "boost2_ids": [EOS], "boost2": 4.0}
        with tempfile.TemporaryDirectory() as tmp:
            ckpt = os.path.join(tmp, "ckpt")
            _synth.write_checkpoint(ckpt, spec, tok_dir)
            spec["sha256"] = _synth.checkpoint_sha256(ckpt)
            from safetensors.numpy import load_file
            dims = _synth.NAMED_DIMS[spec["dims"]]
            oracle = T5Oracle(dims, load_file(os.path.join(ckpt, "model.safetensors")))
            cases = [run_case(ref_rankers, ref_listwise, ckpt, q, scoring, oracle)
                     for scoring in ("generation", "likelihood") for q in queries]
        gen = [c for case in cases if case["scoring"] == "generation" for c in case["compares"]]
        steps = [m for c in gen for m in c["margin"]]
        lik = [c["margin"] for case in cases if case["scoring"] == "likelihood" for c in case["compares"] if c["margin"] is not None]
        lens = [len(c["output_ids"]) for c in gen]
        worst = min(steps + lik) if steps + lik else 0.0
        stops = any(c["output_ids"][-1] == EOS for c in gen)
        full = any(len(c["output_ids"]) == 21 and c["output_ids"][-1] != EOS for c in gen)
        print(f"seed {seed}: {len(gen)} generations (lengths {min(lens)}..{max(lens)}), min margin {worst:.4f}, "
              f"EOS stop {stops}, full length {full}", flush=True)
        if worst > FLOOR and stops and full:
            out = {"about": "tools/make_listwise_golden.py: the reference's ListwiseLlmRanker, CPU fp32, on the checkpoint below",
                   "ckpt": spec, "tokenizer": "tok", "max_new": 20, "floor": FLOOR, "min_margin": worst, "cases": cases}
            with open(os.path.join(GOLD, "listwise_cases.json"), "w") as f:
                json.dump(out, f, indent=None, separators=(",", ":"))
            print("wrote", os.path.join(GOLD, "listwise_cases.json"))
            return
    raise SystemExit("no seed qualified")


if __name__ == "__main__":
    main()
