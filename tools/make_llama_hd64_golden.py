#!/usr/bin/env python
"""Generate tests/golden/llama_hd64_ckpts.json and tests/golden/llama_hd64_cases.json - runs ONLY where the reference and
transformers are installed.

The reference's rankers (ielab/llm-rankers, imported read-only as the other make_*_golden.py tools do) run on the CPU in fp32 over
checkpoints with 64-WIDE heads written from recipes (no weights are committed):

  ckpt_llama_hd64           `toy-llama-hd64` + tests/golden/tok_llama, the 23 label rows boosted as ckpt_llama's are:
                            SetwiseLlmRanker (Llama branch, `generation`, heapsort and bubblesort) and PairwiseLlmRanker (heapsort and
                            bubblesort), every compare logged as tools/make_goldens.py logs them
  ckpt_llama_hd64_listwise  the same dims with the word-start, digit and EOS rows boosted (tools/make_llama_listwise_golden.py's
                            recipe and functions): ListwiseLlmRanker
  ckpt_qwen2_hd64           `toy-qwen2-hd64` + tests/golden/tok_qwen + a seeded LoRA adapter: RankR1SetwiseLlmRanker over the stand-in
                            vllm of tools/make_rankr1_golden.py (its functions, its prompt file)

Margin rule (the project's four-times rule, tools/annotate_margins.py's method: the fp32 oracle replays every decision): a case is
kept only if the top-1 / top-2 margin of EVERY greedy step of every compare is at least 4 x FLOOR = 2e-2.  Seeds and recipes are
searched until every shape of a family has a kept case; a shape that cannot be filled ends the tool with an error.

Usage:  python tools/make_llama_hd64_golden.py --reference <checkout of ielab/llm-rankers> [--seeds 12]
"""
import argparse
import contextlib
import io
import json
import os
import random
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]
from llmrankers import _synth                  # noqa: E402
from oracle.llama_numpy import LlamaOracle     # noqa: E402
# (the sibling tools and the test helpers import OUR package: before the reference's takes the name `llmrankers`)
import make_llama_listwise_golden as L         # noqa: E402
import make_rankr1_golden as R                 # noqa: E402
from _qwen2_ref import host_merge_lora         # noqa: E402

FLOOR = 5e-3
KEEP = 4 * FLOOR                               # the four-times rule
WORDS = ("ocean river carbon energy solar policy market health vaccine protein neural network language model search query "
         "passage ranking climate water forest city history music science data system study result method patient school "
         "price trade law court food soil").split()
SETWISE_SHAPES = [("heapsort", 3, 5, 12), ("bubblesort", 4, 4, 10)]          # (method, num_child, k, passages)
PAIRWISE_SHAPES = [("heapsort", 4, 9), ("bubblesort", 3, 7)]                 # (method, k, passages)
LISTWISE_SHAPES = [(3, 1, 1, 6), (4, 2, 2, 8)]                               # (window, step, repeats, passages)


def rand_text(rs, lo, hi):
    return " ".join(rs.choice(WORDS, size=int(rs.randint(lo, hi + 1))))


def import_reference(ref):
    """the reference's rankers / setwise / pairwise modules under their own package name, ours restored afterwards"""
    import types
    for m in ("openai", "tiktoken"):
        sys.modules.setdefault(m, types.ModuleType(m))
    for k in [k for k in sys.modules if k == "llmrankers" or k.startswith("llmrankers.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref] + [p for p in sys.path if p != os.path.join(REPO, "llm-rankers_amd")]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            import llmrankers.rankers as ref_rankers
            import llmrankers.setwise as ref_setwise
            import llmrankers.pairwise as ref_pairwise
    finally:
        sys.path[:] = saved
    assert ref_setwise.__file__.startswith(os.path.abspath(ref)), ref_setwise.__file__
    return ref_rankers, ref_setwise, ref_pairwise


def hook(rk, oracle, margins, log, ids_of):
    """every compare logged; every generate call's prompt replayed through the fp32 oracle: its arg-max must be the reference's
    token, its top-1 / top-2 margin is recorded"""
    real_tpl = rk.tokenizer.apply_chat_template
    rk.tokenizer.apply_chat_template = lambda *a, **kw: real_tpl(*a, **{**kw, "return_dict": False})   # transformers >= 5
    real_gen = rk.llm.generate

    def generate(input_ids, *a, **kw):
        out = real_gen(input_ids, *a, **kw)
        for b in range(input_ids.shape[0]):                         # (pairwise: both orderings in one call, equal lengths, no padding)
            ids = [int(t) for t in input_ids[b]]
            new = [int(t) for t in out[b]][len(ids):]
            assert len(new) == 1, new
            lg = oracle.last_logits([ids])[0]
            s = np.sort(lg)
            # a step where the fp32 oracle and the reference's torch fp32 disagree is a coin-flip: margin 0, the case is dropped
            margins.append(float(s[-1] - s[-2]) if int(np.argmax(lg)) == new[0] else 0.0)
        return out

    rk.llm.generate = generate
    orig = rk.compare

    def logged(query, docs):
        out = orig(query, docs)
        log.append([ids_of(docs), out])
        return out

    rk.compare = logged


def one_token_cases(ref_rankers, ref_setwise, ref_pairwise, ckpt, oracle):
    """setwise and pairwise cases of ckpt_llama_hd64 -> (cases with their min_margin, shapes with a kept case)"""
    cases, sink = [], io.StringIO()
    rs = np.random.RandomState(164)
    queries = [rand_text(rs, 3, 8) for _ in range(3)]
    pool = [rand_text(rs, 8, 30) for _ in range(40)]
    for kind, shapes in (("setwise", SETWISE_SHAPES), ("pairwise", PAIRWISE_SHAPES)):
        for si, shape in enumerate(shapes):
            margins, log = [], []
            with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
                if kind == "setwise":
                    method, c, k, n = shape
                    rk = ref_setwise.SetwiseLlmRanker(ckpt, ckpt, device="cpu", num_child=c, k=k, scoring="generation", method=method, num_permutation=1)
                    hook(rk, oracle, margins, log, lambda docs: [d.docid for d in docs])
                else:
                    method, k, n = shape
                    rk = ref_pairwise.PairwiseLlmRanker(ckpt, ckpt, device="cpu", method=method, batch_size=2, k=k)
                    hook(rk, oracle, margins, log, lambda docs: list(docs))
                for qi, q in enumerate(queries):
                    ranking = [ref_rankers.SearchResult(docid=f"{kind[0].upper()}{si}{7 * qi + i}", score=float(100 - i), text=pool[(7 * qi + 3 * si + i) % 40])
                               for i in range(n)]
                    inp = [[r.docid, r.score, r.text] for r in ranking]
                    random.seed(929)
                    del log[:], margins[:]
                    try:
                        res = rk.rerank(q, ranking)
                    except IndexError:                              # the reference's bubblesort on an out-of-window label: not a case here
                        continue
                    case = {"kind": f"{kind}-llama", "ckpt": "ckpt_llama_hd64", "shape": si, "scoring": "generation", "method": method, "k": k, "query": q,
                            "input": inp, "result": [[r.docid, r.score] for r in res], "compares": list(log),
                            "caller_list_after": [r.docid for r in ranking],
                            "counters": [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens], "min_margin": min(margins)}
                    if kind == "setwise":
                        case.update(num_child=c, num_permutation=1)
                    cases.append(case)
    kept = [c for c in cases if c["min_margin"] >= KEEP]
    filled = {(c["kind"], c["shape"]) for c in kept}
    return kept, filled


def listwise_cases(ref, seeds, first_seed, tok_dir):
    from safetensors.numpy import load_file
    ref_rankers, ref_listwise = L.import_reference_listwise(ref)
    queries = [q for q in L.make_queries(np.random.RandomState(77)) if (q["window_size"], q["step_size"], q["num_repeat"], len(q["docs"])) in LISTWISE_SHAPES]
    assert len(queries) == len(LISTWISE_SHAPES)
    for seed in range(first_seed, first_seed + seeds):
        for boost, boost_eos in L.RECIPES:
            spec = {"dims": "toy-llama-hd64", "seed": seed, "gain": 2.0, "boost_ids": [L.WORD_START] + [L.DIGIT0 + d for d in range(1, 6)],
                    "boost": boost, "boost2_ids": [L.MODEL_EOS], "boost2": boost_eos, "tokenizer": "tok_llama"}
            with tempfile.TemporaryDirectory() as tmp:
                ckpt = os.path.join(tmp, "toy-llama-hd64")
                _synth.write_checkpoint(ckpt, spec, tok_dir)
                spec["sha256"] = _synth.checkpoint_sha256(ckpt)
                oracle = LlamaOracle(_synth.NAMED_DIMS[spec["dims"]], load_file(os.path.join(ckpt, "model.safetensors")))
                try:
                    cases = [L.run_case(ref_rankers, ref_listwise, ckpt, q, oracle) for q in queries]
                except AssertionError:                              # the oracle's greedy loop left the reference's generation: a coin-flip step
                    continue
            for case in cases:
                case["kind"], case["ckpt"] = "listwise-llama", "ckpt_llama_hd64_listwise"
                case["min_margin"] = min([m for c in case["compares"] for m in c["margin"]] or [0.0])
            ok = all(case["min_margin"] >= KEEP and case["compares"] for case in cases) and any(L.reorders(case) for case in cases)
            print(f"listwise seed {seed} boost {boost}/{boost_eos}: min margins {[round(c['min_margin'], 4) for c in cases]} -> {'kept' if ok else 'no'}", flush=True)
            if ok:
                return spec, cases, L.MODEL_EOS
    raise SystemExit("listwise: no recipe / seed fills every shape with margins of 4 x FLOOR")


def rankr1_cases(ref, seeds, first_seed):
    from safetensors.numpy import load_file
    from transformers import AutoTokenizer
    tok_dir = os.path.join(GOLD, "tok_qwen")
    prompt_path = os.path.join(GOLD, "rankr1_prompt.toml")
    vocab = AutoTokenizer.from_pretrained(tok_dir).get_vocab()
    ref_rankers, ref_setwise = R.import_reference_setwise(ref)
    queries = R.make_queries(np.random.RandomState(78))[:2]          # (3, 3, heapsort) and (5, 2, heapsort, 3 permutations)
    dims = _synth.NAMED_DIMS["toy-qwen2-hd64"]
    eos = vocab["<|im_end|>"]
    assert eos == dims.eos_token_id
    for seed in range(first_seed, first_seed + seeds):
        for boost, boost_eos in R.RECIPES:
            spec = {"dims": "toy-qwen2-hd64", "seed": seed, "gain": 2.0, "boost_ids": [vocab[f"[{i}]"] for i in range(1, 6)], "boost": boost,
                    "boost2_ids": [eos], "boost2": boost_eos, "tokenizer": "tok_qwen"}
            with tempfile.TemporaryDirectory() as tmp:
                ckpt, adir = os.path.join(tmp, "toy-qwen2-hd64"), os.path.join(tmp, "adapter")
                _synth.write_checkpoint(ckpt, spec, tok_dir)
                spec["sha256"] = _synth.checkpoint_sha256(ckpt)
                adapter = dict(R.ADAPTER)
                adapter["sha256"] = _synth.write_lora_adapter(adir, dims, adapter)
                base = load_file(os.path.join(ckpt, "model.safetensors"))
                merged = host_merge_lora(base, _synth.synth_lora_tensors(dims, adapter), adapter["lora_alpha"] / adapter["r"])
                R.StandInLLM.merged = merged
                cases = [R.run_case(ref_rankers, ref_setwise, ckpt, adir, prompt_path, q, tok_dir) for q in queries]
            moved = any(case["docids"] != [d for d, _ in case["docs"]] for case in cases)
            worst = R.add_margins(cases, dims, merged, eos) if moved else -1.0
            print(f"rank-r1 seed {seed} boost {boost}/{boost_eos}: re-orders {moved}, min margin {worst:.4f}", flush=True)
            if not worst >= KEEP:
                continue
            for case in cases:
                case["kind"], case["ckpt"], case["min_margin"] = "rankr1-qwen2", "ckpt_qwen2_hd64", worst
                for c in case["compares"]:
                    for r in c["rows"]:
                        r["prompt_len"], r["prompt_sha256"] = len(r["prompt_ids"]), R.ids_sha256(r["prompt_ids"])
                        del r["prompt_ids"]
            return spec, adapter, cases, eos
    raise SystemExit("rank-r1: no recipe / seed fills every shape with margins of 4 x FLOOR")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (ielab/llm-rankers), read-only")
    ap.add_argument("--seeds", type=int, default=12)
    ap.add_argument("--first-seed", type=int, default=641, help="of the setwise / pairwise checkpoint (645 is the first that qualifies; listwise starts at 701, Rank-R1 at 801)")
    args = ap.parse_args()
    import torch
    torch.set_num_threads(8)
    os.environ.setdefault("HF_HUB_OFFLINE", "1")
    ref = os.path.abspath(args.reference)
    tok_dir = os.path.join(GOLD, "tok_llama")
    with open(os.path.join(GOLD, "ckpts.json")) as f:
        label_ids = json.load(f)["ckpt_llama"]["boost_ids"]           # the 23 label rows, boosted as ckpt_llama's are
    from safetensors.numpy import load_file
    ref_rankers, ref_setwise, ref_pairwise = import_reference(ref)
    want = {("setwise-llama", i) for i in range(len(SETWISE_SHAPES))} | {("pairwise-llama", i) for i in range(len(PAIRWISE_SHAPES))}
    one_spec = one_cases = None
    for seed in range(args.first_seed, args.first_seed + args.seeds):
        spec = {"dims": "toy-llama-hd64", "seed": seed, "gain": 2.0, "boost_ids": label_ids, "boost": 6.0, "tokenizer": "tok_llama"}
        with tempfile.TemporaryDirectory() as tmp:
            ckpt = os.path.join(tmp, "toy-llama-hd64")
            _synth.write_checkpoint(ckpt, spec, tok_dir)
            spec["sha256"] = _synth.checkpoint_sha256(ckpt)
            oracle = LlamaOracle(_synth.NAMED_DIMS[spec["dims"]], load_file(os.path.join(ckpt, "model.safetensors")))
            kept, filled = one_token_cases(ref_rankers, ref_setwise, ref_pairwise, ckpt, oracle)
        print(f"setwise / pairwise seed {seed}: {len(kept)} cases kept, shapes filled {sorted(filled)}", flush=True)
        if filled == want:
            one_spec, one_cases = spec, kept
            break
    if one_spec is None:
        raise SystemExit("setwise / pairwise: no seed fills every shape with margins of 4 x FLOOR")
    lw_spec, lw_cases, lw_eos = listwise_cases(ref, args.seeds, 701, tok_dir)
    r1_spec, adapter, r1_cases, r1_eos = rankr1_cases(ref, args.seeds, 801)
    with open(os.path.join(GOLD, "llama_hd64_ckpts.json"), "w") as f:
        json.dump({"ckpt_llama_hd64": one_spec, "ckpt_llama_hd64_listwise": lw_spec, "ckpt_qwen2_hd64": r1_spec, "adapter_qwen2_hd64": adapter}, f, indent=1)
    out = {"about": "tools/make_llama_hd64_golden.py: the reference's Setwise / Pairwise / Listwise rankers (Llama branch) and its Rank-R1 ranker, CPU "
                    "fp32, on the 64-wide checkpoints of llama_hd64_ckpts.json; every case's every decision has an fp32-oracle margin >= keep",
           "floor": FLOOR, "keep": KEEP, "listwise_model_eos": lw_eos, "listwise_max_new": 20, "rankr1_model_eos": r1_eos,
           "cases": one_cases + lw_cases + r1_cases}
    with open(os.path.join(GOLD, "llama_hd64_cases.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    print("wrote llama_hd64_ckpts.json and llama_hd64_cases.json:", {k: sum(c["kind"] == k for c in out["cases"]) for k in sorted({c["kind"] for c in out["cases"]})})


if __name__ == "__main__":
    main()
