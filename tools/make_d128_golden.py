#!/usr/bin/env python
"""Fixtures for T5 checkpoints with 128-WIDE heads (t5-3b: monoT5-3B, duoT5-3B) from the REFERENCE's MonoT5LlmRanker (ref:
llmrankers/pointwise.py:136-186) and DuoT5LlmRanker (ref: llmrankers/pairwise.py:296-352) on CPU over the toy d128 checkpoint
(`toy-monot5-d128`: TOY_MONOT5 with d_kv = 128) - runs only where the reference (ielab/llm-rankers, imported from where
tools/make_goldens.py finds it: read-only, never copied) and transformers are installed.

-> tests/golden/d128_ckpts.json   the `_synth.write_checkpoint` recipes with their sha256 (weights are not committed):
                                  ckpt_monot5_d128 at gain 1.0 (as ckpt_monot5), ckpt_duot5_d128 at gain 2.0 (as ckpt_duot5)
-> tests/golden/d128_cases.json   "monot5": queries of 2 to 12 passages - input, query, batch_size, result (docid, score), counters;
                                  "duot5": the shapes of tools/make_duot5_golden.py, its records per case and per compare (pair,
                                  verdict, margin, the reference's fp32 logits), the truncating case included;
                                  "provenance": generator, reference, library versions.

Margin rules, so that ORDER is asserted for every committed case with none left out: a monoT5 query is kept only when every adjacent
pair of the reference's sorted scores differs by at least MONO_MIN_GAP = 4e-3, four times the project's SCORE_TOL = 1e-3; a duoT5
query only when EVERY compare has a margin |(t0 - f0) - (t1 - f1)| >= MIN_MARGIN (tools/make_duot5_golden.py's rule;
tests/test_gpu_t5_d128.py measures the engine's logit error and asserts the recorded margins against four times it).  Candidates
are drawn from a fixed seed sequence until a shape is filled, the first that qualifies is kept; a shape that cannot be filled ends
the tool with an error.

usage: python tools/make_d128_golden.py
"""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_goldens as mg                              # noqa: E402  (the stub modules / import path of the reference, WORDS)
from llmrankers import _synth                          # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
SPECS = {"ckpt_monot5_d128": {"dims": "toy-monot5-d128", "seed": 24, "gain": 1.0},
         "ckpt_duot5_d128": {"dims": "toy-monot5-d128", "seed": 25, "gain": 2.0}}
MONO_MIN_GAP = 4e-3        # four times SCORE_TOL
MIN_MARGIN = 4e-2          # tools/make_duot5_golden.py's rule (tests/test_gpu_t5_d128.py: FLOOR)
FALSE_ID, TRUE_ID = 6136, 1176
MONO_SHAPES = [(2, 1), (3, 4), (4, 32), (5, 2), (7, 4), (9, 32), (12, 5), (12, 32)]          # (passages, batch_size)
# (candidates, k, tokenizer.model_max_length or None): make_duot5_golden.py's
DUO_SHAPES = [(2, 1, None), (3, 5, None), (3, 1, None), (7, 1, None), (7, 10, None), (12, 5, None), (12, 10, None), (20, 5, None),
              (20, 10, None), (12, 5, 48)]
MAX_TRIES = 400


def distinct_texts(rs, n):
    texts = []
    while len(texts) < n:
        t = mg.rand_text(rs, 8, 40)
        if t not in texts:
            texts.append(t)
    return texts


def monot5_cases(ref_rankers, ref_pointwise, ckpt):
    sink = io.StringIO()
    rs = np.random.RandomState(178)
    cases, tried = [], 0
    for n, bs in MONO_SHAPES:
        for _ in range(MAX_TRIES):
            tried += 1
            query, texts = mg.rand_text(rs, 3, 8), distinct_texts(rs, n)
            with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
                rk = ref_pointwise.MonoT5LlmRanker(ckpt, ckpt, device="cpu", method="yes_no", batch_size=bs)
                ranking = [ref_rankers.SearchResult(docid=f"M{len(cases)}_{i}", score=float(50 - i), text=t) for i, t in enumerate(texts)]
                inp = [[r.docid, r.score, r.text] for r in ranking]
                res = rk.rerank(query, ranking)
            scores = [float(r.score) for r in res]
            gap = min(a - b for a, b in zip(scores, scores[1:]))
            if gap < MONO_MIN_GAP:
                continue
            cases.append({"kind": "monot5", "ckpt": "ckpt_monot5_d128", "batch_size": bs, "query": query, "input": inp,
                          "result": [[r.docid, float(r.score)] for r in res], "min_gap": gap,
                          "counters": [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens]})
            print(f"[d128 monot5] n={n} batch_size={bs}: min adjacent gap {gap:.4f}, counters {cases[-1]['counters']}", flush=True)
            break
        else:
            raise SystemExit(f"no monoT5 query of {n} passages met the gap rule in {MAX_TRIES} tries")
    return cases, tried


def duot5_cases(ref_rankers, ref_pairwise, ckpt, tok_dir):
    sink = io.StringIO()
    rs = np.random.RandomState(277)
    cases, tried = [], 0
    for n, k, max_len in DUO_SHAPES:
        for _ in range(MAX_TRIES):
            tried += 1
            query, texts = mg.rand_text(rs, 3, 8), distinct_texts(rs, n)
            with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
                rk = ref_pairwise.DuoT5LlmRanker(ckpt, ckpt, device="cpu", method="heapsort", batch_size=2, k=k)
            if max_len is not None:
                rk.tokenizer.model_max_length = max_len
            last = []
            hook = rk.llm.register_forward_hook(lambda mod, args, out: last.append(out.logits[:, 0, [FALSE_ID, TRUE_ID]].detach().numpy().astype(np.float32)))
            ranking = [ref_rankers.SearchResult(docid=f"D{len(cases)}_{i}", score=float(50 - i), text=t) for i, t in enumerate(texts)]
            docid_of = {r.text: r.docid for r in ranking}
            inp = [[r.docid, r.score, r.text] for r in ranking]
            log = []
            orig = rk.compare

            def logged(q, docs, _o=orig):
                del last[:]
                verdict = bool(_o(q, docs))
                (lg,) = last
                margin = abs(float((lg[0, 1] - lg[0, 0]) - (lg[1, 1] - lg[1, 0])))
                log.append({"pair": [docid_of[docs[0]], docid_of[docs[1]]], "first_wins": verdict, "margin": margin,
                            "logits": [[float(x) for x in row] for row in lg]})
                return verdict

            rk.compare = logged
            with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
                res = rk.rerank(query, ranking)
            hook.remove()
            if log and min(c["margin"] for c in log) < MIN_MARGIN:
                continue
            cut = 0
            if max_len is not None:                    # the case must really truncate: count prompts longer than the limit
                from transformers import T5Tokenizer
                plain = T5Tokenizer.from_pretrained(tok_dir)
                for c in log:
                    a, b = (next(t for d, _, t in inp if d == x) for x in c["pair"])
                    for d1, d2 in ((a, b), (b, a)):
                        cut += len(plain(f"Query: {query} Document0: {d1} Document1: {d2} Relevant:")["input_ids"]) > max_len
                if cut == 0:
                    continue
            cases.append({"kind": "duot5", "ckpt": "ckpt_duot5_d128", "method": "heapsort", "k": k, "model_max_length": max_len,
                          "query": query, "input": inp, "result": [[r.docid, r.score] for r in res], "compares": log,
                          "caller_list_after": [r.docid for r in ranking], "prompts_cut": cut,
                          "min_margin": min((c["margin"] for c in log), default=None),
                          "counters": [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens]})
            print(f"[d128 duot5] n={n} k={k} max_len={max_len}: {len(log)} compares, min margin {cases[-1]['min_margin']}, cut {cut}, "
                  f"counters {cases[-1]['counters']}", flush=True)
            break
        else:
            raise SystemExit(f"no duoT5 query of shape n={n} k={k} max_len={max_len} met the margin rule in {MAX_TRIES} tries")
    return cases, tried


def main():
    tok_dir = os.path.join(GOLD, "tok")
    tmp = tempfile.mkdtemp(prefix="rk_d128_")
    specs, ckpts = {}, {}
    for name, spec in SPECS.items():
        ckpts[name] = os.path.join(tmp, name)
        specs[name] = dict(spec)
        specs[name]["sha256"] = mg.write_ckpt(ckpts[name], spec, tok_dir)
    with open(os.path.join(GOLD, "d128_ckpts.json"), "w") as f:
        json.dump(specs, f, indent=1)

    ref_rankers, ref_pointwise, _ = mg.import_reference()
    import llmrankers.pairwise as ref_pairwise
    assert ref_pairwise.__file__.startswith(mg.REF), ref_pairwise.__file__
    mono, mono_tried = monot5_cases(ref_rankers, ref_pointwise, ckpts["ckpt_monot5_d128"])
    duo, duo_tried = duot5_cases(ref_rankers, ref_pairwise, ckpts["ckpt_duot5_d128"], tok_dir)
    import torch
    import transformers
    with open(os.path.join(GOLD, "d128_cases.json"), "w") as f:
        json.dump({"mono_min_gap_rule": MONO_MIN_GAP, "min_margin_rule": MIN_MARGIN, "queries_tried": [mono_tried, duo_tried], "monot5": mono,
                   "duot5": duo, "provenance": {"generator": "tools/make_d128_golden.py", "reference": "ielab/llm-rankers (2025-07-18)",
                                                "transformers": transformers.__version__, "torch": torch.__version__, "numpy": np.__version__}}, f)
    margins = sorted(c["margin"] for case in duo for c in case["compares"])
    print(f"[d128_cases] monoT5 {len(mono)} cases of {mono_tried} tried, smallest gap {min(c['min_gap'] for c in mono):.4f}; duoT5 {len(duo)} cases of "
          f"{duo_tried} tried, {len(margins)} compares, margin min {margins[0]:.4f} median {margins[len(margins) // 2]:.3f}")
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
