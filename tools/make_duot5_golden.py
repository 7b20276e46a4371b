#!/usr/bin/env python
"""duoT5 fixtures from the REFERENCE's DuoT5LlmRanker (ref: llmrankers/pairwise.py:296-352) - runs only where the reference
(ielab/llm-rankers, imported from where tools/make_goldens.py finds it: read-only, never copied) and transformers are installed.

-> tests/golden/duot5_ckpt.json   the `_synth.write_checkpoint` recipe of the fixture checkpoint with its sha256 (a monoT5-like
                                  toy whose vocabulary covers the ids 6136 / 1176 of `false` / `true`; weights are not committed)
-> tests/golden/duot5_cases.json  heapsort queries: input, query, k, result, counters, the caller's list afterwards and, per
                                  compare IN REFERENCE ORDER, the pair (docids), the verdict and the margin
                                  |(t0 - f0) - (t1 - f1)| of the reference's fp32 logits: the distance of the compare from a
                                  tie, in logit units (P(true) = sigmoid(t - f)).

Margin rule: a query is kept only when EVERY one of its compares has a margin >= MIN_MARGIN, so that the fp16 engine takes
every decision of every committed case as the fp32 reference did; candidates are drawn from a fixed seed sequence until a
case's shape is filled, the first that qualifies is kept.  tests/test_gpu_duot5.py measures the engine's logit error and
asserts the recorded margins against four times it.

One case sets tokenizer.model_max_length = 48, so `truncation=True` cuts its prompts.

usage: python tools/make_duot5_golden.py
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
MIN_MARGIN = 4e-2          # above four times the engine's measured per-logit error (tests/test_gpu_duot5.py: FLOOR); 2e-2 at first, raised once that was measured
SPEC = {"dims": "toy-monot5", "seed": 15, "gain": 2.0}
FALSE_ID, TRUE_ID = 6136, 1176
# (candidates, k, tokenizer.model_max_length or None); k exceeds the candidate count in three of them
SHAPES = [(2, 1, None), (3, 5, None), (3, 1, None), (7, 1, None), (7, 10, None), (12, 5, None), (12, 10, None), (20, 5, None),
          (20, 10, None), (12, 5, 48)]
MAX_TRIES = 400


def main():
    tok_dir = os.path.join(GOLD, "tok")
    tmp = tempfile.mkdtemp(prefix="rk_duot5_")
    ckpt = os.path.join(tmp, "ckpt_duot5")
    spec = dict(SPEC)
    spec["sha256"] = mg.write_ckpt(ckpt, spec, tok_dir)
    with open(os.path.join(GOLD, "duot5_ckpt.json"), "w") as f:
        json.dump({"ckpt_duot5": spec}, f, indent=1)

    ref_rankers, _, _ = mg.import_reference()
    import llmrankers.pairwise as ref_pairwise
    assert ref_pairwise.__file__.startswith(mg.REF), ref_pairwise.__file__

    sink = io.StringIO()
    rs = np.random.RandomState(77)
    cases, tried = [], 0
    for n, k, max_len in SHAPES:
        for _ in range(MAX_TRIES):
            tried += 1
            query = mg.rand_text(rs, 3, 8)
            texts = []
            while len(texts) < n:                      # distinct texts: a text names its docid in the compare log
                t = mg.rand_text(rs, 8, 40)
                if t not in texts:
                    texts.append(t)
            with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
                rk = ref_pairwise.DuoT5LlmRanker(ckpt, ckpt, device="cpu", method="heapsort", batch_size=2, k=k)
            no_limit = int(rk.tokenizer.model_max_length)
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
            cases.append({"kind": "duot5", "ckpt": "ckpt_duot5", "method": "heapsort", "k": k, "model_max_length": max_len,
                          "query": query, "input": inp, "result": [[r.docid, r.score] for r in res], "compares": log,
                          "caller_list_after": [r.docid for r in ranking], "prompts_cut": cut,
                          "min_margin": min((c["margin"] for c in log), default=None),
                          "counters": [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens]})
            print(f"[duot5] n={n} k={k} max_len={max_len}: {len(log)} compares, min margin {cases[-1]['min_margin']}, "
                  f"cut {cut}, counters {cases[-1]['counters']} (tokenizer limit {no_limit if max_len is None else max_len})", flush=True)
            break
        else:
            raise SystemExit(f"no query of shape n={n} k={k} max_len={max_len} met the margin rule in {MAX_TRIES} tries")
    with open(os.path.join(GOLD, "duot5_cases.json"), "w") as f:
        json.dump({"min_margin_rule": MIN_MARGIN, "queries_tried": tried, "cases": cases}, f)
    margins = sorted(c["margin"] for case in cases for c in case["compares"])
    print(f"[duot5_cases] {len(cases)} cases of {tried} tried, {len(margins)} compares, margin min {margins[0]:.4f} "
          f"median {margins[len(margins) // 2]:.3f}")
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
