"""Shared by the host and the GPU test of the recorded R1 listwise cases (tests/golden/r1_listwise_cases.json,
tools/make_r1_listwise_golden.py): run one case through a ranker with every compare logged, and hold the log to the record."""
import contextlib
import io

import numpy as np


def ids_sha256(ids):
    import hashlib
    return hashlib.sha256(np.asarray(ids, dtype=np.int32).tobytes()).hexdigest()


def run_r1_case(rk, rt, case, guard=lambda fn, *a, **kw: fn(*a, **kw)):
    """rerank with every compare's prompt and new tokens logged -> (result, [{output, prompt_len, prompt_sha256, new_ids, completion}])"""
    from llmrankers.rankers import SearchResult
    log, real_generate, real_compare = [], rt.generate, rk.compare
    eos = list(rt.generation["eos_token_ids"])

    def generate(seqs, max_new, eos_ids, pad_id, max_total=0):
        out = guard(real_generate, seqs, max_new, eos_ids, pad_id, max_total)
        for s, row in zip(seqs, np.asarray(out)):
            new = [int(t) for t in row if t >= 0]
            stop = next((i for i, t in enumerate(new) if t in eos), None)
            new = new if stop is None else new[:stop + 1]
            log.append({"prompt_len": len(s), "prompt_sha256": ids_sha256(s), "new_ids": new, "completion": rk.tokenizer.decode(new, skip_special_tokens=True)})
        return out

    def compare(query, docs):
        out = real_compare(query, docs)
        log[-1]["output"] = out
        return out

    rt.generate, rk.compare = generate, compare
    try:
        ranking = [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]]
        with contextlib.redirect_stdout(io.StringIO()):
            res = rk.rerank(case["query"], ranking)
        assert [d.docid for d in ranking] == [d for d, _ in case["docs"]]
    finally:
        rt.generate = real_generate
        del rk.compare
    return res, log


def check_r1_case(rk, res, log, case):
    tag = case["qid"]
    want = [{k: c[k] for k in ("prompt_len", "prompt_sha256", "new_ids", "completion", "output")} for c in case["compares"]]
    assert log == want, tag
    assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
    assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
