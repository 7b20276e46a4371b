#!/usr/bin/env python
"""One duoT5 heapsort query end to end: 100 passages of ~100 tokens, k = 10, synthetic weights at duot5-base dimensions (T5
v1.0 base: d_model 768, 12 heads, d_kv 64, d_ff 3072, relu, tied head) and the test tokenizer.  ms per query for
  (a) one compare per `score` call plus the softmax on the host - the most the engine offered before rk_t5_compare,
  (b) DuoT5LlmRanker.rerank: device verdict, level-batched build phase,
  (c) DuoT5LlmRanker.rerank_many at 4 / 8 / 16 / 32 queries: the heapsorts in lock step, two groups alternating over the slots,
and the rk_profile_* time of the head class (pair_verdict_kernel's bracket) within one query of (b).
-> profiles/duot5_bench.txt (or --out PATH); llmrankers._batching.default_queries_per_call("duot5") quotes the sweep.

usage: python tools/bench_duot5.py [--out PATH] [--reps N] [--many 4,8,16,32]"""
import argparse
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
from llmrankers import _synth                      # noqa: E402
from llmrankers._engine import RkEngine            # noqa: E402
from llmrankers._runtime import T5Runtime          # noqa: E402
from llmrankers.pairwise import DuoT5LlmRanker     # noqa: E402
from llmrankers.rankers import SearchResult        # noqa: E402


class ScoreOnly:
    """The runtime as it was before rk_t5_compare: `score` alone, so the ranker takes the softmax and the verdict on the host."""
    model_type, decoder_start_token_id = "t5", 0

    def __init__(self, rt):
        self.config, self.score = rt.config, rt.score


def run(reps=3, many=(4, 8, 16, 32), passages=100, words=100, k=10):
    from transformers import T5Tokenizer
    tok = T5Tokenizer.from_pretrained(os.path.join(REPO, "tests", "golden", "tok"))
    dims = _synth.NAMED_DIMS["duot5-base"]
    eng = RkEngine(dims, 0, max_tokens=49152, max_seqs=256, max_dec_len=8)                 # T5Runtime's default capacities
    eng.load_state(_synth.synth_tensors(dims, seed=929, gain=2.0, threads=min(16, os.cpu_count() or 8)))
    rt = T5Runtime.from_engine(eng, dims)
    rs = random.Random(5)
    vocab = [tok.convert_ids_to_tokens(i).replace("▁", "") for i in range(10, 200)]
    vocab = [w for w in vocab if w.isalpha()] or ["a", "b", "c"]
    docs = [(f"d{i}", float(passages - i), " ".join(rs.choice(vocab) for _ in range(words))) for i in range(passages)]
    queries = [" ".join(rs.choice(vocab) for _ in range(8)) for _ in range(max(many))]

    def ranking():
        return [SearchResult(docid=d, score=s, text=t) for d, s, t in docs]

    def timed(fn):
        best, res = None, None
        for _ in range(reps):
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, res

    out = {"dims": "duot5-base", "passages": passages, "k": k, "reps": reps}
    a = DuoT5LlmRanker.from_runtime(ScoreOnly(rt), tok, method="heapsort", k=k)
    a.batch_independent_compares = False
    t, res_a = timed(lambda: a.rerank(queries[0], ranking()))
    out["a_score_call_per_compare"] = {"ms_per_query": round(t * 1e3, 1), "compares": a.total_compare,
                                       "avg_prompt_tokens": round(a.total_prompt_tokens / (2 * a.total_compare), 1)}
    b = DuoT5LlmRanker.from_runtime(rt, tok, method="heapsort", k=k)
    t, res_b = timed(lambda: b.rerank(queries[0], ranking()))
    out["b_rerank_level_batched"] = {"ms_per_query": round(t * 1e3, 1), "compares": b.total_compare}
    out["b_same_ranking_as_a"] = [r.docid for r in res_a] == [r.docid for r in res_b]
    singles = {}
    for nq in many:
        c = DuoT5LlmRanker.from_runtime(rt, tok, method="heapsort", k=k)
        t, (res, counters) = timed(lambda: c.rerank_many([(q, ranking()) for q in queries[:nq]]))
        out[f"c_rerank_many_{nq}"] = {"ms_per_query": round(t * 1e3 / nq, 2), "queries_per_call": nq, "compares": sum(x[0] for x in counters)}
        singles[nq] = [r.docid for r in res[0]][:k]
    out["c_first_query_same_as_b"] = all(top == [r.docid for r in res_b][:k] for top in singles.values())
    # the head class inside one query of (b): per-kernel events, eager launches
    eng.profile(True)
    eng.profile_reset()
    b.rerank(queries[0], ranking())
    rep = eng.profile_report()
    eng.profile(False)
    total = sum(v["ms"] for v in rep.values())
    out["profile_one_query"] = {"total_kernel_ms": round(total, 3),
                                "classes": {name: {"ms": round(v["ms"], 4), "launches": v["launches"]} for name, v in rep.items() if v["launches"]}}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "duot5_bench.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--many", default="4,8,16,32")
    args = ap.parse_args()
    out = run(reps=args.reps, many=tuple(int(x) for x in args.many.split(",")))
    lines = ["duoT5 heapsort, %d passages of ~100 tokens, k = %d, duot5-base dims, synthetic weights (tools/bench_duot5.py), best of %d"
             % (out["passages"], out["k"], out["reps"]),
             "(a) one compare per score call + host softmax : %8.1f ms / query  (%d compares, ~%s tokens per prompt)"
             % (out["a_score_call_per_compare"]["ms_per_query"], out["a_score_call_per_compare"]["compares"],
                out["a_score_call_per_compare"]["avg_prompt_tokens"]),
             "(b) rerank, device verdict, level-batched build: %8.1f ms / query  (%d compares, same ranking as (a): %s)"
             % (out["b_rerank_level_batched"]["ms_per_query"], out["b_rerank_level_batched"]["compares"], out["b_same_ranking_as_a"])]
    for key, v in out.items():
        if key.startswith("c_rerank_many_"):
            lines.append("(c) rerank_many, %2d queries in lock step        : %8.2f ms / query  (%d compares)"
                         % (v["queries_per_call"], v["ms_per_query"], v["compares"]))
    lines.append("    first query of every (c) ranks as in (b): %s" % out["c_first_query_same_as_b"])
    prof = out["profile_one_query"]
    lines.append("rk_profile_* over one query of (b), %.3f ms of kernels in all:" % prof["total_kernel_ms"])
    for name, v in sorted(prof["classes"].items(), key=lambda kv: -kv[1]["ms"]):
        lines.append("    %-10s %9.4f ms  %6d launches" % (name, v["ms"], v["launches"]))
    lines.append(json.dumps(out))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
