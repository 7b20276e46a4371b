#!/usr/bin/env python
"""Grouped qlm (PointwiseLlmRanker.rerank_many -> rk_t5_qlm_many) against the one-by-one loop (rerank per query, the
single-label rk_t5_qlm path) IN THE SAME PROCESS, on one MI355X: flan-t5-xl dimensions, timing-only pool weights, fixture
tokenizer, 128-token passages, queries of 15..33 label tokens drawn with a fixed seed (they land on both sides of the
16 / 17 position line, so a grouped call usually runs two ragged decoder passes).
  leg "full":  100 passages per query, 1 / 2 / 4 queries per rerank_many;
  leg "share": one of eight ranks' share of hits=100 (13 passages per query) through a one-rank communicator
               (shard_candidates=True: append + ONE gather per call), 1 / 4 / 8 / 16 queries per rerank_many.
Per leg and group size: ms per query grouped and one by one (median of five after two warm-ups, and the spread of the
five), and the engine's per-kernel-class event times of one grouped call.  Lines are appended to
profiles/qlm_many_bench.jsonl.  Without --leg every leg runs in a child process of its own under a time limit, and the
first failure ends the run."""
import argparse, json, os, random, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
LEGS = {"full": (100, (1, 2, 4), False), "share": (13, (1, 4, 8, 16), True)}
OUT = os.path.join(REPO, "profiles", "qlm_many_bench.jsonl")


def run_leg(leg, model="flan-t5-xl", batch_size=32):
    import numpy as np
    import torch  # noqa  (its HIP runtime first)
    from transformers import T5Tokenizer
    from llmrankers import _synth
    from llmrankers._engine import RkEngine
    from llmrankers._runtime import T5Runtime
    from llmrankers.pointwise import PointwiseLlmRanker
    from llmrankers.rankers import SearchResult
    n_docs, group_sizes, shard = LEGS[leg]
    dims = _synth.NAMED_DIMS[model]
    eng = RkEngine(dims, 0, max_tokens=49152, max_seqs=256, max_dec_len=48).load_state(_synth.synth_tensors_pool(dims, seed=929))
    try:
        rt = T5Runtime.from_engine(eng, dims)
        if shard:
            eng.comm_init(eng.comm_unique_id(), 0, 1, 8192)
        tok = T5Tokenizer.from_pretrained(os.path.join(REPO, "tests", "golden", "tok"))
        ranker = PointwiseLlmRanker.from_runtime(rt, tok, method="qlm", batch_size=batch_size, shard_candidates=shard)
        rs = random.Random(3)
        vocab = [tok.convert_ids_to_tokens(i).replace("▁", "") for i in range(10, 200)]
        vocab = [w for w in vocab if w.isalpha()] or ["a", "b", "c"]
        docs = [ranker.truncate(" ".join(rs.choice(vocab) for _ in range(140)), 128) for _ in range(n_docs)]

        def n_labels(q):
            return len(tok.encode(f"<pad> {q}", add_special_tokens=False))

        queries = []
        for _ in range(max(group_sizes)):
            target, words = rs.randint(15, 33), [rs.choice(vocab)]
            while n_labels(" ".join(words)) < target:
                words.append(rs.choice(vocab))
            while n_labels(" ".join(words)) > 33:
                words.pop()
            queries.append(" ".join(words))

        def items(g):
            return [(q, [SearchResult(docid=str(i), score=float(n_docs - i), text=d) for i, d in enumerate(docs)]) for q in queries[:g]]

        def timed(fn, g):
            ts = []
            for _ in range(7):
                its = items(g)
                t = time.perf_counter()
                fn(its)
                ts.append((time.perf_counter() - t) * 1e3 / g)
            five = ts[2:]
            return round(float(np.median(five)), 3), round(float(max(five) - min(five)), 3)

        def one_by_one(its):
            for q, ranking in its:
                ranker.rerank(q, ranking)

        lines = []
        for g in group_sizes:
            labels = [n_labels(q) for q in queries[:g]]
            loop_ms, loop_spread = timed(one_by_one, g)
            many_ms, many_spread = timed(ranker.rerank_many, g)
            eng.profile(True); eng.profile_reset()
            got, _ = ranker.rerank_many(items(g))
            eng.sync()
            rep = eng.profile_report(); eng.profile(False)
            assert all(np.isfinite(d.score) for res in got for d in res)
            lines.append({"tool": "bench_qlm_many", "leg": leg, "model": model + " dims, pool weights", "passages_per_query": n_docs,
                          "queries_per_call": g, "label_counts": labels, "sharded_one_rank_comm": shard,
                          "ms_per_query_grouped": many_ms, "grouped_spread_ms": many_spread,
                          "ms_per_query_one_by_one": loop_ms, "one_by_one_spread_ms": loop_spread,
                          "speedup": round(loop_ms / many_ms, 3),
                          "classes_ms_one_grouped_call": {k: [round(v["ms"], 3), int(v["launches"])] for k, v in rep.items() if v["launches"]}})
        return lines
    finally:
        if shard and getattr(eng, "comm_capacity", 0):
            eng.comm_destroy()
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per leg (child process)")
    args = ap.parse_args()
    if args.leg:
        lines = run_leg(args.leg)
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)
        return 0
    for leg in ("full", "share"):                     # each GPU step in a fresh process under its own limit; stop at the first failure
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"leg {leg}: time limit of {args.timeout} s", file=sys.stderr)
            return 124
        if rc:
            print(f"leg {leg}: exit status {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
