#!/usr/bin/env python
"""monoT5-3B and duoT5-3B on the engine: t5-3b dimensions (d_model 1024, 32 heads of 128, d_ff 16384, relu, tied head, 24 + 24
layers), synthetic timing-only weights (llmrankers._synth.synth_tensors_pool) and the test tokenizer.
  (a) monoT5: 320 prompts of L_e = 184 tokens in calls of batch_size 32 (one staged call per batch, the slots pipelined):
      passages / s, HIP events on the engine's streams, median of three regions;
  (b) duoT5: one heapsort query of 100 candidates of ~100 words, k = 10 (DuoT5LlmRanker.rerank): ms per query, median of three;
  (c) the encoder attention alone at equal I = 4096 on the same 32 x 184 tokens, through rk_debug_attn with per-kernel events:
      the 128-wide kernel (H = 32, attn_enc128_kernel) against the 64-wide default plan (H = 64 at width 64, on a 64-wide toy
      engine): us per launch, median of three, and the 128 / 64 ratio (equal FLOPs: 4 L T I either way).
Appends the results to profiles/t5_3b_bench.txt (or --out PATH).

usage: python tools/bench_t5_3b.py [--out PATH] [--skip-model]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
from llmrankers import _synth                      # noqa: E402
from llmrankers._engine import RkEngine            # noqa: E402
from llmrankers._runtime import T5Runtime          # noqa: E402
from llmrankers.pairwise import DuoT5LlmRanker     # noqa: E402
from llmrankers.rankers import SearchResult        # noqa: E402

FALSE_ID, TRUE_ID = 6136, 1176


def attention_ratio(n_seq=32, L=184, I=4096, band=8):
    """(c): us per launch of the encoder attention on the same tokens, 128-wide against 64-wide"""
    rs = np.random.RandomState(3)
    T = n_seq * L
    q = rs.standard_normal((T + 2 * band, 3 * I)).astype(np.float16)
    off = np.arange(n_seq + 1, dtype=np.int32) * L
    out = np.zeros((T, I), dtype=np.float16)
    res = {}
    for name, dims, H in (("d128", _synth.TOY_MONOT5_D128, I // 128), ("d64", _synth.TOY_MONOT5, I // 64)):
        eng = RkEngine(dims, 0, max_tokens=2048, max_seqs=16, max_dec_len=8).load_state(_synth.synth_state_dict(dims, seed=7, gain=1.0).items())
        lut = (2.0 * rs.standard_normal((H, 257))).astype(np.float32)
        kw = dict(n_seq=n_seq, H=H, q=q, out=out, band_rows=band, ldq=3 * I, ldctx=I, seq_off=off, bias_lut=lut)
        plan = eng.debug_attn(1, plan_only=True, **kw)
        eng.debug_attn(1, **kw)                                      # warm-up (the kernel's one-off attribute call)
        eng.profile(True)
        us = []
        for _ in range(3):
            eng.profile_reset()
            eng.debug_attn(1, **kw)
            rep = eng.profile_report()["enc_attn"]
            us.append(rep["ms"] * 1e3 / max(rep["launches"], 1))
        eng.profile(False)
        eng.close()
        res[name] = {"H": H, "plan_kind": plan["kind"], "grid": plan["grid"], "lds": plan["lds"], "us_per_launch": round(statistics.median(us), 1), "runs": [round(u, 1) for u in us]}
    res["ratio_128_over_64"] = round(res["d128"]["us_per_launch"] / res["d64"]["us_per_launch"], 2)
    return res


def model_legs(batch=32, n_batches=10, L=184, passages=100, words=100, k=10):
    from transformers import T5Tokenizer
    tok = T5Tokenizer.from_pretrained(os.path.join(REPO, "tests", "golden", "tok"))
    dims = _synth.NAMED_DIMS["t5-3b"]
    t0 = time.perf_counter()
    eng = RkEngine(dims, 0, max_tokens=16384, max_seqs=64, max_dec_len=4)
    eng.load_state(_synth.synth_tensors_pool(dims, seed=929))
    load_s = time.perf_counter() - t0
    rt = T5Runtime.from_engine(eng, dims)
    out = {"dims": "t5-3b", "load_s": round(load_s, 1)}
    # (a) monoT5: batches of 32 prompts of 184 tokens, the two slots pipelined
    batches = [_synth.synth_token_batch(batch, L, L, dims.vocab, seed=100 + i) for i in range(n_batches)]
    rt.score_batches(batches[:2], [0], [FALSE_ID, TRUE_ID])          # warm-up: graphs captured, attributes set
    n_slots, regions = eng.num_slots, []
    for _ in range(3):
        eng.sync()
        eng.timer_begin()
        pending = []
        for i, b in enumerate(batches):
            slot = i % n_slots
            if len(pending) == n_slots:
                eng.read_scores(pending.pop(0))
            eng.stage(b, slot=slot)
            eng.score_staged([0], [FALSE_ID, TRUE_ID], slot=slot)
            pending.append(slot)
        for s in pending:
            eng.read_scores(s)
        regions.append(eng.timer_end())
    ms = statistics.median(regions)
    out["monot5"] = {"batch_size": batch, "L_e": L, "passages": batch * n_batches, "ms_regions": [round(x, 2) for x in regions],
                     "passages_per_s": round(batch * n_batches / (ms * 1e-3), 1)}
    # (b) duoT5: one heapsort query of 100 candidates
    rs = random.Random(5)
    vocab = [tok.convert_ids_to_tokens(i).replace("▁", "") for i in range(10, 200)]
    vocab = [w for w in vocab if w.isalpha()] or ["a", "b", "c"]
    docs = [(f"d{i}", float(passages - i), " ".join(rs.choice(vocab) for _ in range(words))) for i in range(passages)]
    query = " ".join(rs.choice(vocab) for _ in range(8))
    rk = DuoT5LlmRanker.from_runtime(rt, tok, method="heapsort", k=k)
    times = []
    for rep in range(4):                                               # the first is the warm-up
        eng.sync()
        eng.timer_begin()
        t0 = time.perf_counter()
        rk.rerank(query, [SearchResult(docid=d, score=s, text=t) for d, s, t in docs])
        wall = (time.perf_counter() - t0) * 1e3
        ev = eng.timer_end()
        if rep:
            times.append((ev, wall))
    out["duot5"] = {"candidates": passages, "k": k, "compares": rk.total_compare, "ms_per_query_events": round(statistics.median(t[0] for t in times), 1),
                    "ms_per_query_wall": round(statistics.median(t[1] for t in times), 1),
                    "avg_prompt_tokens": round(rk.total_prompt_tokens / (2 * rk.total_compare), 1)}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "t5_3b_bench.txt"))
    ap.add_argument("--skip-model", action="store_true", help="the attention comparison (c) only")
    args = ap.parse_args()
    out = {"attention": attention_ratio()}
    a = out["attention"]
    lines = ["t5-3b on the engine (tools/bench_t5_3b.py), synthetic weights, one MI355X, median of three",
             "(c) encoder attention, 32 x 184 tokens, I = 4096: 128-wide (H = 32) %8.1f us / launch, 64-wide default plan (H = 64) %8.1f us / launch, 128 / 64 = %.2f"
             % (a["d128"]["us_per_launch"], a["d64"]["us_per_launch"], a["ratio_128_over_64"])]
    if not args.skip_model:
        out.update(model_legs())
        m, d = out["monot5"], out["duot5"]
        lines.append("(a) monoT5-3B, batch_size %d, L_e = %d: %8.1f passages / s  (%d passages, regions %s ms)"
                     % (m["batch_size"], m["L_e"], m["passages_per_s"], m["passages"], m["ms_regions"]))
        lines.append("(b) duoT5-3B heapsort, %d candidates, k = %d: %8.1f ms / query by HIP events, %.1f wall  (%d compares, ~%s tokens per prompt)"
                     % (d["candidates"], d["k"], d["ms_per_query_events"], d["ms_per_query_wall"], d["compares"], d["avg_prompt_tokens"]))
    lines.append(json.dumps(out))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
