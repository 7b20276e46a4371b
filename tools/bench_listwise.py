#!/usr/bin/env python
"""Listwise ranking on the engine (flan-t5-large dims, seeded synthetic weights, the test tokenizer): one query of 100 passages
of ~100 tokens (varied lengths), window 4, step 2, num_repeat 1 - ListwiseLlmRanker.rerank() wall time per query for
`generation` and `likelihood`; for `generation` the same ranker on rk_t5_generate (KV-cached incremental decoder) against
rk_t5_greedy (whole-prefix recompute), alternated in one process; lockstep (rerank_many) at 1 / 8 / 32 queries per call; and
microseconds per decoder step of rk_t5_generate at 1 and 32 sequences ((t(20 new tokens) - t(1)) / 19 over the same prompts).
One JSON object per line on stdout, and into the file --out names.

--llama: the Llama leg instead (Llama-3-8B dims, _synth's timing-only weights, window-4-sized prompts of 1 536 tokens, 20 new
tokens, no EOS).  Per row count 1 / 8 / 32, median of three: rk_llama_generate's prefill (max_new = 1), ms per KV-cached step
((t(20) - t(1)) / 19), and the same 20 tokens by a loop of rk_llama_greedy1 over the growing prompt (a full prefill per token) in
the same process; plus the per-class split of one 20-token call (event-bracketed pass).  --llama --profile-call: ONE call of 8
rows (for `rocprofv3 --kernel-trace --stats -- python tools/bench_listwise.py --llama --profile-call`).

--profile-call: only ONE lockstep call of 8 windows (for `rocprofv3 --kernel-trace --hip-runtime-trace --stats -- python
tools/bench_listwise.py --profile-call`): every decoder step of it should be one hipGraphLaunch."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
from llmrankers import _synth                      # noqa: E402
from llmrankers._engine import RkEngine            # noqa: E402
from llmrankers._runtime import T5Runtime          # noqa: E402
from llmrankers.listwise import ListwiseLlmRanker  # noqa: E402
from llmrankers.rankers import SearchResult        # noqa: E402


class BenchRuntime(T5Runtime):
    """T5Runtime on an engine with synthetic weights.  Generated ids beyond the test tokenizer's 202 pieces read as <unk> (the
    random model rarely says EOS: every compare decodes the full 20 tokens, the worst case).  recompute=True: `generate` runs
    rk_t5_greedy instead (the A/B)."""
    recompute = False
    n_tok = 202

    def generate(self, seqs, dec_prefix, max_new, eos_id=1, pad_id=0):
        f = T5Runtime.greedy if self.recompute else T5Runtime.generate
        out = np.asarray(f(self, seqs, dec_prefix, max_new, eos_id, pad_id))
        return np.where(out >= self.n_tok, 2, out)


def make_queries(tok, n_queries, n_passages=100, seed=5):
    rs = np.random.RandomState(seed)
    vocab = [w for w in tok.get_vocab() if w.startswith("▁") and w[1:].isalpha() and len(w) > 2]
    words = [w[1:] for w in vocab]
    out = []
    for q in range(n_queries):
        query = " ".join(rs.choice(words, size=4))
        docs = [SearchResult(f"q{q}d{i}", None, " ".join(rs.choice(words, size=int(rs.randint(60, 110))))) for i in range(n_passages)]
        out.append((query, docs))
    return out


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--profile-call", action="store_true")
    ap.add_argument("--llama", action="store_true")
    args = ap.parse_args()
    if args.llama:
        return llama_leg(args)
    from transformers import T5Tokenizer
    tok = T5Tokenizer.from_pretrained(os.path.join(REPO, "tests", "golden", "tok"))
    dims = _synth.FLAN_T5_LARGE
    eng = RkEngine(dims, device=0, max_tokens=49152, max_seqs=64, max_dec_len=24)
    eng.load_state(_synth.synth_tensors(dims, seed=929, threads=16))
    rt = BenchRuntime.from_engine(eng, dims)
    rows = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        rows.append(kw)

    rk = {s: ListwiseLlmRanker.from_runtime(rt, tok, window_size=4, step_size=2, scoring=s, num_repeat=1, max_new=20)
          for s in ("generation", "likelihood")}
    if args.profile_call:
        qs = make_queries(tok, 8)
        rk["generation"]._compare_windows([q for q, _ in qs], [d[96:] for _, d in qs])       # warm: first sighting, capture
        eng.sync()
        ms, _ = timed(lambda: rk["generation"]._compare_windows([q for q, _ in qs], [d[96:] for _, d in qs]))
        emit(what="profile_call", windows=8, ms=ms)
    else:
        sweep(eng, rt, rk, tok, args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def llama_leg(args):
    from llmrankers._engine import RkLlamaEngine
    dims = _synth.LLAMA_3_8B
    L, NEW = 1536, 20
    eng = RkLlamaEngine(dims, device=0, max_tokens=32 * (L + NEW) + 64, max_seqs=32)
    eng.load_state(_synth.synth_tensors_pool(dims, seed=929))
    rows = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        rows.append(kw)

    rs = np.random.RandomState(11)
    prompts = [rs.randint(3, dims.vocab - 28, size=L).astype(np.int32) for _ in range(32)]

    def reprefill(seqs):
        cur = [list(s) for s in seqs]
        for _ in range(NEW):
            nxt = eng.greedy1(cur)
            for c, t in zip(cur, nxt):
                c.append(int(t))
        return cur

    if args.profile_call:
        eng.generate(prompts[:8], NEW, [], 0)
        eng.generate(prompts[:8], NEW, [], 0)                                            # warm: first sighting, capture
        ms, _ = timed(lambda: eng.generate(prompts[:8], NEW, [], 0))
        emit(what="llama_profile_call", rows=8, prompt_tokens=L, new_tokens=NEW, ms=ms)
    else:
        w_bytes = 2.0 * (dims.n_layers * (dims.hidden * (dims.n_heads + 2 * dims.n_kv_heads) * 128 + dims.hidden * dims.n_heads * 128
                                          + 3 * dims.hidden * dims.intermediate) + dims.vocab * dims.hidden)
        for n in (1, 8, 32):
            seqs = prompts[:n]
            for max_new in (1, NEW, NEW):
                eng.generate(seqs, max_new, [], 0)                                         # warm-up: allocation, eager step, capture
            t1 = float(np.median([timed(lambda: eng.generate(seqs, 1, [], 0))[0] for _ in range(3)]))
            t20 = float(np.median([timed(lambda: eng.generate(seqs, NEW, [], 0))[0] for _ in range(3)]))
            eng.greedy1(seqs)
            loop = float(np.median([timed(lambda: reprefill(seqs))[0] for _ in range(3)]))
            step = (t20 - t1) / (NEW - 1)
            kv_bytes = 2.0 * n * (L + NEW / 2) * dims.n_kv_heads * 128 * 2 * dims.n_layers
            emit(what="llama_generate", rows=n, prompt_tokens=L, new_tokens=NEW, prefill_ms=t1, generate_ms=t20, ms_per_step=step,
                 reprefill_loop_ms=loop, speedup=loop / t20, hbm_floor_ms_per_step=(w_bytes + kv_bytes) / 6e12 * 1e3,
                 weight_bytes=w_bytes, kv_bytes=kv_bytes)
        eng.profile(True)                                                                  # per-class split of one 8-row call (eager)
        eng.profile_reset()
        eng.generate(prompts[:8], NEW, [], 0)
        rep = eng.profile_report()
        eng.profile(False)
        emit(what="llama_generate_classes", rows=8, new_tokens=NEW,
             classes={k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in rep.items() if v["launches"]})
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def sweep(eng, rt, rk, tok, args, emit):
    qs = make_queries(tok, 32)
    rk["generation"].rerank(*qs[0])                                                         # warm-up (graphs, LDS opt-ins)
    rk["likelihood"].rerank(*qs[0])
    # whole query, one at a time: generation on the cached decoder vs on the recompute loop, alternated; likelihood
    for r in range(args.rounds):
        for mode in ("generate", "greedy"):
            rt.recompute = mode == "greedy"
            ms, _ = timed(lambda: rk["generation"].rerank(*qs[1 + r]))
            emit(what="query", scoring="generation", engine_call=mode, queries_per_call=1, ms_per_query=ms,
                 compares=rk["generation"].total_compare, completion_tokens=rk["generation"].total_completion_tokens)
        rt.recompute = False
        ms, _ = timed(lambda: rk["likelihood"].rerank(*qs[1 + r]))
        emit(what="query", scoring="likelihood", queries_per_call=1, ms_per_query=ms, compares=rk["likelihood"].total_compare)
    # lockstep sweep
    for n in (8, 32):
        for mode in ("generate", "greedy"):
            rt.recompute = mode == "greedy"
            ms, _ = timed(lambda: rk["generation"].rerank_many(qs[:n]))
            emit(what="lockstep", scoring="generation", engine_call=mode, queries_per_call=n, ms_per_query=ms / n)
        rt.recompute = False
        ms, _ = timed(lambda: rk["likelihood"].rerank_many(qs[:n]))
        emit(what="lockstep", scoring="likelihood", queries_per_call=n, ms_per_query=ms / n)
    # microseconds per decoder step of rk_t5_generate: the same prompts with 20 and with 1 new token
    for n in (1, 32):
        ids = rk["generation"]._truncated_ids([rk["generation"]._permutation_prompt(q, d[96:]) for q, d in qs[:n]])
        for max_new in (1, 20):
            eng.generate(ids, [0], max_new, eos_id=-1)
        t = {}
        for max_new in (1, 20):
            eng.sync()
            t[max_new] = min(timed(lambda: eng.generate(ids, [0], max_new, eos_id=-1))[0] for _ in range(3))
        emit(what="decoder_step", sequences=n, ms_1=t[1], ms_20=t[20], us_per_step=(t[20] - t[1]) / 19 * 1e3)


if __name__ == "__main__":
    main()
