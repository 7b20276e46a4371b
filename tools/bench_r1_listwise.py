#!/usr/bin/env python
"""Mistral-7B dimensions (Zephyr / RankZephyr: 32 heads on 8 kv heads of 128, sliding_window 4096; timing-only pool weights) on one
MI355X, one process, medians of three after a warm-up - the R1 listwise ranker's three regimes, each on an engine WITH the window and
on one WITHOUT it (the same build, the same weights):

  compare_3k  one 20-passage compare's prefill = rk_llama_greedy1 on a 3 072-token prompt: the window is idle (the plain kernels run)
  compare_6k  a 6 144-token prompt: the windowed prefill kernel against the plain one at the same length, whole call and attention
              per layer (the engine's profile class enc_attn: ms / launches of one greedy1 call) - the window can only remove work
  decode      rk_llama_generate at one row, prompts of 2 048 / 4 096 / 8 192 tokens: ms per token
              ((call with 33 new tokens - call with 1) / 32)

Appends one JSON line to profiles/r1_listwise_bench.txt.  The numbers gate nothing.  RK_LAYERS shortens the model for a quick look."""
import dataclasses
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
NEW, REPS = 33, 3
DECODE_AT = (2048, 4096, 8192)


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _median(fn):
    fn()
    return round(statistics.median(_ms(fn) for _ in range(REPS)), 3)


def _attn_per_layer(eng, seqs):
    eng.greedy1(seqs)
    eng.profile(True)
    eng.profile_reset()
    eng.greedy1(seqs)
    eng.sync()
    rep = eng.profile_report()["enc_attn"]
    eng.profile(False)
    return round(rep["ms"] / max(rep["launches"], 1), 4)


def _leg(dims):
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    eng = RkLlamaEngine(dims, 0, max_tokens=max(DECODE_AT) + NEW + 64, max_seqs=2).load_state(_synth.synth_tensors_pool(dims, seed=929))
    out = {"sliding_window": dims.sliding_window}
    for tag, n in (("compare_3k", 3072), ("compare_6k", 6144)):
        one = _synth.synth_token_batch(1, n, n, dims.vocab, seed=3)
        out[tag] = {"prompt": n, "greedy1_ms": _median(lambda: eng.greedy1(one)), "attn_ms_per_layer": _attn_per_layer(eng, one)}
    out["decode"] = {}
    for n in DECODE_AT:
        one = _synth.synth_token_batch(1, n, n, dims.vocab, seed=3)
        eng.generate(one, NEW, [], 0)                                    # warm-up: allocations, graph capture
        pre = _median(lambda: eng.generate(one, 1, [], 0))
        full = _median(lambda: eng.generate(one, NEW, [], 0))
        out["decode"][str(n)] = {"prefill_ms": pre, "ms_per_token": round((full - pre) / (NEW - 1), 4)}
    eng.close()
    return out


def run(layers):
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _synth
    dims = dataclasses.replace(_synth.MISTRAL_7B, n_layers=layers)
    out = {"workload": f"mistral-7b dims, {layers} layers, pool weights (timing only), one row of synthetic token ids", "reps": REPS,
           "windowed": _leg(dims), "window_off": _leg(dataclasses.replace(dims, sliding_window=0))}
    w, p = out["windowed"], out["window_off"]
    out["compare_6k_windowed_over_plain"] = round(w["compare_6k"]["greedy1_ms"] / p["compare_6k"]["greedy1_ms"], 3)
    out["attn_6k_windowed_over_plain"] = round(w["compare_6k"]["attn_ms_per_layer"] / p["compare_6k"]["attn_ms_per_layer"], 3)
    return out


if __name__ == "__main__":
    res = run(int(os.environ.get("RK_LAYERS", "32")))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "r1_listwise_bench.txt"), "a") as f:
        f.write(line + "\n")
