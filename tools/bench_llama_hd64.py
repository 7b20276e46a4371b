#!/usr/bin/env python
"""Llama-3.2-1B dimensions (64-wide heads, timing-only pool weights) on one MI355X, one process, medians of three after a warm-up:

  compare     one setwise compare = rk_llama_greedy1 on a 1 536-token prompt
  generate    rk_llama_generate at 1 and 8 rows of 1 536 tokens: the prefill (call with 1 new token) and ms per step
              ((call with 65 new tokens - call with 1) / 64)
  attention   the prefill attention per layer from the engine's profile classes (enc_attn ms / launches of one greedy1 call):
              attn_causal_tile_kernel<64> at 32 / 8 heads of 64 next to attn_causal_tile_kernel<128> (option llama_attn_dma = 0) and the LDS-DMA
              kernel (= 1) on a twin model with 16 / 4 heads of 128 - equal FLOPs, equal q width, the same prompt

Appends one JSON line to profiles/llama_hd64_bench.txt.  The numbers gate nothing.  RK_LAYERS shortens the model for a quick look."""
import dataclasses
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
PROMPT, NEW, REPS = 1536, 65, 3


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


def run(layers):
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    dims = dataclasses.replace(_synth.LLAMA_32_1B, n_layers=layers)
    out = {"workload": f"Llama-3.2-1B dims, {layers} layers, pool weights (timing only), prompts of {PROMPT} synthetic token ids", "reps": REPS}
    eng = RkLlamaEngine(dims, 0, max_tokens=8 * (PROMPT + NEW) + 64, max_seqs=8).load_state(_synth.synth_tensors_pool(dims, seed=929))
    one = _synth.synth_token_batch(1, PROMPT, PROMPT, dims.vocab, seed=3)
    out["compare_ms"] = _median(lambda: eng.greedy1(one))
    for rows in (1, 8):
        seqs = _synth.synth_token_batch(rows, PROMPT, PROMPT, dims.vocab, seed=3)
        eng.generate(seqs, NEW, [], 0)                                   # warm-up: allocations, graph capture
        pre = _median(lambda: eng.generate(seqs, 1, [], 0))
        full = _median(lambda: eng.generate(seqs, NEW, [], 0))
        out[f"rows{rows}"] = {"prefill_ms": pre, "ms_per_step": round((full - pre) / (NEW - 1), 4)}
    out["attn_causal64_ms_per_layer"] = _attn_per_layer(eng, one)
    eng.close()
    twin = dataclasses.replace(dims, n_heads=16, n_kv_heads=4, head_dim=128, n_layers=min(layers, 4))
    eng = RkLlamaEngine(twin, 0, max_tokens=PROMPT + 64, max_seqs=2).load_state(_synth.synth_tensors_pool(twin, seed=929))
    for tag, dma in (("attn_causal128_ms_per_layer", 0), ("attn_causal128_dma_ms_per_layer", 1)):
        eng.set_option("llama_attn_dma", dma)
        out[tag] = _attn_per_layer(eng, one)
    eng.close()
    out["attn_64_over_plain_128"] = round(out["attn_causal64_ms_per_layer"] / out["attn_causal128_ms_per_layer"], 3)
    return out


if __name__ == "__main__":
    res = run(int(os.environ.get("RK_LAYERS", "16")))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "llama_hd64_bench.txt"), "a") as f:
        f.write(line + "\n")
