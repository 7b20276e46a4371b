#!/usr/bin/env python
"""One Rank-R1 compare on one MI355X: Qwen2.5-7B dimensions (timing-only pool weights), a chat prompt of 20 passages x ~100 tokens
(2 100 tokens), 256 generated tokens with no EOS (rk_llama_generate: one prefill, then one KV-cached row per token), at 1 row
(num_permutation = 1) and 8 rows per engine call.  Reports ms per generated token - (call with 256 new tokens - call with 1) / 255,
median of three after a warm-up, one process - next to the floor of streaming the fp16 weights and the rows' K / V once per step at
the 6 TB/s DESIGN.md uses, with the decode attention at all G = 7 query heads of a kv head per workgroup (option llama_dec_r = 2) and
at one (llama_dec_r = 1, what plan_llama_dec_attn's rule gives G = 7): the A/B behind that rule.  The prompt is 2 100 synthetic
token ids per row, not a tokenised chat prompt (timing only).  RK_LAYERS shortens the model for a quick look."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
HBM_BYTES_PER_S = 6.0e12


def run(layers=28, prompt=2100, new=256, rows=(1, 8), reps=3):
    import dataclasses
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    dims = dataclasses.replace(_synth.QWEN25_7B, n_layers=layers)
    t0 = time.time()
    eng = RkLlamaEngine(dims, 0, max_tokens=max(rows) * (prompt + new) + 64, max_seqs=max(rows)).load_state(_synth.synth_tensors_pool(dims, seed=929))
    print(f"[bench_rankr1] {layers} layers generated + loaded in {time.time() - t0:.0f}s", file=sys.stderr)
    q, kv, h, f = dims.n_heads * 128, dims.n_kv_heads * 128, dims.hidden, dims.intermediate
    weight_bytes = 2.0 * (layers * (h * (q + 2 * kv) + q * h + 3 * h * f) + h * dims.vocab)      # every projection and the head, fp16
    out = {"workload": f"Qwen2.5-7B dims, {layers} layers, Rank-R1 compare = prefill of {prompt} synthetic token ids (the length of a 20-passage chat prompt) + {new} greedy tokens, no EOS "
                       "(rk_llama_generate)", "layers": layers, "prompt": prompt, "new": new, "weights": "pool (timing only)", "reps": reps}

    def call_ms(seqs, n):
        t = time.perf_counter()
        eng.generate(seqs, n, [], 0)
        return (time.perf_counter() - t) * 1e3

    for B in rows:
        seqs = _synth.synth_token_batch(B, prompt, prompt, dims.vocab, seed=3)
        kv_bytes = B * layers * 2.0 * kv * (prompt + new / 2.0) * 2.0
        res = {"floor_ms_per_token": round((weight_bytes + kv_bytes) / HBM_BYTES_PER_S * 1e3, 3)}
        for tag, r in (("R=G", 2), ("R=1", 1)):
            eng.set_option("llama_dec_r", r)
            call_ms(seqs, new)                                                                   # warm-ups: allocations, graph capture
            call_ms(seqs, 1)
            full = statistics.median(call_ms(seqs, new) for _ in range(reps))
            pre = statistics.median(call_ms(seqs, 1) for _ in range(reps))
            res[tag] = {"call_ms": round(full, 1), "prefill_ms": round(pre, 1), "ms_per_token": round((full - pre) / (new - 1), 3)}
        eng.set_option("llama_dec_r", 0)
        eng.profile(True); eng.profile_reset()
        eng.generate(seqs, 9, [], 0); eng.sync()
        res["classes_ms_9_tokens"] = {k: round(v["ms"], 2) for k, v in eng.profile_report().items() if v["launches"]}
        eng.profile(False)
        out[f"rows{B}"] = res
    eng.close()
    return out


if __name__ == "__main__":
    print(json.dumps(run(layers=int(os.environ.get("RK_LAYERS", "28")))))
