#!/usr/bin/env python
"""What the q / k head norm costs on one MI355X: Qwen3-8B dimensions (timing-only pool weights), a prompt of 2 048 synthetic token
ids, 128 generated tokens with no EOS (rk_llama_generate: one prefill, then one KV-cached row per token), at 1 and at 8 rows per
engine call.  Each figure is taken twice in ONE process: on the Qwen3 engine (attn_dec_cached_qkn_kernel, rope128_qkn_kernel) and
on an engine of the same dims with qk_norm off (the Llama kernels: attn_dec_cached_kernel, rope128_kernel) -
  ms per generated token   (call with 129 new tokens - call with 1) / 128, median of three after a warm-up;
  prefill rotary per layer the engine's "other" profile class over one rk_llama_last_logits call of the prompt (the rotary kernel is
                           that class's only launch per layer there), divided by the layer count.
Appends one JSON line to profiles/qwen3_bench.txt.  RK_LAYERS shortens the model for a quick look."""
import dataclasses
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]


def measure(dims, prompt, new, rows, reps):
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    t0 = time.time()
    eng = RkLlamaEngine(dims, 0, max_tokens=max(rows) * (prompt + new) + 64, max_seqs=max(rows)).load_state(_synth.synth_tensors_pool(dims, seed=929))
    print(f"[bench_qwen3] qk_norm={dims.qk_norm}: {dims.n_layers} layers generated + loaded in {time.time() - t0:.0f}s", file=sys.stderr)

    def call_ms(seqs, n):
        t = time.perf_counter()
        eng.generate(seqs, n, [], 0)
        return (time.perf_counter() - t) * 1e3

    out = {}
    for B in rows:
        seqs = _synth.synth_token_batch(B, prompt, prompt, dims.vocab, seed=3)
        call_ms(seqs, new + 1)                                                                    # warm-ups: allocations, graph capture
        call_ms(seqs, 1)
        full = statistics.median(call_ms(seqs, new + 1) for _ in range(reps))
        pre = statistics.median(call_ms(seqs, 1) for _ in range(reps))
        eng.last_logits(seqs, [0])
        eng.profile(True); eng.profile_reset()
        eng.last_logits(seqs, [0]); eng.sync()
        rep = eng.profile_report()
        eng.profile(False)
        other = next(v for k, v in rep.items() if "other" in k.lower())
        out[f"rows{B}"] = {"call_ms": round(full, 1), "prefill_ms": round(pre, 1), "ms_per_token": round((full - pre) / new, 4),
                           "prefill_rotary_us_per_layer": round(other["ms"] * 1e3 / dims.n_layers, 2), "prefill_other_launches": other["launches"]}
    eng.close()
    return out


def run(layers=36, prompt=2048, new=128, rows=(1, 8), reps=3):
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _synth
    on = dataclasses.replace(_synth.QWEN3_8B, n_layers=layers)
    off = dataclasses.replace(on, qk_norm=False)
    res = {"workload": f"Qwen3-8B dims, {layers} layers, prefill of {prompt} synthetic token ids + {new} greedy tokens, no EOS (rk_llama_generate)",
           "layers": layers, "prompt": prompt, "new": new, "weights": "pool (timing only)", "reps": reps,
           "qk_norm_off": measure(off, prompt, new, rows, reps), "qk_norm_on": measure(on, prompt, new, rows, reps)}
    for B in rows:
        a, b = res["qk_norm_on"][f"rows{B}"], res["qk_norm_off"][f"rows{B}"]
        res[f"ratio_rows{B}"] = {"ms_per_token": round(a["ms_per_token"] / b["ms_per_token"], 4),
                                 "prefill_rotary": round(a["prefill_rotary_us_per_layer"] / b["prefill_rotary_us_per_layer"], 3)}
    return res


if __name__ == "__main__":
    out = run(layers=int(os.environ.get("RK_LAYERS", "36")))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "qwen3_bench.txt"), "a") as f:
        f.write(line + "\n")
