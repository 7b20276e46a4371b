#!/usr/bin/env python
"""What the sampling head costs on one MI355X: Llama-3-8B dimensions (timing-only pool weights), a prompt of 512 synthetic token
ids, 128 generated tokens with no EOS, at 1 and at 16 rows per engine call, greedy (rk_llama_generate: arg-max head) against
sampled (rk_llama_generate_sampled at the Llama-3-Instruct settings T = 0.6, top_k = 50, top_p = 0.9: fp32 logits +
sample_rows_kernel) in ONE process on one engine, the two alternating:
  ms per step   (call with 129 new tokens - call with 1) / 128, a host clock around calls that end in a device synchronise, median
                of `reps` after a warm-up of every shape (allocations, graph capture).
RK_PARENT_LIB=<librk_engine.so of the parent commit>: the greedy figures are taken again by a fresh child process on that library
(it has none of the sampling entry points), alternating with this build's greedy child, to show that the greedy step's launches
did not change.  Appends one JSON line to profiles/llama_sampling_bench.txt.  RK_LAYERS shortens the model for a quick look."""
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
SAMPLING = (0.6, 50, 0.9)


def bind(path):
    """bind a library that may predate the sampling entry points (the parent commit's): the names it lacks leave the table"""
    import ctypes
    from llmrankers import _engine
    if path:
        lib = ctypes.CDLL(os.path.abspath(path))
        for name in [n for n in _engine.ABI if not hasattr(lib, n)]:
            del _engine.ABI[name]
        _engine.load_library(os.path.abspath(path), make_default=True)


def measure(layers, prompt, new, rows, reps, sampled):
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    dims = dataclasses.replace(_synth.LLAMA_3_8B, n_layers=layers)
    t0 = time.time()
    eng = RkLlamaEngine(dims, 0, max_tokens=max(rows) * (prompt + new) + 64, max_seqs=max(rows)).load_state(_synth.synth_tensors_pool(dims, seed=929))
    print(f"[bench_llama_sampling] {layers} layers generated + loaded in {time.time() - t0:.0f}s", file=sys.stderr)
    if sampled:
        eng.set_sampling(*SAMPLING)

    def call_ms(seqs, n, seeds):
        t = time.perf_counter()
        eng.generate(seqs, n, [], 0, **({"seeds": seeds} if seeds is not None else {}))      # (ends in a device synchronise)
        return (time.perf_counter() - t) * 1e3

    out = {}
    for B in rows:
        seqs = _synth.synth_token_batch(B, prompt, prompt, dims.vocab, seed=3)
        modes = {"greedy": None, **({"sampled": list(range(1, B + 1))} if sampled else {})}
        for seeds in modes.values():                                                          # warm-ups: allocations, graph capture
            call_ms(seqs, new + 1, seeds)
            call_ms(seqs, new + 1, seeds)
            call_ms(seqs, 1, seeds)
        full = {m: [] for m in modes}
        pre = {m: [] for m in modes}
        for _ in range(reps):                                                                 # alternating
            for m, seeds in modes.items():
                full[m].append(call_ms(seqs, new + 1, seeds))
                pre[m].append(call_ms(seqs, 1, seeds))
        out[f"rows{B}"] = {m: {"call_ms": round(statistics.median(full[m]), 2), "prefill_ms": round(statistics.median(pre[m]), 2),
                               "ms_per_step": round((statistics.median(full[m]) - statistics.median(pre[m])) / new, 4),
                               "call_ms_spread": round(max(full[m]) - min(full[m]), 2)} for m in modes}
    eng.close()
    return out


def child(lib, layers, prompt, new, rows, reps):
    """the greedy figures from a fresh process on `lib` (None: the in-tree build)"""
    env = dict(os.environ, RK_BENCH_CHILD="1", RK_BENCH_LIB=lib or "")
    cmd = [sys.executable, os.path.abspath(__file__), str(layers), str(prompt), str(new), ",".join(map(str, rows)), str(reps)]
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=900).stdout
    return json.loads(out.strip().splitlines()[-1])


if __name__ == "__main__":
    if os.environ.get("RK_BENCH_CHILD"):
        layers, prompt, new, rows, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), tuple(map(int, sys.argv[4].split(","))), int(sys.argv[5])
        bind(os.environ.get("RK_BENCH_LIB"))
        print(json.dumps(measure(layers, prompt, new, rows, reps, sampled=False)))
        sys.exit(0)
    layers, prompt, new, rows, reps = int(os.environ.get("RK_LAYERS", "32")), 512, 128, (1, 16), 5
    res = {"workload": f"Llama-3-8B dims, {layers} layers, prefill of {prompt} synthetic token ids + {new} tokens, no EOS; sampled at "
                       f"T, top_k, top_p = {SAMPLING}", "layers": layers, "prompt": prompt, "new": new, "weights": "pool (timing only)", "reps": reps}
    parent = os.environ.get("RK_PARENT_LIB")
    if parent:                                       # children first: one process at a time holds the weights
        res["greedy_parent_commit"] = child(parent, layers, prompt, new, rows, reps)
        res["greedy_this_commit"] = child(None, layers, prompt, new, rows, reps)
    res["this_commit"] = measure(layers, prompt, new, rows, reps, sampled=True)
    for B in rows:
        r = res["this_commit"][f"rows{B}"]
        res[f"sampling_head_ms_per_step_rows{B}"] = round(r["sampled"]["ms_per_step"] - r["greedy"]["ms_per_step"], 4)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "llama_sampling_bench.txt"), "a") as f:
        f.write(line + "\n")
