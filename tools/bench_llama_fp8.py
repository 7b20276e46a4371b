#!/usr/bin/env python
"""What FP8 step weights buy the decoding step on one MI355X (DESIGN.md section 3 "FP8 step weights").

Llama-3-8B and Qwen2.5-7B dimensions, timing-only pool weights, a prompt of 2 048 synthetic token ids, 128 generated tokens with no
EOS (rk_llama_generate: one prefill, then one KV-cached row per sequence and token), at 1, 8 and 16 rows per call.  ONE engine in FP8
mode; option llama_step_fp8 = 1 (the step's four projections read the FP8 bytes, gemm_skinny_fp8_kernel) and 0 (the dequantised fp16
matrices through gemm_skinny_kernel) ALTERNATE call by call in one process - same weights, same buffers, same clocks.
  ms per step   (call with 129 new tokens - median call with 1) / 128; median, min and max of five calls per option.
`--fp16-only` (a fresh process per run; with RK_ENGINE_LIB=<library> a separately compiled one, e.g. the parent commit's, which has
none of the FP8 entry points): the plain fp16 engine's step, to show it did not move.
`--trace` (for a run of its own under a kernel-trace profiler): a shortened model, a few steps of each option, no timing.
Appends one JSON line per run to profiles/llama_fp8_bench.txt.  RK_LAYERS shortens the models for a quick look."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO, os.path.join(REPO, "tools")]
FP8_ENTRIES = ("rk_llama_set_weight_fp8", "rk_debug_quant_fp8", "rk_debug_gemm_fp8")


def _engine(dims, prompt, new, rows, fp8):
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    t0 = time.time()
    kw = {"weight_fp8": True} if fp8 else {}
    eng = RkLlamaEngine(dims, 0, max_tokens=max(rows) * (prompt + new) + 64, max_seqs=max(rows), **kw).load_state(_synth.synth_tensors_pool(dims, seed=929))
    print(f"[bench_llama_fp8] fp8={fp8}: {dims.n_layers} layers generated + loaded in {time.time() - t0:.0f}s", file=sys.stderr)
    return eng


def _call_ms(eng, seqs, n):
    t = time.perf_counter()
    eng.generate(seqs, n, [], 0)
    return (time.perf_counter() - t) * 1e3


def _stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def measure(name, dims, prompt, new, rows, reps, fp8):
    from llmrankers import _synth
    eng = _engine(dims, prompt, new, rows, fp8)
    options = (1, 0) if fp8 else (None,)
    out = {}
    for B in rows:
        seqs = _synth.synth_token_batch(B, prompt, prompt, dims.vocab, seed=3)
        for o in options:                                             # warm-ups: allocations, graph capture (one graph per option epoch)
            if o is not None:
                eng.set_option("llama_step_fp8", o)
            _call_ms(eng, seqs, new + 1)
            _call_ms(eng, seqs, 1)
        pre = statistics.median(_call_ms(eng, seqs, 1) for _ in range(reps))
        full = {o: [] for o in options}
        for _ in range(reps):                                         # the options alternate call by call
            for o in options:
                if o is not None:
                    eng.set_option("llama_step_fp8", o)
                full[o].append(_call_ms(eng, seqs, new + 1))
        rec = {"prefill_ms": round(pre, 1)}
        for o in options:
            rec["fp16_engine" if o is None else ("fp8_bytes" if o else "fp16_kernel")] = _stats([(x - pre) / new for x in full[o]])
        if fp8:
            rec["ratio_fp8_over_fp16"] = round(rec["fp8_bytes"]["median"] / rec["fp16_kernel"]["median"], 4)
        out[f"rows{B}"] = rec
        print(f"[bench_llama_fp8] {name} rows {B}: {rec}", file=sys.stderr)
    eng.close()
    return out


def trace(dims, prompt, rows):
    """a few steps of each option for a kernel trace: the two weight-streaming kernels' durations come from the profiler's statistics"""
    from llmrankers import _synth
    eng = _engine(dims, prompt, 8, (rows,), True)
    seqs = _synth.synth_token_batch(rows, prompt, prompt, dims.vocab, seed=3)
    for o in (1, 0):
        eng.set_option("llama_step_fp8", o)
        eng.set_option("dec_graph", 0)                                # eager launches: one trace record per kernel
        eng.generate(seqs, 9, [], 0)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="llama-3-8b,qwen2.5-7b")
    ap.add_argument("--rows", default="1,8,16")
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fp16-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _engine, _synth
    lib = os.environ.get("RK_ENGINE_LIB")
    if lib:
        if not a.fp16_only:
            sys.exit("RK_ENGINE_LIB goes with --fp16-only")
        for n in FP8_ENTRIES:                                         # a library from before the FP8 entry points has none of them
            _engine.ABI.pop(n, None)
        import _lib
        _lib.use_env_library()
    rows = tuple(int(x) for x in a.rows.split(","))
    for name in a.models.split(","):
        dims = _synth.NAMED_DIMS[name]
        if os.environ.get("RK_LAYERS"):
            dims = dataclasses.replace(dims, n_layers=int(os.environ["RK_LAYERS"]))
        if a.trace:
            trace(dims, a.prompt, rows[0])
            continue
        res = {"workload": f"{name} dims, {dims.n_layers} layers, prefill of {a.prompt} synthetic token ids + {a.new} greedy tokens, no EOS (rk_llama_generate)",
               "mode": "fp16 engine" if a.fp16_only else "FP8 engine, llama_step_fp8 1 / 0 alternating", "library": a.label or (lib or "in-tree"),
               "weights": "pool (timing only)", "reps": a.reps, "ms_per_step": measure(name, dims, a.prompt, a.new, rows, a.reps, not a.fp16_only)}
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
        with open(os.path.join(REPO, "profiles", "llama_fp8_bench.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
