#!/usr/bin/env python
"""What the FP8 K / V cache costs or buys the decoding step on one MI355X (DESIGN.md section 3 "FP8 K/V cache").

Llama-3-8B and Qwen2.5-7B dimensions, timing-only pool weights, decoding sessions (rk_llama_session_*) of 1 / 8 / 16 / 32 slots whose
rows stand at about 2 048 and 4 096 cache positions: every slot is admitted with a synthetic prompt of P - 64 token ids, then the
session's replayed step graph is timed over 16 steps (no EOS).  ONE engine with an FP8 cache; option llama_kv_fp8 = 1 (the step reads
the cache's bytes: attn_dec_kv8_kernel<.., 1>) and 0 (an fp16-layout cache of the dequantised values, attn_dec_kv8_kernel<.., 2>)
ALTERNATE in one process - same weights, same clocks; a change of the option re-lays the cache, so every measurement opens its own
session and admits again (the admit is not timed).
  ms per step    wall time of session.run(16) / 16 behind a warm-up run that captures the graph; median, min and max of `--reps` sessions
  attn ms        one more session per option with the engine's profiler on (eager launches): the dec_attn class's time per step -
                 the chunk kernel and the merge over all layers - the part of the step the cache format changes
`--weight-fp8`: the same with FP8 step weights on.  `--fp16-only` (a fresh process per run; with RK_ENGINE_LIB=<library> a separately
compiled one, e.g. the parent commit's, which has none of the new entry points): the plain fp16 engine's step, to show it did not move.
Appends one JSON line per run to profiles/llama_kv8_bench.txt.  RK_LAYERS shortens the models (the step's time is linear in the layers
but for the head; the ratio of the attention times does not depend on them)."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO, os.path.join(REPO, "tools")]
KV8_ENTRIES = ("rk_llama_set_kv_fp8", "rk_debug_kv8_quant", "rk_debug_kv8_step")
NEW, STEPS, WARM = 64, 16, 4
ADMIT_TOKENS = 65536      # rows of one admit's prefill (its GEMM operands stay below the tiled kernels' 4 GiB panels)


def _engine(dims, P, slots, kv8, w8):
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    t0 = time.time()
    kw = dict({"kv_fp8": True} if kv8 else {}, **({"weight_fp8": True} if w8 else {}))
    eng = RkLlamaEngine(dims, 0, max_tokens=max(ADMIT_TOKENS, max(P)) + 64, max_seqs=max(slots), **kw).load_state(_synth.synth_tensors_pool(dims, seed=929))
    print(f"[bench_llama_kv8] kv_fp8={kv8} weight_fp8={w8}: {dims.n_layers} layers generated + loaded in {time.time() - t0:.0f}s", file=sys.stderr)
    return eng


def _session_ms(eng, seqs, P, profile=False):
    """one session: admit every slot, a warm-up run, then STEPS timed steps -> ms per step (profile: the dec_attn class's ms per step)"""
    n = len(seqs)
    group = max(1, ADMIT_TOKENS // len(seqs[0]))                       # several admits: a prefill of at most ADMIT_TOKENS rows
    with eng.session(n, P, NEW, [], 0) as s:
        for b in range(0, n, group):
            s.admit(seqs[b:b + group], list(range(b, min(b + group, n))), [NEW] * len(seqs[b:b + group]))
        s.run(WARM)
        eng.sync()
        if profile:
            eng.profile(True)
            eng.profile_reset()
            s.run(STEPS)
            eng.sync()
            rep = eng.profile_report()
            eng.profile(False)
            return rep["dec_attn"]["ms"] / STEPS
        t = time.perf_counter()
        _, steps = s.run(STEPS)
        eng.sync()
        assert steps == STEPS, steps
        return (time.perf_counter() - t) * 1e3 / STEPS


def _stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def measure(name, dims, positions, slots, reps, kv8, w8):
    from llmrankers import _synth
    eng = _engine(dims, positions, slots, kv8, w8)
    options = (1, 0) if kv8 else (None,)
    label = {None: "fp16_engine", 1: "fp8_bytes", 0: "rounded_fp16"}
    out = {}
    for P in positions:
        for B in slots:
            seqs = _synth.synth_token_batch(B, P - NEW, P - NEW, dims.vocab, seed=3)
            ms = {o: [] for o in options}
            for _ in range(reps):                                     # the options alternate session by session
                for o in options:
                    if o is not None:
                        eng.set_option("llama_kv_fp8", o)
                    ms[o].append(_session_ms(eng, seqs, P))
            rec = {label[o]: _stats(ms[o]) for o in options}
            for o in options:
                if o is not None:
                    eng.set_option("llama_kv_fp8", o)
                rec[label[o] + "_attn_ms"] = round(_session_ms(eng, seqs, P, profile=True), 4)
            if kv8:
                rec["ratio_bytes_over_rounded"] = round(rec["fp8_bytes"]["median"] / rec["rounded_fp16"]["median"], 4)
                rec["attn_ratio_bytes_over_rounded"] = round(rec["fp8_bytes_attn_ms"] / rec["rounded_fp16_attn_ms"], 4)
            out[f"P{P}_slots{B}"] = rec
            print(f"[bench_llama_kv8] {name} P {P} slots {B}: {rec}", file=sys.stderr)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="llama-3-8b,qwen2.5-7b")
    ap.add_argument("--slots", default="1,8,16,32")
    ap.add_argument("--positions", default="2048,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--weight-fp8", action="store_true")
    ap.add_argument("--fp16-only", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _engine, _synth
    lib = os.environ.get("RK_ENGINE_LIB")
    if lib:
        if not a.fp16_only:
            sys.exit("RK_ENGINE_LIB goes with --fp16-only")
        for n in KV8_ENTRIES:                                         # a library from before the FP8 cache has none of its entry points
            _engine.ABI.pop(n, None)
        import _lib
        _lib.use_env_library()
    slots = tuple(int(x) for x in a.slots.split(","))
    positions = tuple(int(x) for x in a.positions.split(","))
    for name in a.models.split(","):
        dims = _synth.NAMED_DIMS[name]
        if os.environ.get("RK_LAYERS"):
            dims = dataclasses.replace(dims, n_layers=int(os.environ["RK_LAYERS"]))
        res = {"workload": f"{name} dims, {dims.n_layers} layers, sessions of {list(slots)} slots admitted with P - {NEW} synthetic token ids, {STEPS} timed steps, no EOS (rk_llama_session_run)",
               "mode": ("fp16 engine" if a.fp16_only else "FP8-cache engine, llama_kv_fp8 1 / 0 alternating") + (", FP8 step weights" if a.weight_fp8 else ""),
               "library": a.label or (lib or "in-tree"), "weights": "pool (timing only)", "reps": a.reps,
               "ms_per_step": measure(name, dims, positions, slots, a.reps, not a.fp16_only, a.weight_fp8)}
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
        with open(os.path.join(REPO, "profiles", "llama_kv8_bench.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
