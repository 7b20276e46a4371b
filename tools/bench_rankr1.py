#!/usr/bin/env python
"""One Rank-R1 compare on one MI355X: Qwen2.5-7B dimensions (timing-only pool weights), a chat prompt of 20 passages x ~100 tokens
(2 100 tokens), 256 generated tokens with no EOS (rk_llama_generate: one prefill, then one KV-cached row per token), at 1 row
(num_permutation = 1) and 8 rows per engine call.  Reports ms per generated token - (call with 256 new tokens - call with 1) / 255,
median of three after a warm-up, one process - next to the floor of streaming the fp16 weights and the rows' K / V once per step at
the 6 TB/s DESIGN.md uses, with the decode attention at all G = 7 query heads of a kv head per workgroup (option llama_dec_r = 2) and
at one (llama_dec_r = 1, what plan_llama_dec_attn's rule gives G = 7): the A/B behind that rule.  The prompt is 2 100 synthetic
token ids per row, not a tokenised chat prompt (timing only).  RK_LAYERS shortens the model for a quick look.

--session: the decoding session (rk_llama_session_*, DecodePool).  24 requests of 2 100 ids, each with its own max_new from a fixed
list spread over 64 .. 512 (no EOS: a row ends at its max_new, so slots free at different steps), through a pool of 1 / 4 / 8 / 16
slots: aggregate generated tokens/s, mean step ms, the share of slot-steps that produced no token, admits.
--one-at-a-time [--package-root DIR]: the same requests one by one through rk_llama_generate, three repeats - run it on the
commit before the session (DIR = a tree that holds that commit's llm-rankers_amd with its built library) for the baseline."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv else REPO
sys.path[:0] = [os.path.join(ROOT, "llm-rankers_amd"), ROOT]
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


# 24 values spread over 64 .. 512, in an order that mixes short and long rows (fixed: the same requests in every leg)
SESSION_MAX_NEW = (512, 64, 288, 160, 448, 96, 352, 224, 128, 480, 256, 192, 416, 80, 320, 112, 384, 144, 496, 208, 272, 72, 464, 176)


def _session_engine(layers, prompt, slots):
    import dataclasses
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    dims = dataclasses.replace(_synth.QWEN25_7B, n_layers=layers)
    t0 = time.time()
    eng = RkLlamaEngine(dims, 0, max_tokens=slots * prompt + 1024, max_seqs=slots).load_state(_synth.synth_tensors_pool(dims, seed=929))
    print(f"[bench_rankr1] {layers} layers generated + loaded in {time.time() - t0:.0f}s", file=sys.stderr)
    reqs = _synth.synth_token_batch(len(SESSION_MAX_NEW), prompt, prompt, dims.vocab, seed=3)
    return eng, reqs


def run_one_at_a_time(layers=28, prompt=2100, reps=3):
    """the requests one by one through rk_llama_generate (whatever commit the imported package is)"""
    eng, reqs = _session_engine(layers, prompt, 1)
    eng.generate([reqs[0]], 64, [], 0); eng.generate([reqs[0]], 64, [], 0)       # warm-up: allocations, graph capture
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        for r, m in zip(reqs, SESSION_MAX_NEW):
            eng.generate([r], m, [], 0)
        runs.append(time.perf_counter() - t)
    eng.close()
    total = sum(SESSION_MAX_NEW)
    return {"leg": "one at a time, rk_llama_generate", "package": ROOT, "layers": layers, "prompt": prompt, "requests": len(reqs),
            "generated_tokens": total, "seconds": [round(x, 3) for x in runs], "tokens_per_s": [round(total / x, 1) for x in runs]}


def run_session(layers=28, prompt=2100, slot_counts=(1, 4, 8, 16)):
    from llmrankers._runtime import LlamaRuntime
    eng, reqs = _session_engine(layers, prompt, max(slot_counts))
    rt = LlamaRuntime.from_engine(eng)
    total = sum(SESSION_MAX_NEW)
    out = {"leg": "decoding session (DecodePool)", "layers": layers, "prompt": prompt, "requests": len(reqs), "generated_tokens": total, "slots": {}}

    def drain(n_slots, n_requests):
        t_wait = 0.0
        with rt.open_pool(max_new_cap=max(SESSION_MAX_NEW), eos_ids=[], pad_id=0, n_slots=n_slots) as pool:
            for i in range(n_requests):
                pool.submit(i, reqs[i], SESSION_MAX_NEW[i])
            got = 0
            t = time.perf_counter()
            while pool.pending():
                for key, tokens in pool.wait():
                    assert len(tokens) == SESSION_MAX_NEW[key]
                    got += len(tokens)
            t_wait = time.perf_counter() - t
            return t_wait, got, pool.steps, pool.admits, pool.opens

    for n_slots in slot_counts:
        drain(n_slots, min(len(reqs), 2 * n_slots))                               # warm-up: allocations, the step graph of this size
        sec, got, steps, admits, opens = drain(n_slots, len(reqs))
        # a request's first token comes from its admit: steps * slots slot-steps produced (got - requests) tokens
        idle = 1.0 - (got - len(reqs)) / float(steps * n_slots)
        out["slots"][n_slots] = {"seconds": round(sec, 3), "tokens_per_s": round(got / sec, 1), "steps": steps, "admits": admits,
                                 "session_opens": opens, "idle_slot_step_share": round(idle, 3),
                                 "ms_per_step_incl_admits": round(sec / steps * 1e3, 3)}
        # the step alone: a full pool of equal rows, timed between two finishes (no admit inside)
        with eng.session(n_slots, prompt + 256, 128, [], 0) as s:
            s.admit(reqs[:n_slots], list(range(n_slots)), [100] * n_slots)
            s.run(20)
            t = time.perf_counter()
            _, n = s.run(60)
            out["slots"][n_slots]["ms_per_step"] = round((time.perf_counter() - t) / n * 1e3, 3)
    eng.close()
    return out


if __name__ == "__main__":
    layers = int(os.environ.get("RK_LAYERS", "28"))
    if "--session" in sys.argv:
        print(json.dumps(run_session(layers=layers)))
    elif "--one-at-a-time" in sys.argv:
        print(json.dumps(run_one_at_a_time(layers=layers)))
    else:
        print(json.dumps(run(layers=layers)))
