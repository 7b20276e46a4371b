#!/usr/bin/env python
"""What prompt-lookup drafting costs and buys the decoding session on one MI355X (DESIGN.md section 3 "Drafting by prompt lookup").

Llama-3-8B and Qwen2.5-7B dimensions, timing-only pool weights, ONE engine per model; plain (Kd = 0) and drafting sessions alternate
in one process - same weights, same buffers, same clocks.  Every slot holds a prompt of `--prompt` synthetic ids in a session of
`--max-len` positions, so the steps run at positions near the prompt's length.

  figure 1  ms per step at n_slots x Kd, every draft row live (the drafts come from rk_debug_session_drafts, the table being the
            plain session's output, so a step appends and attends Kd + 1 rows per slot): `--steps` steps behind `--warm` warm-up
            steps (the second step captures the graph), median / min / max of `--reps` sessions per shape.
  figure 2  tokens per second with the oracle table corrupted column by column at set rates (a draft is right with probability
            a: acceptance roughly 0 / 25 / 50 / 75 / 100 %): requests of `--new` tokens decoded to the end, tokens the steps emitted
            / wall time of the steps; the plain session beside it.  break_even: the a at which a drafting shape's tokens per second
            cross the plain session's at the same n_slots (linear between the measured rates; null = never inside 0..1).

`--plain-only` (a fresh process; with RK_ENGINE_LIB=<library> a separately compiled one, e.g. the parent commit's, which has none of
the drafting entry points): figure 1 at Kd = 0 alone, to show the plain step did not move.
Real-text acceptance needs a real checkpoint; this tool measures cost and the acceptance needed, not the acceptance a text gives.
Appends one JSON line per model to profiles/llama_draft_bench.txt.  RK_LAYERS shortens the models for a quick look."""
import argparse
import dataclasses
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO, os.path.join(REPO, "tools")]
DRAFT_ENTRIES = ("rk_llama_session_open_draft", "rk_llama_session_stats", "rk_debug_session_drafts")


def _stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _session(eng, n_slots, max_len, cap, kd):
    return eng.session(n_slots, max_len, cap, [], 0, draft=kd) if kd else eng.session(n_slots, max_len, cap, [], 0)


def _plain_output(eng, prompts, max_len, new):
    """the plain session's tokens for these prompts: the oracle table of both figures"""
    with _session(eng, len(prompts), max_len, new, 0) as s:
        s.admit(prompts, list(range(len(prompts))), [new] * len(prompts))
        done = {}
        while len(done) < len(prompts):
            for slot in s.run()[0]:
                done[slot] = [int(t) for t in s.read(slot)]
    return [done[b] for b in range(len(prompts))]


def _corrupt(table, a, vocab, rs):
    return [t if rs.random() < a else (t + 1) % vocab for t in table]


def step_ms(eng, prompts, tables, max_len, kd, warm, steps):
    """one session: admit, warm-up steps, then `steps` steps timed with the stream drained at both ends"""
    cap = (warm + steps + 2) * (kd + 1) + 2
    with _session(eng, len(prompts), max_len, cap, kd) as s:
        if kd:
            for b, t in enumerate(tables):
                s.set_drafts(b, t[:cap])
        s.admit(prompts, list(range(len(prompts))), [cap] * len(prompts))
        assert s.run(warm) == ([], warm)
        t = time.perf_counter()
        fin, n = s.run(steps)
        ms = (time.perf_counter() - t) * 1e3
        assert fin == [] and n == steps, (fin, n)
    return ms / steps


def tokens_per_s(eng, prompts, tables, max_len, kd, new):
    """requests of `new` tokens decoded to the end -> (tokens the steps emitted per second, tokens per step issued)"""
    with _session(eng, len(prompts), max_len, new, kd) as s:
        if kd:
            for b, t in enumerate(tables):
                s.set_drafts(b, t)
        s.admit(prompts, list(range(len(prompts))), [new] * len(prompts))
        left, t, steps = len(prompts), time.perf_counter(), 0
        while left:
            fin, n = s.run()
            steps += n
            left -= len(fin)
        sec = time.perf_counter() - t
    tokens = len(prompts) * (new - 1)
    return tokens / sec, tokens / steps


def _break_even(rates, tps, plain):
    for (a0, y0), (a1, y1) in zip(zip(rates, tps), zip(rates[1:], tps[1:])):
        if (y0 - plain) * (y1 - plain) <= 0 and y1 != y0:
            return round(a0 + (plain - y0) * (a1 - a0) / (y1 - y0), 3)
    return 0.0 if tps[0] >= plain else None


def measure(name, dims, a, plain_only):
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    slots = tuple(int(x) for x in a.slots.split(","))
    kds = (0,) if plain_only else tuple(int(x) for x in a.kd.split(","))
    rows = max(slots) * (max(kds) + 1)
    t0 = time.time()
    eng = RkLlamaEngine(dims, 0, max_tokens=max(max(slots) * a.prompt + 64, a.max_len), max_seqs=rows).load_state(_synth.synth_tensors_pool(dims, seed=929))
    print(f"[bench_llama_draft] {name}: {dims.n_layers} layers generated + loaded in {time.time() - t0:.0f}s", file=sys.stderr)
    out = {"ms_per_step": {}, "tokens_per_s": {}, "break_even_acceptance": {}}
    rs = random.Random(5)
    rates = [float(x) for x in a.rates.split(",")]
    for S in slots:
        prompts = [list(p) for p in _synth.synth_token_batch(S, a.prompt, a.prompt, dims.vocab, seed=3)]
        need = max(a.new, (a.warm + a.steps + 2) * (max(kds) + 1) + 2)
        tables = _plain_output(eng, prompts, a.max_len, need) if not plain_only else [[] for _ in prompts]
        for kd in kds:                                                 # warm-ups: allocations, the graph of every shape
            step_ms(eng, prompts, tables, a.max_len, kd, 2, 2)
        ms = {kd: [] for kd in kds}
        for _ in range(a.reps):                                        # the shapes alternate session by session
            for kd in kds:
                ms[kd].append(step_ms(eng, prompts, tables, a.max_len, kd, a.warm, a.steps))
        for kd in kds:
            out["ms_per_step"][f"slots{S}_kd{kd}"] = _stats(ms[kd])
        print(f"[bench_llama_draft] {name} slots {S}: " + ", ".join(f"Kd {kd}: {statistics.median(ms[kd]):.3f} ms" for kd in kds), file=sys.stderr)
        if plain_only:
            continue
        plain = statistics.median(tokens_per_s(eng, prompts, tables, a.max_len, 0, a.new)[0] for _ in range(a.tps_reps + 1))
        out["tokens_per_s"][f"slots{S}_kd0"] = round(plain, 1)
        for kd in kds[1:]:
            tps = []
            for r in rates:
                tabs = [_corrupt(t[:a.new], r, dims.vocab, rs) for t in tables]
                got = [tokens_per_s(eng, prompts, tabs, a.max_len, kd, a.new) for _ in range(a.tps_reps)]
                tps.append(statistics.median(g[0] for g in got))
                out["tokens_per_s"][f"slots{S}_kd{kd}_a{r}"] = {"tokens_per_s": round(tps[-1], 1), "tokens_per_step": round(got[0][1], 2)}
            out["break_even_acceptance"][f"slots{S}_kd{kd}"] = _break_even(rates, tps, plain)
            print(f"[bench_llama_draft] {name} slots {S} Kd {kd}: plain {plain:.0f} tok/s, drafted {[round(x) for x in tps]} at a = {rates}, "
                  f"break-even {out['break_even_acceptance'][f'slots{S}_kd{kd}']}", file=sys.stderr)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="llama-3-8b,qwen2.5-7b")
    ap.add_argument("--slots", default="1,4,16")
    ap.add_argument("--kd", default="0,1,3,7")
    ap.add_argument("--rates", default="0,0.25,0.5,0.75,1")
    ap.add_argument("--prompt", type=int, default=2040)
    ap.add_argument("--max-len", type=int, default=4096)
    ap.add_argument("--new", type=int, default=192)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tps-reps", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _engine, _synth
    lib = os.environ.get("RK_ENGINE_LIB")
    if lib:
        if not a.plain_only:
            sys.exit("RK_ENGINE_LIB goes with --plain-only")
        for n in DRAFT_ENTRIES:                                        # a library from before the drafting entry points has none of them
            _engine.ABI.pop(n, None)
        import _lib
        _lib.use_env_library()
    for name in a.models.split(","):
        dims = _synth.NAMED_DIMS[name]
        if os.environ.get("RK_LAYERS"):
            dims = dataclasses.replace(dims, n_layers=int(os.environ["RK_LAYERS"]))
        res = {"workload": f"{name} dims, {dims.n_layers} layers, sessions of {a.max_len} positions, prompts of {a.prompt} synthetic ids per slot",
               "mode": "plain sessions only" if a.plain_only else "plain and drafting sessions alternating, oracle draft tables",
               "library": a.label or (lib or "in-tree"), "weights": "pool (timing only)", "reps": a.reps, "steps": a.steps, "new": a.new}
        res.update(measure(name, dims, a, a.plain_only))
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
        with open(os.path.join(REPO, "profiles", "llama_draft_bench.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
