#!/usr/bin/env python
"""Pointwise scoring on decoder-only dimensions on one MI355X: Llama-3.2-1B and Llama-3-8B (timing-only pool weights), through
LlamaRuntime as PointwiseLlmRanker builds it (64 prompts and 32 768 tokens per engine call), one process, medians of three after a
warm-up.  The workload is the headline one: 100 passages of 184 prompt tokens per query, at 1 and 16 queries per call:

  yes_no       LlamaRuntime.score  = rk_llama_last_logits on two vocabulary rows (hf: LlamaForCausalLM logits[:, -1, [yes, no]];
               the decoder-only counterpart of ref: llmrankers/pointwise.py:116-127)
  qlm          LlamaRuntime.qlm_many = rk_llama_qlm with 12 labels behind every prompt (hf: ForCausalLMLoss with -100 on the prompt,
               summed; the counterpart of ref: llmrankers/pointwise.py:73-79)
  last_logits  the same prompt + label sequences through rk_llama_last_logits in the same process: the prefill alone, so that
               qlm - last_logits prices the qlm tail (final norm of the label rows, head GEMM with the log-sum-exp epilogue over the
               whole vocabulary, the merge kernel) on its own

Per leg: ms per call, passages/s, and the fraction of the fp16 MFMA peak by the algorithmic FLOPs (2 x layer parameters x tokens +
causal attention, + the head rows the leg computes).  Appends one JSON line to profiles/llama_pointwise_bench.txt.  The numbers gate
nothing.  RK_LAYERS shortens the models for a quick look; RK_MODELS picks among "llama-3.2-1b,llama-3-8b"."""
import dataclasses
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "llm-rankers_amd"), REPO]
PASSAGES, PROMPT, LABELS, REPS = 100, 184, 12, 3
MFMA_PEAK_TFLOPS = 2500.0


def _median_ms(fn):
    fn()
    times = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times)


def _flops(dims, lens, head_dots):
    q, kv, h, f = dims.n_heads * dims.head_dim, dims.n_kv_heads * dims.head_dim, dims.hidden, dims.intermediate
    per_token = 2.0 * dims.n_layers * (h * (q + 2 * kv) + q * h + 3 * h * f)
    return sum(L * per_token + dims.n_layers * 2.0 * L * L * q for L in lens) + head_dots * 2.0 * h


def run(name, layers):
    import torch  # noqa: F401  (its HIP runtime first)
    from llmrankers import _synth
    from llmrankers._engine import RkLlamaEngine
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.pointwise import POINTWISE_LLAMA_MAX_SEQS
    base = _synth.NAMED_DIMS[name]
    dims = dataclasses.replace(base, n_layers=layers or base.n_layers)
    eng = RkLlamaEngine(dims, 0, max_tokens=32768, max_seqs=POINTWISE_LLAMA_MAX_SEQS).load_state(_synth.synth_tensors_pool(dims, seed=929))
    rt = LlamaRuntime.from_engine(eng, dims)
    out = {"model": name, "layers": dims.n_layers, "weights": "pool (timing only)", "reps": REPS,
           "workload": f"{PASSAGES} passages of {PROMPT} prompt tokens per query; qlm: {LABELS} labels behind each"}
    for queries in (1, 16):
        n = queries * PASSAGES
        prompts = [list(s) for s in _synth.synth_token_batch(n, PROMPT, PROMPT, dims.vocab, seed=3)]
        labels = [list(s) for s in _synth.synth_token_batch(n, LABELS, LABELS, dims.vocab, seed=4)]
        full = [p + l for p, l in zip(prompts, labels)]
        legs = {
            "yes_no": (lambda: rt.score(prompts, [], [42, 43]), [PROMPT] * n, 2 * n),
            "qlm": (lambda: rt.qlm_many(prompts, labels), [PROMPT + LABELS] * n, n * LABELS * dims.vocab),
            "last_logits": (lambda: rt.last_logits(full, [42, 43]), [PROMPT + LABELS] * n, 2 * n),
        }
        res = {}
        for leg, (fn, lens, head_dots) in legs.items():
            ms = _median_ms(fn)
            tf = _flops(dims, lens, head_dots) / ms / 1e9
            res[leg] = {"ms_per_call": round(ms, 2), "passages_per_s": round(n / ms * 1e3, 1), "algorithmic_tflops": round(tf, 1),
                        "frac_of_mfma_peak": round(tf / MFMA_PEAK_TFLOPS, 4)}
        res["qlm_tail_ms"] = round(res["qlm"]["ms_per_call"] - res["last_logits"]["ms_per_call"], 2)
        out[f"queries{queries}"] = res
    eng.close()
    return out


if __name__ == "__main__":
    layers = int(os.environ.get("RK_LAYERS", "0"))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    for model in os.environ.get("RK_MODELS", "llama-3.2-1b,llama-3-8b").split(","):
        line = json.dumps(run(model.strip(), layers))
        print(line, flush=True)
        with open(os.path.join(REPO, "profiles", "llama_pointwise_bench.txt"), "a") as f:
            f.write(line + "\n")
