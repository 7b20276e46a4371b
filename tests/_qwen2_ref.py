"""Test-side Qwen2 references: the fp32 numpy oracle with q / k / v projection biases, a checkpoint-directory loader that knows
`qwen2`, the fp64 LoRA merge, bias outlier channels, and an oracle-backed runtime double with LlamaRuntime's `generate`."""
import json
import os

import numpy as np

from oracle.llama_numpy import LlamaOracle
from _llama_gen_stub import OracleLlamaGenRuntime


class Qwen2Oracle(LlamaOracle):
    """hf: models/qwen2/modeling_qwen2.py: the Llama forward with `bias=True` on q_proj / k_proj / v_proj."""

    def _lin(self, x, name):
        y = x @ self.w[name].T
        b = self.w.get(name[:-6] + "bias")
        return y if b is None else y + b


def load_qwen2_state(path):
    """checkpoint directory -> (LlamaDims, state dict)"""
    from safetensors.numpy import load_file
    from llmrankers import _synth
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    assert cfg["model_type"] in ("qwen2", "llama"), cfg["model_type"]
    return _synth.LlamaDims.from_hf_config(cfg), load_file(os.path.join(path, "model.safetensors"))


def host_merge_lora(state, adapter, scale):
    """W + scale * B @ A in fp64 for every adapter pair (PEFT key layout) -> new fp64-accurate state (fp32 arrays)"""
    out = dict(state)
    names = sorted({k[len("base_model.model."):k.index(".lora_")] for k in adapter})
    for n in names:
        a = np.asarray(adapter[f"base_model.model.{n}.lora_A.weight"], dtype=np.float64)
        b = np.asarray(adapter[f"base_model.model.{n}.lora_B.weight"], dtype=np.float64)
        w = np.asarray(state[n + ".weight"], dtype=np.float64)
        out[n + ".weight"] = (w + float(scale) * (b @ a)).astype(np.float32)
    return out


def merged_state(dims, state, adapter_spec):
    """the recipe's adapter merged into `state` (fp64), as the fixture's oracle saw it"""
    from llmrankers import _synth
    scale = adapter_spec["lora_alpha"] / adapter_spec["r"]
    return host_merge_lora(state, _synth.synth_lora_tensors(dims, adapter_spec), scale)


OUTLIER_K, OUTLIER_Q, OUTLIER_BIAS_GAIN = (5, 40, 77, 101), (9, 70), 40.0


def with_bias_outliers(state):
    """Real Qwen2 checkpoints carry a few bias channels far above the rest: 4 channels of every k bias and 2 of every head of
    every q bias scaled x 40 (fp16-representable, like every synthetic value).  Returns a new dict."""
    out = dict(state)
    for name, b in state.items():
        if name.endswith("k_proj.bias") or name.endswith("q_proj.bias"):
            b = np.array(b, dtype=np.float32, copy=True).reshape(-1, 128)
            ch = list(OUTLIER_K if name.endswith("k_proj.bias") else OUTLIER_Q)
            b[:, ch] = (b[:, ch] * np.float32(OUTLIER_BIAS_GAIN)).astype(np.float16).astype(np.float32)
            out[name] = b.reshape(-1)
    return out


class OracleQwen2GenRuntime(OracleLlamaGenRuntime):
    model_type = "qwen2"

    def __init__(self, dims, state, generation=None):
        super().__init__(dims, state, generation)
        self.orc = Qwen2Oracle(dims, state)
