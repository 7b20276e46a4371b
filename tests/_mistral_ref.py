"""Test-side Mistral references: the fp32 numpy oracle with the sliding-window mask (oracle/llama_numpy.py's forward, one line of
its mask changed) and an oracle-backed runtime double with LlamaRuntime's `generate`.

hf: models/mistral/modeling_mistral.py builds its mask by sliding_window_causal_mask: query position i sees keys j with
i - sliding_window < j <= i.  Everything else of the forward is Llama's.  tests/test_mistral_host.py pins this oracle against HF's
MistralForCausalLM in fp32 at a toy window."""
import numpy as np

from oracle.llama_numpy import LlamaOracle, rmsnorm, rope_tables, rotate_half
from _llama_gen_stub import OracleLlamaGenRuntime


class MistralOracle(LlamaOracle):
    """LlamaOracle whose mask also hides the keys at or below i - W (W = dims.sliding_window; 0 = none: LlamaOracle itself)."""

    def hidden_states(self, ids):
        d = self.d
        W = int(getattr(d, "sliding_window", 0) or 0)
        if W <= 0:
            return super().hidden_states(ids)
        L = len(ids)
        h = self.w["model.embed_tokens.weight"][np.asarray(ids, dtype=np.int64)]
        cos, sin = rope_tables(L, d.head_dim, d.rope_theta, getattr(d, "rope_scaling", None))
        i, j = np.arange(L)[:, None], np.arange(L)[None, :]
        hidden = (j > i) | (j <= i - W)
        mask = np.where(hidden, np.float32(np.finfo(np.float32).min), np.float32(0.0))
        rep = d.n_heads // d.n_kv_heads
        for n in range(d.n_layers):
            p = f"model.layers.{n}"
            x = rmsnorm(h, self.w[p + ".input_layernorm.weight"], d.eps)
            q = self._lin(x, p + ".self_attn.q_proj.weight").reshape(L, d.n_heads, d.head_dim).transpose(1, 0, 2)
            k = self._lin(x, p + ".self_attn.k_proj.weight").reshape(L, d.n_kv_heads, d.head_dim).transpose(1, 0, 2)
            v = self._lin(x, p + ".self_attn.v_proj.weight").reshape(L, d.n_kv_heads, d.head_dim).transpose(1, 0, 2)
            q = q * cos[None] + rotate_half(q) * sin[None]
            k = k * cos[None] + rotate_half(k) * sin[None]
            k = np.repeat(k, rep, axis=0)
            v = np.repeat(v, rep, axis=0)
            s = (q @ k.transpose(0, 2, 1)) * np.float32(d.head_dim ** -0.5) + mask[None]
            s = s - s.max(axis=-1, keepdims=True)
            pr = np.exp(s)
            pr = pr / pr.sum(axis=-1, keepdims=True)
            ctx = (pr @ v).transpose(1, 0, 2).reshape(L, d.n_heads * d.head_dim)
            h = h + self._lin(ctx, p + ".self_attn.o_proj.weight")
            x = rmsnorm(h, self.w[p + ".post_attention_layernorm.weight"], d.eps)
            g = self._lin(x, p + ".mlp.gate_proj.weight")
            act = g / (1.0 + np.exp(-g))
            h = h + self._lin(act * self._lin(x, p + ".mlp.up_proj.weight"), p + ".mlp.down_proj.weight")
        return rmsnorm(h, self.w["model.norm.weight"], d.eps)


class OracleMistralGenRuntime(OracleLlamaGenRuntime):
    model_type = "mistral"

    def __init__(self, dims, state, generation=None):
        super().__init__(dims, state, generation)
        self.orc = MistralOracle(dims, state)
