"""Oracle-backed stand-in for LlamaRuntime with the incremental decoder's interface: `generate` = greedy continuation by repeated
LlamaOracle.last_logits (fp32, the whole prompt every step), the engine runtime's stop rules and -1 convention."""
import numpy as np

from oracle.llama_numpy import LlamaOracle


def oracle_greedy(orc, prompt, max_new, eos_ids=(), max_total=0):
    """(new tokens up to and including the stop, top-1 / top-2 margin of every step) of one prompt"""
    cur, toks, margins = [int(t) for t in prompt], [], []
    for _ in range(max_new):
        lg = orc.last_logits([cur])[0]
        s = np.sort(lg)
        margins.append(float(s[-1] - s[-2]))
        nxt = int(np.argmax(lg))
        toks.append(nxt)
        cur.append(nxt)
        if nxt in eos_ids or (max_total and len(cur) >= max_total):
            break
    return toks, margins


class OracleLlamaGenRuntime:
    model_type = "llama"

    def __init__(self, dims, state, generation=None):
        from llmrankers._runtime import read_generation_settings
        self.dims, self.orc, self.config = dims, LlamaOracle(dims, state), dims.to_hf_config()
        self.generation = generation if generation is not None else read_generation_settings(None, self.config)
        self.calls = []

    def greedy1(self, seqs):
        return self.orc.greedy1(seqs)

    def generate(self, seqs, max_new, eos_ids, pad_id, max_total=0):
        self.calls.append(len(seqs))
        out = np.full((len(seqs), max_new), pad_id, dtype=np.int32)
        steps = 0
        for b, s in enumerate(seqs):
            toks, _ = oracle_greedy(self.orc, s, max_new, tuple(eos_ids), max_total)
            out[b, :len(toks)] = toks
            steps = max(steps, len(toks))
        out[:, steps:] = -1
        return out
