"""Test-side reference of the pointwise scores on decoder-only checkpoints: the log-likelihood of a continuation (qlm) and P(yes)
(yes_no), evaluated in fp64 on the hidden states of the family oracles the tests already have - oracle/llama_numpy.LlamaOracle and its
Qwen2 / Qwen3 / Mistral subclasses (tests/_qwen2_ref.py, _qwen3_ref.py, _mistral_ref.py) - over the fp16-representable weights the
engine loads.  Never the engine.

hf: models/llama/modeling_llama.py LlamaForCausalLM.forward with labels: loss_utils.ForCausalLMLoss shifts the labels by one, ignores
-100 and takes cross_entropy of logits[t - 1] against token t.  With -100 on the prompt and reduction "none", summed and negated:

    score = sum_{j = 0 .. n - 1}  z[p + j - 1][tok[p + j]] - logsumexp(z[p + j - 1])        (p = len - n, natural logarithm)

the decoder-only counterpart of ref: llmrankers/pointwise.py:73-79.

Tolerances, from the project's own number.  The Llama prefill is held to |logit - oracle| < BOUND x scale with BOUND = 4e-3
(tests/test_gpu_rankr1.py).  A label term is a logit minus a log-sum-exp; the log-sum-exp is 1-Lipschitz in the maximum norm, so each
is off by at most that bound and a score by 2 n BOUND scale, scale = the reference's largest |logit| over the sequence's label rows.
P(yes) = sigmoid(z_yes - z_no): slope at most 1/4 times a difference off by 2 BOUND scale = BOUND scale / 2, scale = the largest
|logit| of the row behind the prompt.

MUTANTS are the ways the arithmetic above is usually got wrong; tests/test_llama_pointwise_host.py shows that each is more than five
tolerances away on the inputs the tests use, i.e. that the tolerance can tell them apart."""
import numpy as np

from oracle.llama_numpy import LlamaOracle

BOUND = 4e-3
MUTANTS = ("own_position", "drop_last", "first_from_p", "lse_over_labels", "log2")


def family_oracle(dims, state):
    """the oracle of the dims' family"""
    if getattr(dims, "qk_norm", False):
        from _qwen3_ref import Qwen3Oracle
        return Qwen3Oracle(dims, state)
    if getattr(dims, "qkv_bias", False):
        from _qwen2_ref import Qwen2Oracle
        return Qwen2Oracle(dims, state)
    if getattr(dims, "sliding_window", 0):
        from _mistral_ref import MistralOracle
        return MistralOracle(dims, state)
    return LlamaOracle(dims, state)


def head64(orc):
    w = orc.w["model.embed_tokens.weight"] if orc.d.tied_head else orc.w["lm_head.weight"]
    return np.asarray(w, dtype=np.float64)


def logits64(orc, ids, rows=None):
    """fp64 logits [len(rows), vocab] of the positions `rows` (default: all) of one sequence"""
    h = np.asarray(orc.hidden_states(list(ids)), dtype=np.float64)
    return (h if rows is None else h[np.asarray(rows, dtype=np.int64)]) @ head64(orc).T


def _lse(z):
    m = z.max(axis=-1)
    return m + np.log(np.exp(z - m[..., None]).sum(axis=-1))


def loglik_from_logits(z, ids, n_labels, mut=None):
    """The score of one sequence from its fp64 logits z [len, vocab] -> (score, scale).  mut: one of MUTANTS."""
    ids = np.asarray(ids, dtype=np.int64)
    L, n = len(ids), int(n_labels)
    assert 1 <= n < L
    p = L - n
    lab = ids[p:]
    rows = np.arange(p - 1, L - 1)
    scale = float(np.abs(z[rows]).max())
    if mut == "own_position":
        rows = rows + 1
    elif mut == "first_from_p":
        rows = rows.copy()
        rows[0] = p
    zr = z[rows]
    lse = _lse(zr[:, np.unique(lab)]) if mut == "lse_over_labels" else _lse(zr)
    terms = zr[np.arange(n), lab] - lse
    if mut == "drop_last":
        terms = terms[:-1]
    score = float(terms.sum())
    return (score / np.log(2.0) if mut == "log2" else score), scale


def loglik(orc, ids, n_labels, mut=None):
    return loglik_from_logits(logits64(orc, ids), ids, n_labels, mut)


def qlm_tolerance(n_labels, scale):
    return 2.0 * int(n_labels) * BOUND * float(scale)


def p_yes(orc, ids, yes_id, no_id):
    """(P(yes), scale) behind the prompt `ids`: softmax over the two logits of the last row, fp64"""
    z = logits64(orc, ids, rows=[len(ids) - 1])[0]
    return float(1.0 / (1.0 + np.exp(-(z[yes_id] - z[no_id])))), float(np.abs(z).max())


def yes_no_tolerance(scale):
    return BOUND * float(scale) / 2.0


def min_gap(scores):
    """smallest gap between adjacent scores of the sorted list (inf for fewer than two)"""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    return float(np.diff(s).min()) if len(s) > 1 else float("inf")


# ---- end to end: the ranker's inputs and what the reference says of them ----------------------------------------------------------------
E2E_WORDS = ("ocean river carbon energy solar policy market health vaccine protein neural network language model search query passage "
             "ranking climate water forest city history music science data study result method patient school price trade law court food "
             "soil").split()
# (toy, tokenizer, method) -> the seed of e2e_inputs: of the seeds 0 .. 399 the one whose smallest gap between adjacent reference
# scores, over its queries, is the widest in tolerances (8.4, 4.9 and 7.0) - above the 4 the ranking test asks for, so that no query
# is left out.  Found on the reference alone; tests/test_llama_pointwise_host.py re-checks it.  The toys' weights are random, so a
# passage moves a score little: three passages and two queries are what clears the cap.
# tok_qwen maps "Yes" and "No" to one id - every P(yes) is 0.5 - so yes_no runs on tok_llama only.
E2E_SEEDS = {("toy-llama", "tok_llama", "yes_no"): 361, ("toy-llama", "tok_llama", "qlm"): 190, ("toy-qwen2", "tok_qwen", "qlm"): 274}
E2E_MIN_GAP = 4.0


def e2e_inputs(seed, n_passages=3, n_queries=2):
    """(queries, passages): words of the toy tokenizers' vocabulary, drawn from the seed"""
    rs = np.random.RandomState(seed)
    passages = [" ".join(rs.choice(E2E_WORDS, size=int(rs.randint(2, 7)))) for _ in range(n_passages)]
    queries = [" ".join(rs.choice(E2E_WORDS, size=int(rs.randint(1, 3)))) for _ in range(n_queries)]
    return queries, passages


def chat_prompt_ids(tok, text):
    """one user turn through the chat template with the generation prompt, then the tokenizer (the ranker's rule, restated)"""
    return list(tok(tok.apply_chat_template([{"role": "user", "content": text}], tokenize=False, add_generation_prompt=True))["input_ids"])


def e2e_expected(tok, orc, method, query, passages):
    """(fp64 reference scores [n], the largest tolerance among them, prompt lengths, dec_len) of one query"""
    from llmrankers.pointwise import QLM_PROMPT, YES_NO_PROMPT
    if method == "qlm":
        labels = tok.encode(query, add_special_tokens=False)
        seqs = [chat_prompt_ids(tok, QLM_PROMPT.format(text=t)) for t in passages]
        got = [loglik(orc, s + labels, len(labels)) for s in seqs]
        return np.asarray([g[0] for g in got]), max(qlm_tolerance(len(labels), g[1]) for g in got), [len(s) for s in seqs], len(labels)
    yes, no = tok.encode("Yes", add_special_tokens=False)[0], tok.encode("No", add_special_tokens=False)[0]
    seqs = [chat_prompt_ids(tok, YES_NO_PROMPT.format(text=t, query=query)) for t in passages]
    got = [p_yes(orc, s, yes, no) for s in seqs]
    return np.asarray([g[0] for g in got]), max(yes_no_tolerance(g[1]) for g in got), [len(s) for s in seqs], 0


class OraclePointwiseRuntime:
    """The three calls PointwiseLlmRanker makes on a decoder-only runtime (LlamaRuntime.score / qlm / qlm_many), answered by the
    oracle: the CPU suite's stand-in for the engine, as tests/_stub.py is for T5.  `calls` records (name, sequences) per call."""

    def __init__(self, dims, state, model_type=None):
        self.dims, self.orc, self.config = dims, family_oracle(dims, state), dims.to_hf_config()
        self.model_type = model_type or self.config["model_type"]
        self.calls = []

    def score(self, seqs, dec_prefix, out_ids):
        assert len(dec_prefix) == 0, "a decoder-only model takes no decoder prefix"
        self.calls.append(("score", len(seqs)))
        if not len(seqs):
            return np.zeros((0, len(out_ids)), np.float32)
        oi = np.asarray(out_ids, dtype=np.int64)
        return np.stack([logits64(self.orc, s, rows=[len(s) - 1])[0][oi] for s in seqs]).astype(np.float32)

    def qlm(self, seqs, labels):
        return self.qlm_many(seqs, [labels] * len(seqs))

    def qlm_many(self, seqs, labels_per_seq):
        self.calls.append(("qlm_many", len(seqs)))
        out = np.zeros(len(seqs), np.float32)
        for b, (s, lab) in enumerate(zip(seqs, labels_per_seq)):
            if len(lab):
                out[b] = loglik(self.orc, list(s) + list(lab), len(lab))[0]
        return out
