"""Host logic for T5 models with 128-wide heads (t5-3b): the registered dimensions, and which rankers accept a runtime that serves
one decoder position only - without a GPU (a stub runtime on the numpy oracle)."""
import os

import pytest

from conftest import GOLD
from llmrankers import _synth


def test_named_dims():
    d = _synth.NAMED_DIMS["t5-3b"]
    assert d is _synth.T5_3B
    assert (d.vocab, d.d_model, d.n_heads, d.d_kv, d.d_ff, d.n_enc, d.n_dec, d.gated, d.tied_head) == (32128, 1024, 32, 128, 16384, 24, 24, False, True)
    assert d.inner == 4096
    t = _synth.NAMED_DIMS["toy-monot5-d128"]
    assert t is _synth.TOY_MONOT5_D128
    assert (t.vocab, t.d_model, t.n_heads, t.d_kv, t.d_ff, t.n_enc, t.n_dec, t.gated, t.tied_head) == (6144, 128, 3, 128, 256, 2, 2, False, True)
    assert _synth.T5Dims.from_hf_config(t.to_hf_config()) == t


@pytest.fixture(scope="module")
def stub():
    from transformers import T5Tokenizer
    from _stub import OracleRuntime
    dims = _synth.TOY_MONOT5_D128
    rt = OracleRuntime(dims, _synth.synth_state_dict(dims, seed=24, gain=1.0))
    rt.one_position_only = True
    return rt, T5Tokenizer.from_pretrained(os.path.join(GOLD, "tok"))


def test_rankers_beyond_one_position_refuse_at_construction(stub):
    from llmrankers.listwise import ListwiseLlmRanker
    from llmrankers.pairwise import PairwiseLlmRanker
    from llmrankers.pointwise import PointwiseLlmRanker
    from llmrankers.setwise import SetwiseLlmRanker
    rt, tok = stub
    for build in (lambda: PointwiseLlmRanker.from_runtime(rt, tok, method="qlm"), lambda: SetwiseLlmRanker.from_runtime(rt, tok),
                  lambda: ListwiseLlmRanker.from_runtime(rt, tok), lambda: PairwiseLlmRanker.from_runtime(rt, tok)):
        with pytest.raises(NotImplementedError, match="d_kv=128"):
            build()
    rt.one_position_only = False                          # the same runtime without the flag: every one of them builds
    try:
        for build in (lambda: PointwiseLlmRanker.from_runtime(rt, tok, method="qlm"), lambda: SetwiseLlmRanker.from_runtime(rt, tok),
                      lambda: ListwiseLlmRanker.from_runtime(rt, tok), lambda: PairwiseLlmRanker.from_runtime(rt, tok)):
            build()
    finally:
        rt.one_position_only = True


def test_one_position_rankers_run_on_the_oracle(stub):
    """MonoT5LlmRanker (whatever `method` says), yes_no and DuoT5LlmRanker build on a one-position runtime and rank"""
    from llmrankers.pairwise import DuoT5LlmRanker
    from llmrankers.pointwise import MonoT5LlmRanker, PointwiseLlmRanker
    from llmrankers.rankers import SearchResult
    rt, tok = stub
    docs = [SearchResult(docid=f"d{i}", score=float(9 - i), text=t) for i, t in enumerate(("river law court", "neural model batch", "market price trade"))]
    for rk in (MonoT5LlmRanker.from_runtime(rt, tok), MonoT5LlmRanker.from_runtime(rt, tok, method="yes_no", batch_size=2),
               PointwiseLlmRanker.from_runtime(rt, tok, method="yes_no"), DuoT5LlmRanker.from_runtime(rt, tok, method="heapsort", k=2)):
        res = rk.rerank("model list", list(docs))
        assert sorted(r.docid for r in res) == ["d0", "d1", "d2"]
