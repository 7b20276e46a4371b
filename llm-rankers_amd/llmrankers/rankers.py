"""Public result record and ranker base class — the outer drop-in surface.

Mirrors ref: llmrankers/rankers.py:5-17 (field names, positional order and method names are the contract
`run.py` and library users rely on: ref run.py:176,192-195; README.md:38-54).
"""
from dataclasses import dataclass
from typing import List, Optional


@dataclass
class SearchResult:
    """One candidate of a first-stage ranking.  `text` is None in setwise results (ref: setwise.py:306,310)."""
    docid: str
    score: float
    text: Optional[str]


def top_k_then_rest(ordered, original_docids, k) -> List[SearchResult]:
    """Result assembly of the sorting rankers (ref: setwise.py:299-313, pairwise.py:281-295): the first k of `ordered` with
    score -rank, then every other docid in the caller's original order, ranks running on."""
    results, top = [], set()
    for doc in ordered[:k]:
        top.add(doc.docid)
        results.append(SearchResult(docid=doc.docid, score=-(len(results) + 1), text=None))
    for docid in original_docids:
        if docid not in top:
            results.append(SearchResult(docid=docid, score=-(len(results) + 1), text=None))
    return results


def rerank_each(ranker, items):
    """The fallback of every `rerank_many`: one `rerank` per query -> (results, the counters each call left)."""
    out, counters = [], []
    for query, ranking in items:
        out.append(ranker.rerank(query, ranking))
        counters.append((ranker.total_compare, ranker.total_prompt_tokens, ranker.total_completion_tokens))
    return out, counters


def tally(counts, keys, answers, prompt_tokens, completion_tokens=None):
    """One answered compare per key: counts[q] = [compares, prompt tokens, completion tokens] of query q; -> answers."""
    for q, p, c in zip(keys, prompt_tokens, completion_tokens or [0] * len(keys)):
        counts[q][0] += 1
        counts[q][1] += p
        counts[q][2] += c
    return answers


def close_counters(ranker, counts):
    """-> the per-query counters as tuples; the ranker's own totals are the last query's, as after one `rerank` per query."""
    counters = [tuple(c) for c in counts]
    if counters:
        ranker.total_compare, ranker.total_prompt_tokens, ranker.total_completion_tokens = counters[-1]
    return counters


class KvDtypeOption:
    """The rankers that decode on a Llama-family checkpoint (setwise, pairwise, listwise and the two Rank-R1 rankers): an FP8 K / V
    cache for the decoding step (LlamaRuntime's kv_dtype; lossy, opt-in).  Their constructors keep their parameter lists, so the
    option is the class's: Cls.with_kv_dtype("fp8")(model, ...); a T5 checkpoint refuses "fp8" as it refuses weight_dtype="fp8"."""
    kv_dtype = "fp16"

    @classmethod
    def with_kv_dtype(cls, kv_dtype):
        from ._runtime import class_with_kv_dtype
        return class_with_kv_dtype(cls, kv_dtype)


class LlmRanker:
    """Interface every ranker implements: rerank a candidate list for a query; truncate text by tokens."""

    def rerank(self, query: str, ranking: List[SearchResult]) -> List[SearchResult]:
        raise NotImplementedError

    def truncate(self, text: str, length: int) -> str:
        raise NotImplementedError
