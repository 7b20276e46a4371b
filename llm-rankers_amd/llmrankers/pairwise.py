"""Pairwise ranking prompting (PRP) on the MI355X engine: allpair / heapsort / bubblesort over "which of the two
passages is more relevant" calls.

Drop-in for ref: llmrankers/pairwise.py:29-295 (PairwiseLlmRanker, T5 family) — same constructor, prompt, `compare()`
contract (two prompts, A/B and B/A, decoded generations returned), counters and result assembly.  The model call is the
same primitive the setwise ranker uses: greedy continuation of "<pad> Passage" by two tokens (rk_t5_greedy), here for
the two orderings of a pair in one engine call, and for `allpair` for as many pairs as fit the engine's capacity at
once (the reference's batch_size only shapes its host loop and the padded-shape counters, reproduced arithmetically).
Llama-family checkpoints (ref: pairwise.py:60-77, 104-129) take the decoder-only path of the setwise ranker: chat-template
prompt + " Passage:", prefill and ONE greedy token per ordering (rk_llama_greedy1), outputs "Passage <token>"; `allpair`
is T5-only there too (it reads `self.decoder_input_ids`, which the reference only sets for T5: AttributeError).

DuoT5LlmRanker (ref: llmrankers/pairwise.py:296-352) is the monoT5-style pairwise ranker: both orderings of a pair through the
model at one decoder position, softmax over the logits of `false` / `true`, the first passage wins iff its P(true) is strictly
larger.  The whole tail of a compare runs on the device (rk_t5_compare), and heapsorts of several queries advance in lock step.
"""
from itertools import combinations
from typing import List

import numpy as np

from ._batching import batches, padded_token_count, tokenize_prompts
from ._lockstep import Lockstep, alternate, drive, heapsort_steps
from .pointwise import _softmax_first
from .rankers import KvDtypeOption, LlmRanker, SearchResult, close_counters, rerank_each, tally, top_k_then_rest

PROMPT = ('Given a query "{query}", which of the following two passages is more relevant to the query?\n\n'
          'Passage A: "{doc1}"\n\nPassage B: "{doc2}"\n\nOutput Passage A or Passage B:')
WIN = ["Passage A", "Passage B"]       # the first passage of the pair wins iff the A/B prompt says A and the B/A prompt says B


def sift(arr, n, i):
    """Sift node i of the binary max-heap arr[:n] down (ref: pairwise.py:133-147, a loop instead of tail recursion), as a chain
    of _lockstep: yields one ordered pair [(a, b)] at a time and is sent its verdict `a > b`.  At most two compares per level,
    in this order: (left, i) then (right, largest)."""
    while True:
        largest, left, right = i, 2 * i + 1, 2 * i + 2
        if left < n:
            (gt,) = yield [(arr[left], arr[i])]
            if gt:
                largest = left
        if right < n:
            (gt,) = yield [(arr[right], arr[largest])]
            if gt:
                largest = right
        if largest == i:
            return
        arr[i], arr[largest] = arr[largest], arr[i]
        i = largest


class PairwiseLlmRanker(KvDtypeOption, LlmRanker):
    needs_decoder_positions = True            # PRP generates two tokens behind "<pad> Passage" (DuoT5LlmRanker: one position)

    def __init__(self, model_name_or_path, tokenizer_name_or_path, device, method="allpair", batch_size=2, k=10,
                 cache_dir=None, weight_dtype="fp16"):
        # ref: pairwise.py:30-82: T5 or Llama family by config.model_type, NotImplementedError otherwise
        # weight_dtype (not in the reference): "fp8" = FP8 step weights on a Llama-family checkpoint (LlamaRuntime; lossy, opt-in)
        from ._runtime import kv_dtype_kw, load_runtime, weight_dtype_kw
        try:
            runtime = load_runtime(model_name_or_path, device, cache_dir=cache_dir, **weight_dtype_kw(weight_dtype), **kv_dtype_kw(self.kv_dtype))
        except NotImplementedError as exc:
            raise NotImplementedError(f"{exc} (pairwise)") from None
        if runtime.model_type == "llama":
            from transformers import AutoTokenizer
            from .setwise import VICUNA_TEMPLATE
            tokenizer = AutoTokenizer.from_pretrained(model_name_or_path, cache_dir=cache_dir)   # (the reference ignores tokenizer_name_or_path here)
            tokenizer.use_default_system_prompt = False
            if 'v1.5' in model_name_or_path:       # the reference's `'vicuna' and 'v1.5' in name` (ref :62)
                tokenizer.chat_template = VICUNA_TEMPLATE
            tokenizer.pad_token = "[PAD]"          # ref :65-66 (never used: both orderings of a pair are scored unpadded)
            tokenizer.padding_side = "left"
        else:
            from transformers import T5Tokenizer
            tokenizer = T5Tokenizer.from_pretrained(
                tokenizer_name_or_path if tokenizer_name_or_path is not None else model_name_or_path, cache_dir=cache_dir)
        self._setup(runtime, tokenizer, device, method, batch_size, k)

    @classmethod
    def from_runtime(cls, runtime, tokenizer, device="cuda", method="allpair", batch_size=2, k=10):
        """Build the ranker around an existing runtime (a loaded engine, or a test double) and tokenizer."""
        self = cls.__new__(cls)
        self._setup(runtime, tokenizer, device, method, batch_size, k)
        return self

    def _setup(self, runtime, tokenizer, device, method, batch_size, k):
        if self.needs_decoder_positions:
            from ._runtime import require_decoder_positions
            require_decoder_positions(runtime, type(self).__name__)
        self.device, self.method, self.batch_size, self.k = device, method, batch_size, k
        self.prompt = PROMPT
        self.llm, self.tokenizer = runtime, tokenizer
        self.config = getattr(runtime, "config", None)
        self.model_type = getattr(runtime, "model_type", "t5")
        if self.model_type == "t5":                         # (ref :53-56: only the T5 branch has a decoder prompt)
            self.decoder_input_ids = self.tokenizer.encode("<pad> Passage", add_special_tokens=False)
            # the two labels a generation normally starts with: hint for the one-pass two-token greedy (rk_t5_greedy2)
            self._label_ids = [self.tokenizer.encode(f"<pad> Passage {c}", add_special_tokens=False)[-1] for c in "AB"]
        self.total_compare = 0
        self.total_completion_tokens = 0
        self.total_prompt_tokens = 0

    # -- the model call --------------------------------------------------------------------------------------
    def _generate(self, token_lists: List[List[int]]):
        """Greedy, max_new_tokens=2, continuing "<pad> Passage" for every prompt.  Returns (texts, new_lens): the decoded
        generation of each row (prefix included, specials skipped - what batch_decode gives the reference) and the
        number of new tokens each row needed (EOS included), from which the reference's batch-level output length
        follows: HF stops a batch when all its rows have finished."""
        eos, pad = self.tokenizer.eos_token_id, self.tokenizer.pad_token_id
        if getattr(self.llm, "supports_greedy_candidates", False):
            new = np.asarray(self.llm.greedy(token_lists, self.decoder_input_ids, 2, eos, pad, candidates=self._label_ids))
        else:
            new = np.asarray(self.llm.greedy(token_lists, self.decoder_input_ids, 2, eos, pad))
        texts, lens = [], []
        for row in new:
            toks = [int(t) for t in row if t >= 0]
            n = toks.index(eos) + 1 if eos in toks else 2
            lens.append(n)
            texts.append(self.tokenizer.decode(list(self.decoder_input_ids) + toks[:n], skip_special_tokens=True))
        return texts, lens

    def compare(self, query: str, docs: List):
        # ref: pairwise.py:84-131 — docs = the two passage TEXTS; both orderings in one call
        self.total_compare += 1
        texts = [self.prompt.format(query=query, doc1=docs[0], doc2=docs[1]),
                 self.prompt.format(query=query, doc1=docs[1], doc2=docs[0])]
        if self.model_type == "llama":
            # ref :104-129: chat template + " Passage:", one greedy token per ordering.  The reference tokenises the two prompts
            # into ONE tensor without padding - they hold the same words in another order and normally the same number of
            # tokens (it raises when they do not; here the counters then take the longer one, as a padded batch would)
            ids = []
            for t in texts:
                prompt = self.tokenizer.apply_chat_template([{"role": "user", "content": t}], tokenize=False, add_generation_prompt=True)
                ids.append(list(self.tokenizer(prompt + " Passage:")["input_ids"]))
            width = max(len(x) for x in ids)
            self.total_prompt_tokens += len(ids) * width
            toks = self.llm.greedy1(ids)
            self.total_completion_tokens += len(ids) * (width + 1)      # generate() returns prompt + new token
            return [f"Passage {self.tokenizer.decode([int(t)], skip_special_tokens=True).strip().upper()}" for t in toks]
        ids = tokenize_prompts(self.tokenizer, texts)
        self.total_prompt_tokens += padded_token_count(ids)                 # padding='longest' (ref :93-97)
        out, lens = self._generate(ids)
        self.total_completion_tokens += len(ids) * (len(self.decoder_input_ids) + max(lens))
        return out

    def _first_wins(self, query, a_text, b_text) -> bool:
        return self.compare(query, [a_text, b_text]) == WIN

    # -- sort drivers --------------------------------------------------------------------------------------------
    def _allpair(self, query, ranking):
        # ref: pairwise.py:169-216 — every unordered pair in both orders, one generation each; a win needs both
        # orderings to agree, anything else is half a point each
        pairs = list(combinations(ranking, 2))
        prompts = []
        for d1, d2 in pairs:
            prompts.append(self.prompt.format(query=query, doc1=d1.text, doc2=d2.text))
            prompts.append(self.prompt.format(query=query, doc1=d2.text, doc2=d1.text))
        seqs = tokenize_prompts(self.tokenizer, prompts)
        outputs, lens = self._generate(seqs) if seqs else ([], [])
        for s, e in batches(len(seqs), self.batch_size):        # the reference's batches only shape its counters
            self.total_compare += 1
            self.total_prompt_tokens += padded_token_count(seqs[s:e])
            self.total_completion_tokens += (e - s) * (len(self.decoder_input_ids) + max(lens[s:e]))
        scores = {}
        for i, (d1, d2) in enumerate(pairs):
            o1, o2 = outputs[2 * i], outputs[2 * i + 1]
            if o1 == "Passage A" and o2 == "Passage B":
                scores[d1.docid] = scores.get(d1.docid, 0.0) + 1
            elif o1 == "Passage B" and o2 == "Passage A":
                scores[d2.docid] = scores.get(d2.docid, 0.0) + 1
            else:
                scores[d1.docid] = scores.get(d1.docid, 0.0) + 0.5
                scores[d2.docid] = scores.get(d2.docid, 0.0) + 0.5
        # documents enter in the order they first score (dict order) and the sort is stable, as in the reference
        return sorted([SearchResult(docid=d, score=s, text=None) for d, s in scores.items()], key=lambda x: x.score, reverse=True)

    def rerank(self, query: str, ranking: List[SearchResult]) -> List[SearchResult]:
        # ref: pairwise.py:164-295
        original_docids = [doc.docid for doc in ranking]      # (the reference deep-copies the list; only the docid order is read)
        self.total_compare = 0
        self.total_completion_tokens = 0
        self.total_prompt_tokens = 0
        if self.method == "allpair":
            ranking = self._allpair(query, ranking)
        elif self.method == "heapsort":
            arr = list(ranking)                                # ref: pairwise.py:149-162, one compare at a time
            drive(heapsort_steps(arr, self.k, 2, sift, False), lambda pairs: [self._first_wins(query, a.text, b.text) for a, b in pairs])
            ranking = [SearchResult(docid=d.docid, score=-i, text=None) for i, d in enumerate(reversed(arr))]
        elif self.method == "bubblesort":
            # ref: pairwise.py:246-269 — the reference's variant that skips pairs already known to be in order
            k = min(self.k, len(ranking))
            last_end = len(ranking) - 1
            for i in range(k):
                cur, changed = last_end, False
                while cur > i:
                    if self._first_wins(query, ranking[cur].text, ranking[cur - 1].text):
                        ranking[cur - 1], ranking[cur] = ranking[cur], ranking[cur - 1]
                        if not changed:
                            changed = True
                            if last_end != len(ranking) - 1:
                                last_end += 1
                    if not changed:
                        last_end -= 1
                    cur -= 1
        else:
            raise NotImplementedError(f'Method {self.method} is not implemented.')
        return top_k_then_rest(ranking, original_docids, self.k)

    def truncate(self, text, length):
        return self.tokenizer.convert_tokens_to_string(self.tokenizer.tokenize(text)[:length])


DUO_PROMPT = 'Query: {query} Document0: {doc1} Document1: {doc2} Relevant:'
HF_NO_LIMIT = int(1e20)      # transformers' LARGE_INTEGER: a model_max_length above it means "no limit", nothing is truncated


class DuoT5LlmRanker(PairwiseLlmRanker):
    """duoT5 (ref: llmrankers/pairwise.py:296-352): heapsort over "is document 0 more relevant than document 1" compares.  One
    compare = the A/B and the B/A prompt at ONE decoder position (decoder_start_token_id), softmax over the logits of `false` /
    `true` per ordering, verdict P(true)[A/B] > P(true)[B/A] - strict, a tie is False.  On the engine the logits, the softmax and
    the verdict of every pair of a call come from the device (T5Runtime.compare_pairs, rk_t5_compare); a runtime without it gives
    the four logits through `score` and the softmax runs on the host.  Same constructor, counters (completion tokens stay 0) and
    result assembly as the reference; the caller's list is not reordered."""
    FALSE_ID, TRUE_ID = 6136, 1176            # the ids of "false" / "true" in the T5 vocabulary (ref :314-315)
    fp16_scores = False                       # True: the host verdict from the returned logits, rounded as the reference's fp16 model does
    needs_decoder_positions = False

    @classmethod
    def with_kv_dtype(cls, kv_dtype):            # duoT5 serves T5 checkpoints: "fp8" is refused by name, "fp16" changes nothing
        from ._runtime import refuse_t5_kv_dtype
        refuse_t5_kv_dtype(kv_dtype)
        return cls

    def _setup(self, runtime, tokenizer, device, method, batch_size, k):
        super()._setup(runtime, tokenizer, device, method, batch_size, k)
        if self.model_type != "t5":
            raise NotImplementedError(f"Model type {self.model_type} is not supported yet for duoT5 :(")
        # heapsort build phase: the independent sift-downs of a tree level share an engine call (same array, set of compares and
        # counters as the reference's one-by-one order)
        self.batch_independent_compares = True

    # -- the model call ------------------------------------------------------------------------------------------
    def _pair_ids(self, queries, pairs) -> List[List[int]]:
        """Token ids of the two prompts of every (a_text, b_text) pair, A/B then B/A: tokenizer(inputs, truncation=True) - each
        sequence cut to tokenizer.model_max_length with the EOS kept (ref :303; 512 for the published duoT5 tokenizers), nothing
        cut when the tokenizer carries transformers' "no limit" value."""
        texts = []
        for q, (a, b) in zip(queries, pairs):
            texts.append(DUO_PROMPT.format(query=q, doc1=a, doc2=b))
            texts.append(DUO_PROMPT.format(query=q, doc1=b, doc2=a))
        ids = tokenize_prompts(self.tokenizer, texts)
        limit = getattr(self.tokenizer, "model_max_length", None)
        if limit is not None and 0 < limit <= HF_NO_LIMIT:
            limit = int(limit)
            ids = [seq if len(seq) <= limit else seq[:limit - 1] + seq[-1:] for seq in ids]
        return ids

    def _decoder_start(self) -> int:
        start = getattr(self.llm, "decoder_start_token_id", None)
        if start is None:
            start = (self.config or {}).get("decoder_start_token_id", 0)
        return int(start)

    def _verdicts(self, result) -> List[bool]:
        """compare_pairs' triple (or bare logits [2n, 2] of a runtime without it) -> the n verdicts."""
        if isinstance(result, tuple):
            logits, _, wins = result
            if not self.fp16_scores:
                return [bool(w) for w in wins]
        else:
            logits = result
        logits = np.asarray(logits, dtype=np.float32)
        p_true = _softmax_first(logits[:, 1], logits[:, 0], self.fp16_scores)
        return [bool(a > b) for a, b in zip(p_true[0::2], p_true[1::2])]

    def _compare_pairs(self, queries, pairs):
        """The engine call behind `compare`, for pairs that may belong to different queries -> (verdicts, prompt tokens per
        compare); touches no counter."""
        ids = self._pair_ids(queries, pairs)
        prompt_tokens = [padded_token_count(ids[i:i + 2]) for i in range(0, len(ids), 2)]     # padding=True (ref :303, :308)
        if getattr(self.llm, "supports_compare_pairs", False):
            result = self.llm.compare_pairs(ids, self._decoder_start(), self.FALSE_ID, self.TRUE_ID)
        else:
            result = self.llm.score(ids, [self._decoder_start()], [self.FALSE_ID, self.TRUE_ID])
        return self._verdicts(result), prompt_tokens

    def compare(self, query: str, docs: List) -> bool:
        # ref: pairwise.py:297-318 — docs = the two passage TEXTS
        self.total_compare += 1
        self.prompt = DUO_PROMPT
        (verdict,), (prompt_tokens,) = self._compare_pairs([query], [(docs[0], docs[1])])
        self.total_prompt_tokens += prompt_tokens
        return verdict

    # ---- the same compare, launched and collected separately (a runtime with batch slots) -------------------------
    def _can_alternate(self) -> bool:
        return (getattr(self, "alternate_groups", True) and hasattr(self.llm, "compare_async")
                and getattr(getattr(self.llm, "engine", None), "num_slots", 1) >= 2)

    def _launch_pairs(self, queries, pairs, slot: int):
        """First half of `_compare_pairs`: ONE engine call enqueued on `slot`; None when the pairs do not fit one call."""
        ids = self._pair_ids(queries, pairs)
        handle = self.llm.compare_async(ids, self._decoder_start(), self.FALSE_ID, self.TRUE_ID, slot)
        if handle is None:
            return None
        return handle, [padded_token_count(ids[i:i + 2]) for i in range(0, len(ids), 2)]

    def _collect_pairs(self, launched):
        handle, prompt_tokens = launched
        return self._verdicts(self.llm.compare_collect(handle)), prompt_tokens

    def _batched_ok(self) -> bool:
        # sharing an engine call needs compare() to be ours (no subclass / instance override)
        return (getattr(self, "batch_independent_compares", False) and "compare" not in self.__dict__
                and type(self).compare is DuoT5LlmRanker.compare)

    def _compare_many(self, query, windows) -> List[bool]:
        """Independent compares of one query in ONE engine call: same verdicts and counters as `compare()` on each in turn."""
        verdicts, prompt_tokens = self._compare_pairs([query] * len(windows), [(a.text, b.text) for a, b in windows])
        self.total_compare += len(windows)
        self.total_prompt_tokens += sum(prompt_tokens)
        return verdicts

    def rerank(self, query: str, ranking: List[SearchResult]) -> List[SearchResult]:
        # ref: pairwise.py:320-352.  The sort works on a new list: the caller's is left as it is.
        original_docids = [doc.docid for doc in ranking]
        self.total_compare = 0
        self.total_completion_tokens = 0
        self.total_prompt_tokens = 0
        if self.method != "heapsort":
            raise NotImplementedError(f'Method {self.method} is not implemented.')
        arr = list(ranking)
        # the binary heapsort with the build phase level-batched (one `_compare_many` per yielded list of pairs); a replaced
        # compare() gets the reference's order, one pair at a time (looked up on the instance: tests and subclasses replace it)
        level_batched = self._batched_ok()
        drive(heapsort_steps(arr, self.k, 2, sift, level_batched),
              (lambda pairs: self._compare_many(query, pairs)) if level_batched
              else (lambda pairs: [self.compare(query, [a.text, b.text]) for a, b in pairs]))
        return top_k_then_rest(list(reversed(arr)), original_docids, self.k)

    # ---- several queries at once ---------------------------------------------------------------------------
    def rerank_many(self, items):
        """Several queries at once: `items` = [(query, ranking), ...] -> (results, counters); results[i] and counters[i] =
        (total_compare, total_prompt_tokens, total_completion_tokens) are exactly what `rerank(*items[i])` gives.  A query's
        heapsort is several hundred DEPENDENT compares of two sequences each; the chains of different queries are independent, so
        their pending compares share an engine call, one call per step of all the chains (a pair's verdict does not depend on
        what shares its call: ragged execution, bit-exact).  With at least four live chains on a runtime with batch slots two
        groups alternate over them, as in SetwiseLlmRanker.rerank_many; a round that does not fit one engine call takes the
        blocking call for that round.  A replaced compare(), or fewer than two queries: one rerank per query."""
        items = list(items)
        if self.method != "heapsort" or not self._batched_ok() or len(items) < 2:
            return rerank_each(self, items)
        originals = [[doc.docid for doc in ranking] for _, ranking in items]
        arrs = [list(ranking) for _, ranking in items]
        counts = [[0, 0, 0] for _ in items]
        chains = Lockstep({q: heapsort_steps(arr, self.k, 2, sift, True) for q, arr in enumerate(arrs)})

        def call_args(keys, windows):
            return [items[q][0] for q in keys], [(a.text, b.text) for a, b in windows]

        def blocking(keys, windows):
            return tally(counts, keys, *self._compare_pairs(*call_args(keys, windows)))

        if len(chains.live()) >= 4 and self._can_alternate():
            # two groups of chains alternate over the engine's two batch slots: while one group's call is on the GPU the host
            # advances the other group's heaps, tokenises its prompts and launches them; a round that does not fit one engine
            # call (the build phase of many long heaps) goes through the blocking call, which cuts it
            alternate(chains, lambda keys, windows, slot: self._launch_pairs(*call_args(keys, windows), slot=slot),
                      lambda keys, launched: tally(counts, keys, *self._collect_pairs(launched)), blocking)
        while chains:
            chains.advance(blocking(*chains.pending()))
        results = [top_k_then_rest(list(reversed(arr)), original, self.k) for arr, original in zip(arrs, originals)]
        return results, close_counters(self, counts)
