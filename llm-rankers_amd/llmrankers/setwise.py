"""Setwise ranker on the MI355X engine: c-ary heapsort / bubblesort over an LLM "which passage is most relevant" call.

Drop-in for ref: llmrankers/setwise.py:21-316 (SetwiseLlmRanker) — same constructor, `compare()` contract,
counters, fallbacks for malformed model output and result assembly.  Each compare is one encoder pass over a
single long prompt plus either two greedy decoder steps (`scoring='generation'`, engine call rk_t5_greedy) or
one label-row read at decoder position 1 (`scoring='likelihood'`, rk_t5_score with the 23 label ids).
Llama-family models (ref: setwise.py:60-69,159-177): chat-template prompt + " Passage:", prefill and ONE greedy token
(rk_llama_greedy1); `likelihood` scoring raises NotImplementedError for them exactly as in the reference.
"""
import random
from collections import Counter
from typing import List

import numpy as np

from ._batching import tokenize_prompts
from ._lockstep import Lockstep, alternate, drive, heapsort_steps
from .rankers import KvDtypeOption, LlmRanker, SearchResult, close_counters, rerank_each, tally, top_k_then_rest

random.seed(929)   # same import-time seeding as the reference (ref: setwise.py:18): permutation voting depends on it

# the chat template the reference installs for vicuna-v1.5 checkpoints (ref: setwise.py:63-64) — data, quoted as is
VICUNA_TEMPLATE = ("{% if messages[0]['role'] == 'system' %}{% set loop_messages = messages[1:] %}{% set system_message = messages[0]['content'] %}"
                   "{% else %}{% set loop_messages = messages %}{% set system_message = 'A chat between a curious user and an artificial intelligence "
                   "assistant. The assistant gives helpful, detailed, and polite answers to the user\\'s questions.' %}{% endif %}"
                   "{% for message in loop_messages %}{% if (message['role'] == 'user') != (loop.index0 % 2 == 0) %}"
                   "{{ raise_exception('Conversation roles must alternate user/assistant/user/assistant/...') }}{% endif %}"
                   "{% if loop.index0 == 0 %}{{ system_message }}{% endif %}{% if message['role'] == 'user' %}{{ ' USER: ' + message['content'].strip() }}"
                   "{% elif message['role'] == 'assistant' %}{{ ' ASSISTANT: ' + message['content'].strip() + eos_token }}{% endif %}{% endfor %}"
                   "{% if add_generation_prompt %}{{ ' ASSISTANT:' }}{% endif %}")

QUESTION = 'Given a query "{query}", which of the following passages is the most relevant one to the query?\n\n'
INSTRUCTION = '\n\nOutput only the passage label of the most relevant passage:'


def vote(refs, answers, characters, say, rng=random):
    """The permutation vote (ref: setwise.py:132-150, 520-548): refs[p] = (docids, labels) of permutation p, answers[p] what
    the model said to it.  Answers that name no label of their permutation are reported through `say` and dropped; the docid
    named most often wins, a tie is broken by one `rng.choice` (the module-level `random` like the reference, unless the caller
    brings a generator of its own); no usable answer at all -> "Unexpected voting."."""
    candidates = []
    for (docids, labels), answer in zip(refs, answers):
        if answer not in labels:
            say(f"Unexpected output: {answer}")
            continue
        candidates.append(docids[labels.index(answer)])
    if len(candidates) == 0:
        return "Unexpected voting."
    counts = Counter(candidates)
    top = max(counts.values())
    winners = [c for c, v in counts.items() if v == top]
    return characters[winners[0] if len(winners) == 1 else rng.choice(winners)]


class SetwiseLlmRanker(KvDtypeOption, LlmRanker):
    # "Passage X" / "Passage Y" tokenize into 3 tokens with the T5 vocabulary, hence 23 labels (ref: setwise.py:22-23)
    CHARACTERS = ["A", "B", "C", "D", "E", "F", "G", "H", "I", "J", "K", "L",
                  "M", "N", "O", "P", "Q", "R", "S", "T", "U", "V", "W"]

    def __init__(self, model_name_or_path, tokenizer_name_or_path, device, num_child=3, k=10, scoring='generation',
                 method="heapsort", num_permutation=1, cache_dir=None, weight_dtype="fp16"):
        # ref: setwise.py:25-77: T5 or Llama family by config.model_type, NotImplementedError otherwise
        # weight_dtype (not in the reference): "fp8" = FP8 step weights on a Llama-family checkpoint (LlamaRuntime; lossy, opt-in)
        from ._runtime import kv_dtype_kw, load_runtime, weight_dtype_kw
        try:
            runtime = load_runtime(model_name_or_path, device, cache_dir=cache_dir, **weight_dtype_kw(weight_dtype), **kv_dtype_kw(self.kv_dtype))
        except NotImplementedError as exc:   # same message shape as ref: setwise.py:71
            raise NotImplementedError(f"{exc} (setwise)") from None
        if runtime.model_type == "llama":
            from transformers import AutoTokenizer
            tokenizer = AutoTokenizer.from_pretrained(model_name_or_path, cache_dir=cache_dir)   # (the reference ignores tokenizer_name_or_path here)
            tokenizer.use_default_system_prompt = False
            if 'v1.5' in model_name_or_path:       # the reference's `'vicuna' and 'v1.5' in name` (ref :63)
                tokenizer.chat_template = VICUNA_TEMPLATE
        else:
            from transformers import T5Tokenizer
            tokenizer = T5Tokenizer.from_pretrained(
                tokenizer_name_or_path if tokenizer_name_or_path is not None else model_name_or_path, cache_dir=cache_dir)
        self._setup(runtime, tokenizer, device, num_child, k, scoring, method, num_permutation)

    @classmethod
    def from_runtime(cls, runtime, tokenizer, device="cuda", num_child=3, k=10, scoring='generation', method="heapsort",
                     num_permutation=1):
        """Build the ranker around an existing runtime (a loaded engine, or a test double) and tokenizer."""
        self = cls.__new__(cls)
        self._setup(runtime, tokenizer, device, num_child, k, scoring, method, num_permutation)
        return self

    def _setup(self, runtime, tokenizer, device, num_child, k, scoring, method, num_permutation):
        from ._runtime import require_decoder_positions
        require_decoder_positions(runtime, type(self).__name__)
        self.device = device
        self.num_child = num_child
        self.num_permutation = num_permutation
        self.k = k
        self.llm = runtime
        self.config = getattr(runtime, "config", None)
        self.tokenizer = tokenizer
        self.model_type = getattr(runtime, "model_type", "t5")
        if self.model_type == "t5":
            # decoder prompt "<pad> Passage" and the last token of "<pad> Passage {label}" (ref: setwise.py:51-59)
            self.decoder_input_ids = self.tokenizer.encode("<pad> Passage", add_special_tokens=False)
            self.target_token_ids = [self.tokenizer.encode(f"<pad> Passage {c}", add_special_tokens=False)[-1]
                                     for c in self.CHARACTERS]
        self.scoring = scoring
        self.method = method
        # heapsort build phase: advance the independent sift-downs of a tree level in one engine call each (same
        # result, compares and counters as the reference's one-by-one order; 9 of the 29 compares at hits=100, c=10)
        self.batch_independent_compares = True
        self.total_compare = 0
        self.total_completion_tokens = 0
        self.total_prompt_tokens = 0

    # ------------------------------------------------------------------------------------------------------
    def _prompt(self, query: str, labels: List[str], texts: List[str]) -> str:
        passages = "\n\n".join(f'Passage {lab}: "{txt}"' for lab, txt in zip(labels, texts))
        return QUESTION.format(query=query) + passages + INSTRUCTION

    def _generate(self, token_lists: List[List[int]]) -> List[List[int]]:
        """Greedy, max_new_tokens=2, continuing "<pad> Passage".  Returns full output id rows the way
        HF generate does: prefix + new tokens, all rows cut at the step where every row had finished."""
        eos, pad = self.tokenizer.eos_token_id, self.tokenizer.pad_token_id
        if getattr(self.llm, "supports_greedy_candidates", False):
            # hint: the first new token is normally a passage label -> both steps in one decoder pass (rk_t5_greedy2)
            new = self.llm.greedy(token_lists, self.decoder_input_ids, 2, eos, pad,
                                  candidates=self.target_token_ids[:self.num_child + 1])
        else:
            new = self.llm.greedy(token_lists, self.decoder_input_ids, 2, eos, pad)
        out = []
        for row in np.asarray(new):
            out.append(list(self.decoder_input_ids) + [int(t) for t in row if t >= 0])
        return out

    def compare(self, query: str, docs: List):
        # ref: setwise.py:79-198
        self.total_compare += 1 if self.num_permutation == 1 else self.num_permutation
        if self.model_type != "llama" and self.scoring == 'generation' and self.num_permutation > 1:
            return self._compare_permuted(query, docs)
        # one window of `_compare_windows` (a Llama model ignores num_permutation: it only entered total_compare above)
        (output,), (ptok,), (ctok,) = self._compare_windows([query], [docs])
        self.total_prompt_tokens += ptok
        self.total_completion_tokens += ctok
        return output

    def _compare_permuted(self, query: str, docs: List):
        """T5 `generation` with num_permutation > 1 (ref: setwise.py:100-150): every permutation's prompt in one call, then the vote"""
        id_passage = [(i, p) for i, p in enumerate(docs)]
        labels = [self.CHARACTERS[i] for i in range(len(docs))]
        perms = []
        for _ in range(self.num_permutation):   # two draws per permutation, in this order (ref :107-109)
            perms.append([random.sample(id_passage, len(id_passage)), random.sample(labels, len(labels))])
        refs, texts = [], []
        for shuffled, chars in perms:
            refs.append(([p[0] for p in shuffled], list(chars)))
            texts.append(self._prompt(query, list(chars), [p[1].text for p in shuffled]))
        ids = tokenize_prompts(self.tokenizer, texts)
        # return_tensors="pt" without padding requires equal lengths; permuting passages keeps them equal
        self.total_prompt_tokens += len(ids[0]) * len(ids)
        rows = self._generate(ids)
        plen = len(self.decoder_input_ids)
        decoded = self.tokenizer.batch_decode([r[plen:] for r in rows], skip_special_tokens=True)
        output = vote(refs, [result.strip().upper() for result in decoded], self.CHARACTERS, print)
        if output not in self.CHARACTERS:
            print(f"Unexpected voting: {decoded}")
            print(f"Unexpected output: {output}")
        return output

    def _llama_prompt_ids(self, input_text: str) -> List[int]:
        """chat template + " Passage:" -> token ids, as ref: setwise.py:160-165 builds them"""
        prompt = self.tokenizer.apply_chat_template([{"role": "user", "content": input_text}], tokenize=False, add_generation_prompt=True)
        return list(self.tokenizer(prompt + " Passage:")["input_ids"])

    def _compare_many(self, query: str, doc_lists: List[List]) -> List[str]:
        """Independent compares in ONE engine call.  Same outputs and counters as `compare()` on each window in turn
        (num_permutation == 1 only: no random draws are involved); the engine's results do not depend on which
        prompts share a call (ragged execution, bit-exact batch independence)."""
        outs, prompt_tokens, completion_tokens = self._compare_windows([query] * len(doc_lists), doc_lists)
        self.total_compare += len(doc_lists)
        self.total_prompt_tokens += sum(prompt_tokens)
        self.total_completion_tokens += sum(completion_tokens)
        return outs

    def _compare_windows(self, queries: List[str], doc_lists: List[List]):
        """The engine call behind `compare` and `_compare_many`, for windows that may belong to different queries (`rerank_many`):
        -> (labels, prompt tokens per window, completion tokens per window); touches no counter and draws no random number."""
        if self.model_type == "llama" and self.scoring == 'likelihood':
            raise NotImplementedError                           # ref: setwise.py:175-176, before any token is counted
        if self.scoring not in ('generation', 'likelihood'):
            raise UnboundLocalError("local variable 'output' referenced before assignment")  # what the reference does
        texts = [self._prompt(q, self.CHARACTERS[:len(docs)], [d.text for d in docs]) for q, docs in zip(queries, doc_lists)]
        if self.model_type == "llama":
            # ref: setwise.py:159-177 — prefill and one greedy token; generate() returns prompt + new token for a decoder-only model
            ids = [self._llama_prompt_ids(t) for t in texts]
            toks = self.llm.greedy1(ids)
            outs = [self.tokenizer.decode([int(tok)], skip_special_tokens=True).strip().upper() for tok in toks]
            prompt_tokens, completion_tokens = [len(seq) for seq in ids], [len(seq) + 1 for seq in ids]
        elif self.scoring == 'generation':
            ids = tokenize_prompts(self.tokenizer, texts)
            prompt_tokens, completion_tokens = [len(i) for i in ids], []
            outs, eos = [], self.tokenizer.eos_token_id
            for row in self._generate(ids):
                new = row[len(self.decoder_input_ids):]
                if eos in new:                                  # alone, this row would have stopped at its own EOS
                    new = new[:new.index(eos) + 1]
                row = list(self.decoder_input_ids) + new
                completion_tokens.append(len(row))
                outs.append(self.tokenizer.decode(row, skip_special_tokens=True).strip()[-1])
        else:
            # softmax over the vocabulary is monotone, so the best label is the arg-max of the label logits;
            # stable descending sort = first maximum wins (ref: setwise.py:184-188)
            if any(len(docs) == 0 for docs in doc_lists):
                raise IndexError("list index out of range")     # ranked[0] on an empty list in the reference (:188)
            ids = tokenize_prompts(self.tokenizer, texts)
            prompt_tokens, completion_tokens = [len(i) for i in ids], [0] * len(ids)
            nmax = max(len(docs) for docs in doc_lists)
            lg = np.asarray(self.llm.score(ids, self.decoder_input_ids, self.target_token_ids[:nmax]))
            outs = [self.CHARACTERS[int(np.argmax(lg[r, :len(docs)]))] for r, docs in enumerate(doc_lists)]
        for output in outs:
            if not (len(output) == 1 and output in self.CHARACTERS):
                print(f"Unexpected output: {output}")
        return outs, prompt_tokens, completion_tokens

    # ---- the same compare, launched and collected separately (likelihood scoring on a runtime with batch slots) ----------
    def _can_alternate(self) -> bool:
        """Two groups of lockstep queries can alternate over the engine's batch slots: T5 likelihood scoring (one engine call
        per step, no host decision inside it) on a runtime that launches without waiting (T5Runtime.score_async)."""
        return (self.model_type != "llama" and self.scoring == "likelihood" and getattr(self, "alternate_groups", True)
                and hasattr(self.llm, "score_async") and getattr(getattr(self.llm, "engine", None), "num_slots", 1) >= 2)

    def _launch_windows(self, queries: List[str], doc_lists: List[List], slot: int):
        """First half of `_compare_windows` (likelihood): prompts, tokens, ONE engine call enqueued on `slot`; returns at once.
        None when the windows do not fit one engine call (the caller then takes the blocking call for this round)."""
        if any(len(docs) == 0 for docs in doc_lists):
            raise IndexError("list index out of range")
        texts = [self._prompt(q, self.CHARACTERS[:len(docs)], [d.text for d in docs]) for q, docs in zip(queries, doc_lists)]
        ids = tokenize_prompts(self.tokenizer, texts)
        nmax = max(len(docs) for docs in doc_lists)
        handle = self.llm.score_async(ids, self.decoder_input_ids, self.target_token_ids[:nmax], slot)
        if handle is None:
            return None
        return handle, [len(docs) for docs in doc_lists], [len(i) for i in ids]

    def _collect_windows(self, launched):
        """Second half: waits for the slot, -> (labels, prompt tokens per window, completion tokens per window)."""
        handle, sizes, prompt_tokens = launched
        lg = np.asarray(self.llm.score_collect(handle))
        outs = [self.CHARACTERS[int(np.argmax(lg[r, :n]))] for r, n in enumerate(sizes)]
        return outs, prompt_tokens, [0] * len(sizes)

    def _batched_ok(self) -> bool:
        # level-wise batching needs compare() to be ours (no subclass / instance override) and draw-free
        return (getattr(self, "batch_independent_compares", False) and self.num_permutation == 1
                and "compare" not in self.__dict__ and type(self).compare is SetwiseLlmRanker.compare)

    # ---- the sorts: pure index logic, must reproduce the reference's comparisons exactly -------------------------
    # Each is a generator that yields a list of windows whose compares are independent of each other and is sent their labels.
    def _pick(self, output: str) -> int:
        try:
            return self.CHARACTERS.index(output)
        except ValueError:
            return 0                              # malformed output -> first document wins (ref :206-209)

    def _sift(self, arr, n, i):
        """Sift node i of the c-ary max-heap arr[:n] down (ref: setwise.py:200-217, a loop instead of tail recursion): one
        window, the parent and its children, per step."""
        c = self.num_child
        while True:
            first = c * i + 1                                  # node i's children are first .. first + c - 1
            if first >= n:
                return
            inds = [i] + list(range(first, min(first + c, n)))
            (label,) = yield [[arr[j] for j in inds]]
            best = self._pick(label)
            largest = inds[best] if best < len(inds) else i   # label beyond the window keeps the parent (ref :210-213)
            if largest == i:
                return
            arr[i], arr[largest] = arr[largest], arr[i]
            i = largest

    def _bubblesort_steps(self, ranking):
        # ref: setwise.py:243-273 — sliding window of num_child+1 bubbling the best document to position i,
        # with the reference's `last_start` shortcut that skips windows already known to be in order.
        c = self.num_child
        full = len(ranking) - (c + 1)
        last_start = full
        for i in range(self.k):
            start, end = last_start, last_start + (c + 1)
            changed = False
            while True:
                if start < i:
                    start = i
                window = ranking[start:end]
                (label,) = yield [window]
                best = self._pick(label)
                if best != 0:
                    # no guard here in the reference either: an out-of-window label raises IndexError
                    ranking[start], ranking[start + best] = ranking[start + best], ranking[start]
                    if not changed:
                        changed = True
                        if last_start != full and best == len(window) - 1:
                            last_start += len(window) - 1
                if start == i:
                    break
                if not changed:
                    last_start -= c
                start -= c
                end -= c

    def _sort_steps(self, ranking, level_batched):
        if self.method == "heapsort":
            return heapsort_steps(ranking, self.k, self.num_child, self._sift, level_batched)      # ref: setwise.py:219-232
        if self.method == "bubblesort":
            return self._bubblesort_steps(ranking)
        raise NotImplementedError(f'Method {self.method} is not implemented.')

    def _answer(self, query, level_batched):
        """How the windows of one query's sort are answered.  Reference order: every window through `compare`, one at a time
        (looked up on the instance: tests, golden generators and subclasses replace it); level order: every yielded list is one
        `_compare_many`."""
        if level_batched:
            return lambda windows: self._compare_many(query, windows)
        return lambda windows: [self.compare(query, w) for w in windows]

    def heapify(self, arr, n, i, query):
        # ref: setwise.py:200-217, always one compare at a time
        drive(self._sift(arr, n, i), self._answer(query, False))

    def heapSort(self, arr, query, k):
        # ref: setwise.py:219-232
        level_batched = self._batched_ok()
        drive(heapsort_steps(arr, k, self.num_child, self._sift, level_batched), self._answer(query, level_batched))

    def rerank(self, query: str, ranking: List[SearchResult]) -> List[SearchResult]:
        # ref: setwise.py:234-313.  NB: like the reference, the caller's list is re-ordered in place.
        original_docids = [doc.docid for doc in ranking]     # (the reference deep-copies the whole list: 3 ms for 100 passages; only the docid order is read)
        self.total_compare = 0
        self.total_completion_tokens = 0
        self.total_prompt_tokens = 0
        level_batched = self.method == "heapsort" and self._batched_ok()
        drive(self._sort_steps(ranking, level_batched), self._answer(query, level_batched))
        return top_k_then_rest(list(reversed(ranking)) if self.method == "heapsort" else ranking, original_docids, self.k)

    # ---- several queries at once ---------------------------------------------------------------------------
    def rerank_many(self, items):
        """Several queries at once: `items` = [(query, ranking), ...] -> (results, counters); results[i] and counters[i] =
        (total_compare, total_prompt_tokens, total_completion_tokens) are exactly what `rerank(*items[i])` gives, and the
        callers' lists end up re-ordered the same way.  The compares of ONE query are a dependency chain (each sift-down step
        needs the previous label), but the chains of different queries are independent: their pending compares go to the
        engine together, one call per step of all the chains - several ~900-token prompts per launch sequence instead of one
        (a compare's result does not depend on what shares its engine call: ragged execution, bit-exact).
        heapsort and bubblesort with the draw-free default settings; anything else (permutation voting, a compare() of a
        subclass - Rank-R1's has a rerank_many of its own) is one rerank per query."""
        items = list(items)
        if self.method not in ("heapsort", "bubblesort") or not self._batched_ok() or len(items) < 2:
            return rerank_each(self, items)
        originals = [[doc.docid for doc in ranking] for _, ranking in items]
        counts = [[0, 0, 0] for _ in items]
        chains = Lockstep({q: self._sort_steps(ranking, True) for q, (_, ranking) in enumerate(items)})

        def queries_of(keys):
            return [items[q][0] for q in keys]

        def blocking(keys, windows):
            return tally(counts, keys, *self._compare_windows(queries_of(keys), windows))

        if len(chains.live()) >= 4 and self._can_alternate():
            # Two groups of chains alternate over the engine's two batch slots: while one group's call is on the GPU the host
            # advances the other group's heaps, builds and tokenises its prompts and launches them - the launch-bound decoder
            # chain of one call runs under the encoder of the next, and the host part of a step is hidden.  A chain sees the
            # same labels as alone (batch independence), so rankings and counters do not change (tests).  A round that does
            # not fit one engine call takes the blocking call, which cuts it; the next round is launched again.
            alternate(chains, lambda keys, windows, slot: self._launch_windows(queries_of(keys), windows, slot=slot),
                      lambda keys, launched: tally(counts, keys, *self._collect_windows(launched)), blocking)
        while chains:
            chains.advance(blocking(*chains.pending()))
        heap = self.method == "heapsort"
        results = [top_k_then_rest(list(reversed(ranking)) if heap else ranking, original, self.k)
                   for (_, ranking), original in zip(items, originals)]
        return results, close_counters(self, counts)

    def truncate(self, text, length):
        return self.tokenizer.convert_tokens_to_string(self.tokenizer.tokenize(text)[:length])


def load_prompt_file(prompt_file):
    """The Rank-R1 prompt settings (prompt_system, prompt_user, pattern): a mapping as it is, or a TOML file (ref:
    llmrankers/setwise.py:426-427 reads it with `toml`) through whichever TOML reader is installed."""
    if isinstance(prompt_file, dict) or hasattr(prompt_file, "keys"):
        prompt = dict(prompt_file)
    else:
        reader = None
        for name in ("tomllib", "tomli", "toml"):
            try:
                reader = __import__(name)
                break
            except ImportError:
                continue
        if reader is None:
            raise ImportError("reading a Rank-R1 prompt file needs a TOML reader (Python >= 3.11's tomllib, or the tomli or toml "
                              "package); alternatively pass the parsed mapping as prompt_file")
        if reader.__name__ == "toml":
            prompt = dict(reader.load(prompt_file))
        else:
            with open(prompt_file, "rb") as f:
                prompt = dict(reader.load(f))
    missing = [k for k in ("prompt_system", "prompt_user", "pattern") if k not in prompt]
    if missing:
        raise KeyError(f"prompt file lacks {missing}")
    return prompt


_WEIGHT_DTYPE_CLASSES = {}      # (class, weight_dtype) -> the subclass with_weight_dtype hands out


class RankR1SetwiseLlmRanker(SetwiseLlmRanker):
    """Rank-R1, the reasoning setwise reranker (ref: llmrankers/setwise.py:406-553; Qwen2.5-Instruct + a LoRA adapter served by
    vLLM there): one compare = a chat prompt listing the passages as "[n] text", a generated chain of thought of up to
    max_new_tokens tokens, and a regular expression that takes the answer's "[n]" label out of it.  Here the checkpoint (the
    adapter merged on the host, _runtime.merge_lora) runs on the engine's KV-cached greedy decoder (rk_llama_generate; several
    queries at once: rerank_many over a decoding session, rk_llama_session_*).  Same
    constructor, compare() contract, counters, vote and sort drivers as the reference; stand-ins for vLLM ("Qwen2 family and Rank-R1"):
    the stop ids are the checkpoint's generation settings, the EOS that ended a row counts as a completion token, the completion
    text is the new tokens decoded without special tokens."""
    CHARACTERS = [f'[{i + 1}]' for i in range(20)]

    # FP8 step weights (LlamaRuntime's weight_dtype; lossy, opt-in).  The constructor keeps the reference's parameter list, so the
    # option is the class's: RankR1SetwiseLlmRanker.with_weight_dtype("fp8")(model, prompt_file, ...)
    weight_dtype = "fp16"

    @classmethod
    def with_weight_dtype(cls, weight_dtype):
        from ._runtime import weight_dtype_kw
        weight_dtype_kw(weight_dtype)                                  # ValueError for anything but "fp16" / "fp8"
        if weight_dtype == cls.weight_dtype:
            return cls
        made = _WEIGHT_DTYPE_CLASSES
        if (cls, weight_dtype) not in made:                            # one subclass per (class, dtype), not one per call
            made[cls, weight_dtype] = type(cls.__name__, (cls,), {"weight_dtype": weight_dtype})
        return made[cls, weight_dtype]

    # Drafting by prompt lookup (LlamaRuntime.open_pool's draft_tokens; lossless, opt-in: the same tokens in fewer steps).  Like
    # weight_dtype the option is the class's: RankR1SetwiseLlmRanker.with_draft_tokens(3)(model, prompt_file, ...).  With it on,
    # compare() decodes its prompts through a pool of one slot per prompt instead of rk_llama_generate.
    draft_tokens = 0

    @classmethod
    def with_draft_tokens(cls, draft_tokens):
        from ._runtime import draft_tokens_kw
        draft_tokens_kw(draft_tokens)                                  # ValueError outside 0..7
        if int(draft_tokens) == cls.draft_tokens:
            return cls
        made = _WEIGHT_DTYPE_CLASSES
        if (cls, "draft_tokens", int(draft_tokens)) not in made:
            made[cls, "draft_tokens", int(draft_tokens)] = type(cls.__name__, (cls,), {"draft_tokens": int(draft_tokens)})
        return made[cls, "draft_tokens", int(draft_tokens)]

    def __init__(self, model_name_or_path, prompt_file, lora_name_or_path=None, tokenizer_name_or_path=None, num_child=19, k=10,
                 scoring='generation', method="heapsort", num_permutation=1, cache_dir=None, verbose=False, device="cuda",
                 max_new_tokens=2048):
        if scoring != 'generation':
            raise NotImplementedError(f"Scoring method {scoring} is not supported for RankR1SetwiseLlmRanker. RankR1SetwiseLlmRanker only supports 'generation' scoring.")
        from transformers import AutoTokenizer
        from ._runtime import LlamaRuntime, kv_dtype_kw, resolve_checkpoint, weight_dtype_kw
        prompt = load_prompt_file(prompt_file)
        lora_path = resolve_checkpoint(lora_name_or_path, cache_dir) if lora_name_or_path is not None else None
        tokenizer = AutoTokenizer.from_pretrained(tokenizer_name_or_path if tokenizer_name_or_path is not None else model_name_or_path,
                                                  cache_dir=cache_dir)
        runtime = LlamaRuntime(model_name_or_path, device, cache_dir=cache_dir, accept_model_types=("qwen2", "llama", "mistral", "qwen3"),
                               adapter_dir=lora_path, **weight_dtype_kw(self.weight_dtype), **kv_dtype_kw(self.kv_dtype))
        self._setup_r1(runtime, tokenizer, prompt, lora_path, device, num_child, k, method, num_permutation, verbose, max_new_tokens)

    @classmethod
    def from_runtime(cls, runtime, tokenizer, prompt_file, device="cuda", num_child=19, k=10, scoring='generation', method="heapsort",
                     num_permutation=1, verbose=False, max_new_tokens=2048):
        """Build the ranker around an existing runtime (a loaded engine - adapter already merged - or a test double)."""
        if scoring != 'generation':
            raise NotImplementedError(f"Scoring method {scoring} is not supported for RankR1SetwiseLlmRanker. RankR1SetwiseLlmRanker only supports 'generation' scoring.")
        self = cls.__new__(cls)
        self._setup_r1(runtime, tokenizer, load_prompt_file(prompt_file), None, device, num_child, k, method, num_permutation, verbose,
                       max_new_tokens)
        return self

    def _setup_r1(self, runtime, tokenizer, prompt, lora_path, device, num_child, k, method, num_permutation, verbose, max_new_tokens):
        self.verbose = verbose
        self.prompt = prompt
        self.lora_path = lora_path
        self.device = device
        self.num_child = num_child
        self.num_permutation = num_permutation
        self.k = k
        self.max_new_tokens = int(max_new_tokens)          # the reference's SamplingParams(temperature=0.0, max_tokens=2048)
        self.tokenizer = tokenizer
        self.llm = runtime
        self.config = getattr(runtime, "config", None)
        self.model_type = getattr(runtime, "model_type", "qwen2")
        self.scoring = 'generation'
        self.method = method
        self.batch_independent_compares = False           # compare() draws from `random`: the one-by-one order is the contract
        self.total_compare = 0
        self.total_completion_tokens = 0
        self.total_prompt_tokens = 0

    compare_rng = None    # the generator compare() draws from; None: the module-level `random`, the reference's one global stream

    def compare(self, query: str, docs: List):
        # ref: setwise.py:462-553, in three parts: the prompts (draws), ONE engine call, the verdict (draws on a tie)
        rng = self.compare_rng if self.compare_rng is not None else random
        self.total_compare += 1 if self.num_permutation == 1 else self.num_permutation
        batch_ref, input_text, ids = self._compare_prompts(query, docs, rng)
        gen = self.llm.generation
        if self.draft_tokens and hasattr(self.llm, "open_pool"):           # the same tokens through a drafting pool, one slot per prompt
            from ._runtime import generate_drafted
            rows = generate_drafted(self.llm, ids, self.max_new_tokens, list(gen["eos_token_ids"]), int(gen["pad_token_id"]), self.draft_tokens)
        else:
            rows = np.asarray(self.llm.generate(ids, self.max_new_tokens, list(gen["eos_token_ids"]), int(gen["pad_token_id"])))   # ONE engine call
        output, prompt_tokens, completion_tokens = self._compare_verdict(query, batch_ref, input_text, ids, rows, rng)
        self.total_prompt_tokens += prompt_tokens
        self.total_completion_tokens += completion_tokens
        return output

    def _compare_prompts(self, query: str, docs: List, rng):
        """-> (batch_ref, messages, prompt ids) of the window's num_permutation prompts"""
        id_passage = [(i, p) for i, p in enumerate(docs)]
        labels = [self.CHARACTERS[i] for i in range(len(docs))]
        batch_ref, input_text = [], []
        for _ in range(self.num_permutation):               # one draw per permutation (also for a single one); labels stay in order
            shuffled = rng.sample(id_passage, len(id_passage))
            batch_ref.append(([p[0] for p in shuffled], list(labels)))
            passages = "\n".join(f'{c} {p[1].text}' for p, c in zip(shuffled, labels))
            input_text.append([{'role': "system", 'content': self.prompt["prompt_system"]},
                               {'role': "user", 'content': self.prompt['prompt_user'].format(query=query, docs=passages)}])
        return batch_ref, input_text, [self._chat_ids(messages) for messages in input_text]

    def _compare_verdict(self, query: str, batch_ref, input_text, ids, rows, rng):
        """rows[p] = the new tokens of prompt p (columns < 0 and whatever follows the EOS that ended the row are not part of it)
        -> (label, prompt tokens, completion tokens): the regular expression, then the vote"""
        import re
        eos_ids = list(self.llm.generation["eos_token_ids"])
        prompt_tokens = completion_tokens = 0
        results = []
        for prompt_ids, row, messages in zip(ids, rows, input_text):
            new = [int(t) for t in row if t >= 0]
            stop = next((i for i, t in enumerate(new) if t in eos_ids), None)
            if stop is not None:                             # vLLM's token_ids keep the EOS that ended the row
                new = new[:stop + 1]
            completion_tokens += len(new)
            prompt_tokens += len(prompt_ids)
            completion = self.tokenizer.decode(new, skip_special_tokens=True)
            if self.verbose:
                print('--------------------------------------')
                print(f'query: {query}')
                print(f'input_text:\n{self.tokenizer.apply_chat_template(messages, tokenize=False)}')
                print(f'completion:\n{completion}')
                print('--------------------------------------')
            match = re.search(rf'{self.prompt["pattern"]}', completion.lower(), re.DOTALL)
            results.append(match.group(1).strip() if match else f'input_text:\n{messages}, completion:\n{completion}')
        say = print if self.verbose else (lambda *_: None)
        output = vote(batch_ref, [result.strip() for result in results], self.CHARACTERS, say, rng)
        if output not in self.CHARACTERS:
            say(f"Unexpected voting: {results}")
            say(f"Unexpected output: {output}")
        return output, prompt_tokens, completion_tokens

    def rerank_many(self, items):
        """Several queries at once over the runtime's decoding pool (LlamaRuntime.open_pool: continuous batching, what vLLM gives
        the reference): every query is a chain of its own - its pending window's num_permutation prompts are submitted, the window
        is answered (regular expression, then the vote, as in compare) when all its completions have returned, and that chain alone
        advances and submits its next window.  No lock step: chains of thought end at any length, and a finished row's slot goes to
        whichever chain is waiting.
        Randomness: compare draws (one `sample` per permutation, one `choice` per tied vote), and interleaved queries cannot share
        one stream reproducibly.  Query i gets its own random.Random(seed_i), seed_i = random.getrandbits(64) drawn from the
        module-level stream in item order at the start of the call - a documented deviation from the reference's one global stream
        (DESIGN.md section 4).  results[i], counters[i] and the caller's re-ordered list equal `rerank(*items[i])` run with that
        generator as `compare_rng`.  One query, or a runtime without a pool: one `rerank` per query on the module-level stream."""
        items = list(items)
        if (len(items) < 2 or not hasattr(self.llm, "open_pool") or self.method not in ("heapsort", "bubblesort")
                or "compare" in self.__dict__):             # (a compare replaced on the instance is the caller's: one at a time)
            return super().rerank_many(items)
        rngs = [random.Random(seed) for seed in [random.getrandbits(64) for _ in items]]
        originals = [[doc.docid for doc in ranking] for _, ranking in items]
        counts = [[0, 0, 0] for _ in items]
        chains = [Lockstep({0: self._sort_steps(ranking, False)}) for _, ranking in items]
        waiting = {}                                         # query -> its pending window: prompts, references, rows so far
        gen = self.llm.generation

        def submit(pool, q):
            (docs,) = chains[q].pending()[1]
            counts[q][0] += 1 if self.num_permutation == 1 else self.num_permutation
            batch_ref, input_text, ids = self._compare_prompts(items[q][0], docs, rngs[q])
            waiting[q] = (batch_ref, input_text, ids, {})
            for p, prompt in enumerate(ids):
                pool.submit((q, p), prompt, self.max_new_tokens)

        from ._runtime import draft_tokens_kw
        with self.llm.open_pool(max_new_cap=self.max_new_tokens, eos_ids=list(gen["eos_token_ids"]), pad_id=int(gen["pad_token_id"]),
                                **draft_tokens_kw(self.draft_tokens)) as pool:
            for q in range(len(items)):
                if chains[q]:
                    submit(pool, q)
            while waiting:
                for (q, p), tokens in pool.wait():
                    batch_ref, input_text, ids, rows = waiting[q]
                    rows[p] = tokens
                    if len(rows) < len(ids):
                        continue
                    del waiting[q]
                    label, prompt_tokens, completion_tokens = self._compare_verdict(items[q][0], batch_ref, input_text, ids,
                                                                                    [rows[i] for i in range(len(ids))], rngs[q])
                    counts[q][1] += prompt_tokens
                    counts[q][2] += completion_tokens
                    chains[q].advance([label])
                    if chains[q]:
                        submit(pool, q)
        heap = self.method == "heapsort"
        results = [top_k_then_rest(list(reversed(ranking)) if heap else ranking, original, self.k)
                   for (_, ranking), original in zip(items, originals)]
        return results, close_counters(self, counts)

    def _chat_ids(self, messages) -> List[int]:
        """what vLLM's LLM.chat feeds the model: the chat template with the generation prompt, tokenized"""
        out = self.tokenizer.apply_chat_template(messages, add_generation_prompt=True, tokenize=True)
        if hasattr(out, "keys"):                             # transformers >= 5 returns a BatchEncoding
            out = out["input_ids"]
        return [int(t) for t in out]

    def _compare_windows(self, queries, doc_lists):
        raise NotImplementedError("RankR1SetwiseLlmRanker compares one window at a time")
