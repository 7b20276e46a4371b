"""Listwise ranker on the MI355X engine: RankGPT-style sliding windows over a "rank these passages" call.

Drop-in for ref: llmrankers/listwise.py:202-291 (ListwiseLlmRanker) on T5 and Llama checkpoints - same constructor, `compare()`
contract, counters, window walk and permutation rules.  Each compare is one encoder pass over the window's prompt plus either
a greedy continuation of up to 20 tokens read as a permutation (`scoring='generation'`, engine call rk_t5_generate: one decoder
row per sequence and step against a K / V cache) or one label-row read at decoder position 1 ordering the passages by their
label logits (`scoring='likelihood'`, rk_t5_score with the window's label ids).
On a Llama checkpoint (ref: listwise.py:235-245, 261-271) a compare is the chat-template prompt (system message, one user /
assistant pair per passage, the closing instruction) continued greedily by rk_llama_generate - the prefill once, then one
KV-cached decoder row per new token - with the length, EOS ids and pad id of the checkpoint's generation settings; `likelihood`
fails there as it does in the reference.
"""
import copy
from typing import List, Optional

import numpy as np

from ._batching import tokenize_prompts
from ._lockstep import Lockstep, drive
from .rankers import KvDtypeOption, LlmRanker, SearchResult, close_counters, tally

# the "complete" prompt of the reference (ref: listwise.py:85-104) - model input, byte for byte
HEAD = ("This is RankGPT, an intelligent assistant that can rank passages based on their relevancy to the query.\n\n"
        "The following are {num} passages, each indicated by number identifier []. "
        "I can rank them based on their relevance to query: {query}\n\n")
ENTRY = "[{rank}] {content}\n\n"
TAIL = ("The search query is: {query}"
        "I will rank the {num} passages above based on their relevance to the search query. The passages "
        "will be listed in descending order using identifiers, and the most relevant passages should be listed "
        "first, and the output format should be [] > [] > etc, e.g., [1] > [2] > etc.\n\n"
        "The ranking results of the {num} passages (only identifiers) is:")
MAX_WORDS = 300                                   # words kept per passage (ref: listwise.py:97)
# the setwise-style prompt of `likelihood` scoring (ref: listwise.py:265-267)
QUESTION = 'Given a query "{query}", which of the following passages is the most relevant one to the query?\n\n'
INSTRUCTION = '\n\nOutput only the passage label of the most relevant passage:'

LLAMA_MESSAGE = "listwise on a Llama checkpoint needs a runtime with the incremental (KV-cached) decoder: `generate` is missing"
# the chat prompt of the Llama branch (ref: listwise.py:17-26, 63-88 with model_name=None: no length loop) - model input, as is
CHAT_SYSTEM = "You are RankGPT, an intelligent assistant that can rank passages based on their relevancy to the query."
CHAT_OPEN = "I will provide you with {num} passages, each indicated by number identifier []. \nRank the passages based on their relevance to query: {query}."
CHAT_OPEN_REPLY = "Okay, please provide the passages."
CHAT_POST = ("Search Query: {query}. \nRank the {num} passages above based on their relevance to the search query. The passages should be "
             "listed in descending order using identifiers. The most relevant passages should be listed first. The output format should "
             "be [] > [], e.g., [1] > [2]. Only response the ranking results, do not say any word or explain.")


def resolve_max_new(model_dir: Optional[str] = None) -> int:
    """New tokens of the reference's bare `llm.generate(input_ids)` (ref: listwise.py:248) for an encoder-decoder checkpoint: the
    checkpoint's generation_config.json when it sets a length, otherwise the installed transformers' default (>= 5: 20 new
    tokens; before: max_length 20 counting the decoder start token)."""
    import json
    import os
    if model_dir and os.path.exists(os.path.join(model_dir, "generation_config.json")):
        with open(os.path.join(model_dir, "generation_config.json")) as f:
            gc = json.load(f)
        if gc.get("max_new_tokens") is not None:
            return int(gc["max_new_tokens"])
        if gc.get("max_length") is not None:
            return int(gc["max_length"]) - 1
    try:
        from transformers import GenerationConfig
        ml = GenerationConfig().max_length
    except Exception:                      # (no transformers: the current default)
        ml = None
    return 20 if ml is None else int(ml) - 1


def permutation_order(response: str, n: int) -> List[int]:
    """The window order a generated permutation asks for (ref: listwise.py:118-148): the digit runs of the text are 1-based ids;
    repeats after the first and ids outside 1..n are dropped; ids never named follow in their current order."""
    seen, order = set(), []
    for word in "".join(c if c.isdigit() else " " for c in response).split():
        k = int(word) - 1
        if 0 <= k < n and k not in seen:
            seen.add(k)
            order.append(k)
    return order + [k for k in range(n) if k not in seen]


class ListwiseLlmRanker(KvDtypeOption, LlmRanker):
    # "Passage X" / "Passage Y" tokenize into 3 tokens with the T5 vocabulary, hence 23 labels (ref: listwise.py:203-205)
    CHARACTERS = ["A", "B", "C", "D", "E", "F", "G", "H", "I", "J", "K", "L",
                  "M", "N", "O", "P", "Q", "R", "S", "T", "U", "V", "W"]

    def __init__(self, model_name_or_path, tokenizer_name_or_path, device, window_size, step_size,
                 scoring='generation', num_repeat=1, cache_dir=None, sample_seed=None, weight_dtype="fp16"):
        # ref: listwise.py:207-247: T5 or Llama by config.model_type, NotImplementedError otherwise
        # sample_seed (decoder-only checkpoints; not in the reference, whose sampling follows torch's global generator): None =
        # greedy decoding whatever the checkpoint's generation settings say; an integer = a checkpoint that says do_sample: true
        # is sampled on the device with its own temperature / top_k / top_p, reproducibly (see _setup)
        # weight_dtype (not in the reference): "fp8" = FP8 step weights on a Llama-family checkpoint (LlamaRuntime; lossy, opt-in)
        from ._runtime import kv_dtype_kw, load_runtime, resolve_checkpoint, weight_dtype_kw
        path = resolve_checkpoint(model_name_or_path, cache_dir)
        try:
            runtime = load_runtime(path, device, cache_dir=cache_dir, **weight_dtype_kw(weight_dtype), **kv_dtype_kw(self.kv_dtype))
        except NotImplementedError as exc:   # same message shape as ref: listwise.py:247
            raise NotImplementedError(f"{exc} (listwise)") from None
        if runtime.model_type == "llama":
            from transformers import AutoTokenizer
            from .setwise import VICUNA_TEMPLATE
            tokenizer = AutoTokenizer.from_pretrained(model_name_or_path, cache_dir=cache_dir)   # (the reference ignores tokenizer_name_or_path here)
            tokenizer.use_default_system_prompt = False
            if 'v1.5' in model_name_or_path:       # the reference's `'vicuna' and 'v1.5' in name` (ref :238)
                tokenizer.chat_template = VICUNA_TEMPLATE
            self._setup(runtime, tokenizer, device, window_size, step_size, scoring, num_repeat, None, sample_seed)
            return
        from transformers import T5Tokenizer
        tokenizer = T5Tokenizer.from_pretrained(
            tokenizer_name_or_path if tokenizer_name_or_path is not None else model_name_or_path, cache_dir=cache_dir)
        self._setup(runtime, tokenizer, device, window_size, step_size, scoring, num_repeat, resolve_max_new(path))

    @classmethod
    def from_runtime(cls, runtime, tokenizer, device="cuda", window_size=3, step_size=1, scoring='generation', num_repeat=1,
                     max_new=None, sample_seed=None):
        """Build the ranker around an existing runtime (a loaded engine, or a test double) and tokenizer.  max_new: new tokens
        per `generation` compare (None: the installed transformers' default, resolve_max_new).  sample_seed: as in __init__
        (decoder-only runtimes)."""
        self = cls.__new__(cls)
        if getattr(runtime, "model_type", "t5") == "llama":        # the length comes from the runtime's generation settings
            self._setup(runtime, tokenizer, device, window_size, step_size, scoring, num_repeat, max_new, sample_seed)
        else:
            self._setup(runtime, tokenizer, device, window_size, step_size, scoring, num_repeat,
                        resolve_max_new() if max_new is None else int(max_new))
        return self

    def _setup(self, runtime, tokenizer, device, window_size, step_size, scoring, num_repeat, max_new, sample_seed=None):
        from ._runtime import require_decoder_positions
        require_decoder_positions(runtime, type(self).__name__)
        self.model_type = getattr(runtime, "model_type", "t5")
        if self.model_type == "llama" and not hasattr(runtime, "generate"):
            raise NotImplementedError(f"{LLAMA_MESSAGE} (Llama runtime {type(runtime).__name__})")
        self.device = device
        self.window_size = window_size
        self.step_size = step_size
        self.num_repeat = num_repeat
        self.scoring = scoring
        self.llm = runtime
        self.config = getattr(runtime, "config", None)
        self.tokenizer = tokenizer
        self.max_new = max_new
        self.total_compare = 0
        self.total_prompt_tokens = 0
        self.total_completion_tokens = 0
        self._seed_rng = None                    # sampling: one seed per compare, in compare order (the row's Philox key)
        if self.model_type == "llama":           # no decoder prompt / label ids: the reference's Llama branch sets none (ref :235-245)
            from ._runtime import sampling_plan
            plan = sampling_plan(runtime) if sample_seed is not None else None
            if plan is not None:                 # (an integer on a greedy checkpoint changes nothing)
                import random
                runtime.set_sampling(*plan)
                self._seed_rng = random.Random(int(sample_seed))
            return
        self.decoder_start = [int(getattr(runtime, "decoder_start_token_id", 0) or 0)]
        # likelihood: decoder prompt "<pad> Passage" and the last token of "<pad> Passage {label}" (ref: listwise.py:225-231)
        self.decoder_input_ids = self.tokenizer.encode("<pad> Passage", add_special_tokens=False)
        self.target_token_ids = [self.tokenizer.encode(f"<pad> Passage {c}", add_special_tokens=False)[-1] for c in self.CHARACTERS]

    # ------------------------------------------------------------------------------------------------------
    def _permutation_prompt(self, query: str, docs: List) -> str:
        num = len(docs)
        body = "".join(ENTRY.format(rank=r + 1, content=" ".join(d.text.replace('Title: Content: ', '').strip().split()[:MAX_WORDS]))
                       for r, d in enumerate(docs))
        return HEAD.format(num=num, query=query) + body + TAIL.format(num=num, query=query)

    def _chat_messages(self, query: str, docs: List) -> List[dict]:
        """create_permutation_instruction_chat(query, docs, model_name=None) (ref: listwise.py:63-88)"""
        num = len(docs)
        messages = [{'role': 'system', 'content': CHAT_SYSTEM},
                    {'role': 'user', 'content': CHAT_OPEN.format(num=num, query=query)},
                    {'role': 'assistant', 'content': CHAT_OPEN_REPLY}]
        for r, d in enumerate(docs):
            content = " ".join(d.text.replace('Title: Content: ', '').strip().split()[:MAX_WORDS])
            messages.append({'role': 'user', 'content': f"[{r + 1}] {content}"})
            messages.append({'role': 'assistant', 'content': f'Received passage [{r + 1}].'})
        messages.append({'role': 'user', 'content': CHAT_POST.format(num=num, query=query)})
        return messages

    def _chat_ids(self, query: str, docs: List) -> List[int]:
        """tokenizer.apply_chat_template(messages, add_generation_prompt=True) with tokenisation on (ref: listwise.py:263-264)"""
        ids = self.tokenizer.apply_chat_template(self._chat_messages(query, docs), add_generation_prompt=True, return_dict=False)
        return [int(t) for t in ids]

    def _compare_windows_llama(self, queries: List[str], doc_lists: List[List]):
        if self.scoring == 'likelihood':
            # ref: listwise.py:282 reads self.decoder_input_ids, which only the T5 branch sets
            raise AttributeError("'ListwiseLlmRanker' object has no attribute 'decoder_input_ids'")
        if self.scoring != 'generation':
            raise UnboundLocalError("local variable 'output' referenced before assignment")
        from ._runtime import generation_plan
        ids = [self._chat_ids(q, docs) for q, docs in zip(queries, doc_lists)]
        plan = generation_plan(self.llm, [len(i) for i in ids])
        if self.max_new is not None:
            plan["max_new"], plan["max_total"] = int(self.max_new), 0
        if self._seed_rng is not None:
            seeds = [self._seed_rng.getrandbits(64) for _ in ids]
            new = np.asarray(self.llm.generate(ids, plan["max_new"], plan["eos_ids"], plan["pad_id"], plan["max_total"], seeds=seeds))
        else:
            new = np.asarray(self.llm.generate(ids, plan["max_new"], plan["eos_ids"], plan["pad_id"], plan["max_total"]))
        outs, completion = [], []
        for prompt, row in zip(ids, new):
            toks = [int(t) for t in row if t >= 0]
            if plan["max_total"]:                                # alone, this row would have stopped at its own length limit
                toks = toks[:plan["max_total"] - len(prompt)]
            stop = next((i for i, t in enumerate(toks) if t in plan["eos_ids"]), None)
            if stop is not None:                                 # ... or at its own EOS
                toks = toks[:stop + 1]
            completion.append(len(prompt) + len(toks))           # the reference counts the prompt too (ref :269)
            outs.append(self.tokenizer.decode(toks, skip_special_tokens=True).strip())
        return outs, [len(i) for i in ids], completion

    def _label_prompt(self, query: str, docs: List) -> str:
        passages = "\n\n".join(f'Passage {self.CHARACTERS[i]}: "{doc.text}"' for i, doc in enumerate(docs))
        return QUESTION.format(query=query) + passages + INSTRUCTION

    def _truncated_ids(self, texts: List[str]) -> List[List[int]]:
        """tokenizer(text, truncation=True).input_ids (ref: listwise.py:244): the memoised full tokenisation, and the tokenizer
        itself for the prompts longer than model_max_length"""
        ids = tokenize_prompts(self.tokenizer, texts)
        limit = getattr(self.tokenizer, "model_max_length", None)
        for i, row in enumerate(ids):
            if limit is not None and len(row) > limit:
                ids[i] = list(self.tokenizer(texts[i], truncation=True)["input_ids"])
        return ids

    def _compare_windows(self, queries: List[str], doc_lists: List[List]):
        """ONE engine call for windows that may belong to different queries -> (outputs, prompt tokens per window, completion
        tokens per window); touches no counter.  A window's result does not depend on what shares the call."""
        if self.model_type == "llama":
            return self._compare_windows_llama(queries, doc_lists)
        if self.scoring == 'generation':
            ids = self._truncated_ids([self._permutation_prompt(q, docs) for q, docs in zip(queries, doc_lists)])
            eos, pad = self.tokenizer.eos_token_id, self.tokenizer.pad_token_id
            new = np.asarray(self.llm.generate(ids, self.decoder_start, self.max_new, eos, pad))
            outs, completion = [], []
            for row in new:
                toks = [int(t) for t in row if t >= 0]
                if eos in toks:                                  # alone, this row would have stopped at its own EOS
                    toks = toks[:toks.index(eos) + 1]
                out_ids = self.decoder_start + toks              # what generate() returns: the start token + the new ones
                completion.append(len(out_ids))
                outs.append(self.tokenizer.decode(out_ids, skip_special_tokens=True).strip())
            return outs, [len(i) for i in ids], completion
        if self.scoring == 'likelihood':
            ids = tokenize_prompts(self.tokenizer, [self._label_prompt(q, docs) for q, docs in zip(queries, doc_lists)])
            nmax = max(len(docs) for docs in doc_lists)
            lg = np.asarray(self.llm.score(ids, self.decoder_input_ids, self.target_token_ids[:nmax]))
            outs = []
            for r, docs in enumerate(doc_lists):
                # softmax is monotone: descending label logits, ties in window order (the reference's stable sort, :270-271)
                order = sorted(range(len(docs)), key=lambda i: -float(lg[r, i]))
                outs.append('>'.join(f"[{i + 1}]" for i in order))
            return outs, [len(i) for i in ids], [0] * len(ids)
        raise UnboundLocalError("local variable 'output' referenced before assignment")   # what the reference does

    def compare(self, query: str, docs: List):
        # ref: listwise.py:240-283
        self.total_compare += 1
        (output,), (ptok,), (ctok,) = self._compare_windows([query], [docs])
        self.total_prompt_tokens += ptok
        self.total_completion_tokens += ctok
        return output

    # ---- the sliding-window walk ------------------------------------------------------------------------------
    def _walk(self, ranking):
        """The reference's walk (ref: listwise.py:180-199) as a chain of _lockstep: yields each window (a list of one), is sent
        the compare's output, and returns the final ranking.  Windows start at n - window_size and move down by step_size while
        the start is >= 0."""
        for _ in range(self.num_repeat):
            ranking = copy.deepcopy(ranking)
            end, start = len(ranking), len(ranking) - self.window_size
            while start >= 0:
                window = ranking[start:end]
                (output,) = yield [window]
                ranking[start:end] = [window[k] for k in permutation_order(output, len(window))]
                end -= self.step_size
                start -= self.step_size
        for i, doc in enumerate(ranking):
            doc.score = -i
        return ranking

    def rerank(self, query: str, ranking: List[SearchResult]) -> List[SearchResult]:
        self.total_compare = 0
        self.total_prompt_tokens = 0
        self.total_completion_tokens = 0
        return drive(self._walk(ranking), lambda windows: [self.compare(query, window) for window in windows])

    def rerank_many(self, items):
        """Several queries at once: `items` = [(query, ranking), ...] -> (results, counters); results[i] and counters[i] =
        (total_compare, total_prompt_tokens, total_completion_tokens) are what `rerank(*items[i])` gives.  Each query's windows
        are a dependency chain; the pending windows of all live chains go to the engine as ONE call per step."""
        items = list(items)
        counts = [[0, 0, 0] for _ in items]
        walks = Lockstep({q: self._walk(ranking) for q, (_, ranking) in enumerate(items)})
        while walks:
            keys, windows = walks.pending()
            walks.advance(tally(counts, keys, *self._compare_windows([items[q][0] for q in keys], windows)))
        return [walks.returned[q] for q in range(len(items))], close_counters(self, counts)

    def truncate(self, text, length):
        return self.tokenizer.convert_tokens_to_string(self.tokenizer.tokenize(text)[:length])


_WEIGHT_DTYPE_CLASSES = {}      # (class, weight_dtype) -> the subclass with_weight_dtype hands out


class R1ListwiseLlmRanker(ListwiseLlmRanker):
    """The listwise baseline of Rank-R1 (ref: Rank-R1/run_listwise.py:89-156; RankZephyr - a Zephyr / Mistral-7B checkpoint with a
    sliding window - or any chat model, served by vLLM there): one compare = the two-message chat prompt of the prompt settings
    (system, and the user message with the window's passages as "[n] text" lines), a greedy completion of up to max_new_tokens
    tokens, and the settings' regular expression that takes the permutation out of it ('None' when it does not match: the window
    stays as it is).  Here the checkpoint (a LoRA adapter merged on the host, _runtime.merge_lora) runs on the engine's KV-cached
    greedy decoder; a Mistral checkpoint's sliding window is the engine's (rk_llama_set_sliding_window).  Same constructor,
    compare() contract, counters and window walk as the reference; the stand-ins for vLLM are RankR1SetwiseLlmRanker's (DESIGN.md
    section 3, "Qwen2 family and Rank-R1"): the stop ids and the pad id are the checkpoint's generation settings, the EOS that ended
    a row counts as a completion token, the completion text is the new tokens decoded without special tokens.  Only the windows
    call is this class's own: compare, rerank, rerank_many (the pending windows of all live queries in ONE generate call per step)
    and truncate are ListwiseLlmRanker's."""
    CHARACTERS = [f'[{i + 1}]' for i in range(20)]
    ACCEPT_MODEL_TYPES = ("qwen2", "llama", "mistral", "qwen3")      # vLLM takes any chat model; these are the families the engine serves

    # FP8 step weights (LlamaRuntime's weight_dtype; lossy, opt-in).  The constructor keeps the reference's parameter list, so the
    # option is the class's: R1ListwiseLlmRanker.with_weight_dtype("fp8")(model, tokenizer, prompt, ...)
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

    # Drafting by prompt lookup (LlamaRuntime.open_pool's draft_tokens; lossless, opt-in: the same tokens in fewer steps):
    # R1ListwiseLlmRanker.with_draft_tokens(3)(model, tokenizer, prompt, ...).  With it on, the windows of a call decode through a
    # drafting pool instead of rk_llama_generate.
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

    def __init__(self, model_name_or_path, tokenizer_name_or_path, prompt, window_size, step_size, lora_path=None,
                 scoring='generation', num_repeat=1, cache_dir=None, device="cuda", max_new_tokens=2048):
        from transformers import AutoTokenizer
        from ._runtime import LlamaRuntime, kv_dtype_kw, resolve_checkpoint, weight_dtype_kw
        from .setwise import load_prompt_file
        prompt = load_prompt_file(prompt)
        lora_path = resolve_checkpoint(lora_path, cache_dir) if lora_path is not None else None
        tokenizer = AutoTokenizer.from_pretrained(tokenizer_name_or_path if tokenizer_name_or_path is not None else model_name_or_path,
                                                  cache_dir=cache_dir)
        runtime = LlamaRuntime(model_name_or_path, device, cache_dir=cache_dir, accept_model_types=self.ACCEPT_MODEL_TYPES,
                               adapter_dir=lora_path, **weight_dtype_kw(self.weight_dtype), **kv_dtype_kw(self.kv_dtype))
        self._setup_r1(runtime, tokenizer, prompt, lora_path, device, window_size, step_size, scoring, num_repeat, max_new_tokens)

    @classmethod
    def from_runtime(cls, runtime, tokenizer, prompt, device="cuda", window_size=3, step_size=1, scoring='generation', num_repeat=1,
                     max_new_tokens=2048):
        """Build the ranker around an existing runtime (a loaded engine - adapter already merged - or a test double)."""
        from .setwise import load_prompt_file
        self = cls.__new__(cls)
        self._setup_r1(runtime, tokenizer, load_prompt_file(prompt), None, device, window_size, step_size, scoring, num_repeat, max_new_tokens)
        return self

    def _setup_r1(self, runtime, tokenizer, prompt, lora_path, device, window_size, step_size, scoring, num_repeat, max_new_tokens):
        if not hasattr(runtime, "generate"):
            raise NotImplementedError(f"{LLAMA_MESSAGE} (runtime {type(runtime).__name__})")
        self.prompt = prompt
        self.lora_path = lora_path
        self.device = device
        self.window_size = window_size
        self.step_size = step_size
        self.num_repeat = num_repeat
        self.scoring = scoring                              # (the reference takes the argument and never reads it)
        self.max_new_tokens = int(max_new_tokens)           # the reference's SamplingParams(temperature=0.0, max_tokens=2048)
        self.tokenizer = tokenizer
        self.llm = runtime
        self.config = getattr(runtime, "config", None)
        self.model_type = getattr(runtime, "model_type", "mistral")
        self.total_compare = 0
        self.total_prompt_tokens = 0
        self.total_completion_tokens = 0

    def _chat_messages(self, query: str, docs: List) -> List[dict]:
        passages = "\n".join(f'{self.CHARACTERS[i]} {doc.text}' for i, doc in enumerate(docs))
        return [{'role': "system", 'content': self.prompt["prompt_system"]},
                {'role': "user", 'content': self.prompt['prompt_user'].format(query=query, num=len(docs), docs=passages)}]

    def _chat_ids(self, query: str, docs: List) -> List[int]:
        """what vLLM's LLM.chat feeds the model: the chat template with the generation prompt, tokenized"""
        out = self.tokenizer.apply_chat_template(self._chat_messages(query, docs), add_generation_prompt=True, tokenize=True)
        if hasattr(out, "keys"):                             # transformers >= 5 returns a BatchEncoding
            out = out["input_ids"]
        return [int(t) for t in out]

    def _compare_windows(self, queries: List[str], doc_lists: List[List]):
        """ONE generate call for windows that may belong to different queries -> (returned strings, prompt tokens per window, new
        tokens per window); touches no counter (ref: run_listwise.py:121-156 per window)."""
        import re
        ids = [self._chat_ids(q, docs) for q, docs in zip(queries, doc_lists)]
        gen = self.llm.generation
        eos_ids = list(gen["eos_token_ids"])
        if self.draft_tokens and hasattr(self.llm, "open_pool"):           # the same tokens through a drafting pool
            from ._runtime import generate_drafted
            rows = generate_drafted(self.llm, ids, self.max_new_tokens, eos_ids, int(gen["pad_token_id"]), self.draft_tokens)
        else:
            rows = np.asarray(self.llm.generate(ids, self.max_new_tokens, eos_ids, int(gen["pad_token_id"])))
        outs, completion = [], []
        for q, docs, row in zip(queries, doc_lists, rows):
            new = [int(t) for t in row if t >= 0]
            stop = next((i for i, t in enumerate(new) if t in eos_ids), None)
            if stop is not None:                             # vLLM's token_ids keep the EOS that ended the row
                new = new[:stop + 1]
            completion.append(len(new))
            text = self.tokenizer.decode(new, skip_special_tokens=True)
            match = re.search(rf'{self.prompt["pattern"]}', text.lower(), re.DOTALL)
            if match:
                outs.append(match.group(1).strip())
            else:
                outs.append('None')
                print('Input for no match:', self._chat_messages(q, docs))
                print('Completion for no match:', text)
        return outs, [len(i) for i in ids], completion
