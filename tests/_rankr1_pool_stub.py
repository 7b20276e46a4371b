"""Host stand-ins for the Rank-R1 many-query path: a decoding session that replays scripted completions one token per step, and a
runtime whose `generate` and `open_pool` answer every prompt from the same table - a pure function of the prompt's ids, so a prompt
gets the same completion whichever way it reaches the runtime."""
import hashlib

import numpy as np

EOS, PAD = 2, 0            # tok_qwen: <|im_end|>, <|endoftext|>


class FakeSession:
    """RkLlamaEngine.session's interface over a `completion(ids, max_new) -> tokens` function.  Like the engine's: column 0 is
    produced at admit, a run steps every active slot until one finishes and issues one more step (the one queued ahead), a
    finished slot keeps its row until it is read."""

    def __init__(self, completion, n_slots, max_len, max_new_cap, log):
        self.completion, self.n_slots, self.max_len, self.max_new_cap, self.log = completion, n_slots, max_len, max_new_cap, log
        self.busy, self.rows, self.col, self.told = set(), {}, {}, set()
        self.is_open, self.steps = True, 0
        log.append(("open", n_slots, max_len))

    def close(self):
        if self.is_open:
            self.is_open = False
            self.log.append(("close", sorted(self.busy)))

    def admit(self, seqs, slots, max_new):
        assert self.is_open and len(seqs) == len(slots) == len(max_new) and len(set(slots)) == len(slots)
        for ids, slot, m in zip(seqs, slots, max_new):
            assert 0 <= slot < self.n_slots and slot not in self.busy, "admit to a busy slot"
            assert m <= self.max_new_cap and len(ids) + m <= self.max_len
            self.rows[slot] = list(self.completion(ids, m))
            self.col[slot] = 1
            self.busy.add(slot)
        assert len(self.busy) <= self.n_slots
        self.log.append(("admit", list(slots), [len(s) for s in seqs]))

    def _done(self, slot):
        return self.col[slot] >= len(self.rows[slot])

    def run(self, max_steps=1 << 30):
        assert self.is_open
        steps = 0

        def untold():
            return any(self._done(s) and s not in self.told for s in self.busy)

        def step():
            for s in self.busy:
                if not self._done(s):
                    self.col[s] += 1
            return 1

        if not untold():
            while steps < max_steps and any(not self._done(s) for s in self.busy):
                steps += step()
                if untold():
                    if steps < max_steps and any(not self._done(s) for s in self.busy):
                        steps += step()                                # the step queued ahead of the host's check
                    break
        finished = sorted(s for s in self.busy if self._done(s) and s not in self.told)
        self.told.update(finished)
        self.steps += steps
        return finished, steps

    def read(self, slot):
        assert slot in self.told, "read of a slot that no run reported"
        self.busy.discard(slot)
        self.told.discard(slot)
        return np.asarray(self.rows.pop(slot), dtype=np.int32)


class ScriptedRuntime:
    """generate / open_pool over a table of completions: entry = (filler tokens before the answer, answer kind).  Which entry and
    which label a prompt gets follows from a hash of its ids; lengths differ, so completions return out of submission order."""
    model_type = "qwen2"
    TABLE = ((0, "label"), (7, "label"), (2, "none"), (11, "label"), (4, "label"), (1, "beyond"), (9, "label"))

    def __init__(self, tokenizer, n_slots=4, max_tokens=4096):
        self.tok = tokenizer
        self.generation = {"eos_token_ids": [EOS], "pad_token_id": PAD}
        self.max_seqs, self.max_tokens = n_slots, max_tokens
        self.think = tokenizer.convert_tokens_to_ids("think")
        self.labels = [tokenizer.convert_tokens_to_ids(f"[{i + 1}]") for i in range(20)]
        self.log, self.generate_calls = [], 0

    def completion(self, ids, max_new):
        h = int.from_bytes(hashlib.sha256(np.asarray(ids, np.int32).tobytes()).digest()[:8], "little")
        filler, kind = self.TABLE[h % len(self.TABLE)]
        shown = sum(1 for t in ids if t in self.labels)                # labels the prompt lists
        new = [self.think] * filler
        if kind == "label":
            new.append(self.labels[(h >> 8) % max(1, shown)])
        elif kind == "beyond":
            new.append(self.labels[min(shown, 19)])                    # a label no passage of the window carries
        return (new + [EOS])[:max_new]

    def generate(self, seqs, max_new, eos_ids, pad_id, max_total=0):
        self.generate_calls += 1
        rows = [self.completion(s, max_new) for s in seqs]
        steps = max(len(r) for r in rows)
        out = np.full((len(seqs), max_new), -1, dtype=np.int32)
        for b, r in enumerate(rows):
            out[b, :steps] = pad_id
            out[b, :len(r)] = r
        return out

    def open_pool(self, max_new_cap, eos_ids, pad_id, n_slots=None):
        from llmrankers._runtime import DecodePool
        n = self.max_seqs if n_slots is None else n_slots
        return DecodePool(lambda max_len: FakeSession(self.completion, n, max_len, max_new_cap, self.log), n, self.max_tokens, max_new_cap)
