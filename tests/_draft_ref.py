"""Python reference of a drafting session (rk_llama_session_open_draft): the prompt-lookup proposer (draft_lookup_kernel) and the
accept machine (llama_session_advance_draft_kernel), as pure functions of (prompt, plain output, Kd, ngram range, max_new, eos).

The model enters through the PLAIN session's output alone: a row whose fed tokens are the plain session's tokens emits the plain
session's next token (a row's bits follow from its own tokens and position), and the machine never needs the token of a row behind
a wrong draft - that row is rejected whatever it says."""
from typing import List, Optional, Sequence, Tuple


def propose(hist: Sequence[int], kd: int, ngram_min: int, ngram_max: int) -> List[int]:
    """The drafts for history h[0, n): for N from ngram_max down to ngram_min, the largest i with h[i, i+N) == h[n-N, n) and
    i + N < n proposes h[i+N, min(i+N+kd, n)).  [] without a match."""
    h, n = list(hist), len(hist)
    for N in range(ngram_max, ngram_min - 1, -1):
        if N > n - 1:
            continue
        tail = h[n - N:]
        for i in range(n - N - 1, -1, -1):
            if h[i:i + N] == tail:
                return h[i + N:min(i + N + kd, n)]
    return []


def draft_limit(n: int, col: int, kd: int, max_new: int, max_len: int, cap: Optional[int] = None) -> int:
    """How many draft rows may be live for a slot whose history has n tokens and whose output has col: none beyond position
    max_len - 1 (row j sits at n - 1 + j), none beyond the tokens the request may still emit after this step's first."""
    cap = max_new if cap is None else cap
    return max(0, min(kd, max_len - n, min(max_new, cap) - col - 1))


def run_machine(prompt: Sequence[int], plain_out: Sequence[int], kd: int, ngram: Tuple[int, int], max_new: int, eos: Sequence[int],
                max_len: int, cap: Optional[int] = None, table: Optional[Sequence[int]] = None):
    """-> (tokens, steps, accepted per step).  plain_out: what the plain session emits for this prompt (its EOS included).
    table: rk_debug_session_drafts' continuation table (the draft for column c is table[c]) in place of the lookup."""
    cap = max_new if cap is None else cap
    eos = set(int(t) for t in eos)
    plain_out = [int(t) for t in plain_out]

    def ended(out):
        return out[-1] in eos or len(out) >= max_new or len(out) >= cap

    out = [plain_out[0]]                                   # the admit's token: the prefill's arg-max
    steps, accepted = 0, []
    while not ended(out):
        c = len(out)
        n = len(prompt) + c
        lim = draft_limit(n, c, kd, max_new, max_len, cap)
        if table is not None:
            drafts = [int(t) for t in table[c:c + lim]]
        else:
            drafts = propose(list(prompt) + out, kd, ngram[0], ngram[1])[:lim]
        steps += 1
        out.append(plain_out[c])                           # t_0: always accepted
        k = 1
        for j, d in enumerate(drafts, 1):
            if ended(out) or d != out[-1]:
                break
            out.append(plain_out[c + j])                   # row j saw the plain session's tokens: it emits the plain token
            k += 1
        accepted.append(k)
    return out, steps, accepted


# ---- the drafting session's device state, array for array (rk_debug_draft_steps) -----------------------------------------------------------
import numpy as np

ARRAYS = ("st", "len", "col", "max_new", "done", "out", "rnext", "rpos", "rlive", "dlen", "nstep", "tabn", "tab", "hist")
MUTANTS = ("lookup_smallest_i", "lookup_drops_256", "lookup_nmin_first", "accept_past_mismatch", "accept_past_eos")


class DraftMachine:
    """The whole int state of a drafting session and its three transitions, written from the comments above
    llama_session_advance_draft_kernel and draft_lookup_kernel (csrc/misc_kernels.h), integers only.
    st = {finishes so far, pad, n_eos, max_len, cap, ngram_min, ngram_max, 0, eos[8]}; per slot len, col, max_new, done (1: idle or
    finished), out [cap], nstep, dlen, tabn (-1: the lookup), tab [cap], hist [max_len]; per step row rnext, rpos, rlive.
    Every slot starts idle.  `events` collects what the run met (the host test asserts the fixed scripts meet every edge).
    mut: one of MUTANTS - a machine that is wrong in that one way."""

    def __init__(self, n_slots, g1, max_len, cap, eos, pad, ngram, mut=None):
        i32 = np.int32
        S = n_slots
        self.S, self.g1, self.max_len, self.cap, self.pad, self.mut = S, g1, max_len, cap, pad, mut
        self.eos, self.nmin, self.nmax = [int(t) for t in eos], int(ngram[0]), int(ngram[1])
        self.st = np.array([0, pad, len(self.eos), max_len, cap, self.nmin, self.nmax, 0] + (self.eos + [0] * 8)[:8], i32)
        self.len, self.col, self.max_new, self.dlen, self.nstep = (np.zeros(S, i32) for _ in range(5))
        self.done = np.ones(S, i32)
        self.out, self.tab = np.full((S, cap), -1, i32), np.full((S, cap), -1, i32)
        self.hist = np.full((S, max_len), -1, i32)
        self.tabn = np.full(S, -1, i32)
        self.rnext, self.rpos, self.rlive = np.full((S, g1), pad, i32), np.zeros((S, g1), i32), np.zeros((S, g1), i32)
        self.rlive[:, 0] = 1
        self.events = set()

    def state(self):
        return [getattr(self, k).reshape(-1).copy() for k in ARRAYS]

    # -- the accept machine --
    def _accept(self, b, toks, dl):
        """toks: the arg-max of the slot's rows 0 .. dl; t_0 always, t_j while d_j == t_{j-1} and no accepted token ended the slot."""
        c, L, mn = int(self.col[b]), int(self.len[b]), int(self.max_new[b])
        ended, seen_eos, k = False, False, 0
        for j in range(dl + 1):
            if j > 0 and int(self.rnext[b, j]) != int(toks[j - 1]) and self.mut != "accept_past_mismatch":
                break
            tok = int(toks[j])
            if c < self.cap:
                self.out[b, c] = tok
            if L + c < self.max_len:
                self.hist[b, L + c] = tok
            c += 1
            k += 1
            is_eos, full = tok in self.eos, c >= mn or c >= self.cap
            if is_eos and j == 0 and dl > 0:
                self.events.add("eos_row0_live_drafts")
            if is_eos and 0 < j < dl:
                self.events.add("eos_middle")
            if full and not is_eos and 0 < j < self.g1 - 1:
                self.events.add("end_cap_middle" if mn >= self.cap else "end_max_new_middle")
            seen_eos = seen_eos or is_eos
            if full or (is_eos and self.mut != "accept_past_eos"):
                ended = True
                break
        self.col[b] = c
        if dl > 0:
            self.events.add("accept_all" if k == self.g1 else ("accept_t0_only" if k == 1 else "accept_some"))
        if ended or seen_eos:
            self.done[b] = 1
            self.st[0] += 1

    # -- the proposer --
    def _match(self, h, n, N):
        """the largest i with h[i, i + N) == h[n - N, n) and i + N < n, or -1"""
        w = np.lib.stride_tricks.sliding_window_view(h[:n - 1], N)            # windows i = 0 .. n - 1 - N
        hit = np.flatnonzero((w == h[n - N:n]).all(axis=1))
        if self.mut == "lookup_drops_256":
            hit = hit[hit < 256]
        if hit.size == 0:
            return -1
        best = int(hit[-1])
        if n > 512 and best >= 256 and (hit < 256).any():
            self.events.add("best_beyond_256_of_several")
        if best + N > n - N:
            self.events.add("overlapping_match")
        return int(hit[0]) if self.mut == "lookup_smallest_i" else best

    def _lookup(self, s):
        g1, Kd, pad = self.g1, self.g1 - 1, self.pad
        if self.done[s]:                                       # row 0 feeds pad at the position it has
            self.rnext[s, :] = pad
            self.rpos[s, 1:] = 0
            self.rlive[s, 0], self.rlive[s, 1:] = 1, 0
            self.dlen[s] = 0
            return
        c, L, mn = int(self.col[s]), int(self.len[s]), int(self.max_new[s])
        n = L + c
        h = self.hist[s]
        terms = (Kd, self.max_len - n, min(mn, self.cap) - c - 1)
        lim = max(0, min(terms))
        assert terms[1] > terms[2], "len + max_new <= max_len: the cache's end never binds before the request's"
        if Kd > 0:
            self.events.add("lim_by_kd" if terms[0] <= terms[2] else "lim_by_remaining")
        drafts = []
        if self.tabn[s] >= 0:
            if self.tabn[s] < c:
                self.events.add("table_shorter_than_col")
            drafts = [int(t) for t in self.tab[s, c:max(c, min(c + lim, int(self.tabn[s])))]]
        elif lim > 0:
            order = range(self.nmax, self.nmin - 1, -1) if self.mut != "lookup_nmin_first" else range(self.nmin, self.nmax + 1)
            tried = 0
            for N in order:
                if N > n - 1:
                    if L == 1:
                        self.events.add("ngram_longer_than_one_token_prompt")
                    continue
                tried += 1
                i = self._match(h, n, N)
                if i >= 0:
                    self.events.add("match_at_nmax" if N == self.nmax else "match_at_smaller_n")
                    src = i + N
                    if n - src < min(lim, Kd):
                        self.events.add("continuation_clipped_by_n")
                    drafts = [int(t) for t in h[src:min(src + lim, n)]]
                    break
            else:
                if tried:
                    self.events.add("no_match")
        dl = len(drafts)
        self.rnext[s, 0], self.rpos[s, 0], self.rlive[s, 0], self.dlen[s] = h[n - 1], min(n - 1, self.max_len - 1), 1, dl
        for j in range(1, g1):
            on = j <= dl
            self.rnext[s, j], self.rpos[s, j], self.rlive[s, j] = (drafts[j - 1], n - 1 + j, 1) if on else (pad, 0, 0)

    def _propose(self):
        for s in range(self.S):
            self._lookup(s)

    # -- the three transitions --
    def step(self, argmax):
        """argmax [n_slots g1]: one decoding step of every active slot, then the proposer"""
        argmax = np.asarray(argmax).reshape(-1)
        for b in range(self.S):
            if self.done[b]:
                continue
            dl = int(self.dlen[b])
            self._accept(b, argmax[b * self.g1:b * self.g1 + dl + 1], dl)
            self.nstep[b] += 1
        self._propose()
        return self

    def admit(self, slots, lens, max_news, prompts, argmax):
        """Row r of argmax is the prefill's last row of slot slots[r], which starts here with prompts[r] (lens[r] tokens) in its
        history and argmax[r] as its column 0; a slot id outside [0, n_slots) is skipped.  Then the proposer."""
        if len(slots) == 0:
            self.events.add("empty_admit")
        for r, b in enumerate(slots):
            if b < 0 or b >= self.S:
                self.events.add("admit_slot_out_of_range")
                continue
            if (self.done == 0).any():
                self.events.add("admit_beside_running_slots")
            L = int(lens[r])
            if L > 256:
                self.events.add("prompt_longer_than_256")
            self.len[b], self.max_new[b], self.col[b], self.done[b], self.nstep[b] = L, max_news[r], 0, 0, 0
            self.hist[b, :min(L, self.max_len)] = np.asarray(prompts[r][:L], np.int32)[:self.max_len]
            self._accept(b, [argmax[r]], 0)
        self._propose()
        return self

    def set_table(self, slot, tokens):
        """rk_debug_session_drafts: the slot's drafts come from `tokens` by output column (None: back to the lookup); the proposer alone"""
        self.events.add("table_change")
        if tokens is None:
            self.tabn[slot] = -1
        else:
            self.tab[slot, :len(tokens)] = tokens
            self.tabn[slot] = len(tokens)
        self._propose()
        return self


# ---- fixed scripts: the reference run in lock step with a generator that knows the next drafts ---------------------------------------------
import functools

MAX_LEN, CAP, PAD, EOS, VOCAB = 640, 24, 0, (1, 2), (5, 6, 7)
N_SLOTS, G1S, NGRAMS = (3, 257), (2, 4, 8), ((1, 3), (2, 4), (8, 8), (1, 8))
P_DRAFT, P_EOS = 0.7, 0.08                                    # a row repeats the next draft / emits an EOS id with these probabilities


def record_len(n_slots, g1, max_admit, max_tokens):
    return 4 + max(n_slots * g1, max_admit) + 3 * max_admit + (max_admit + 1) + max_tokens


def pack_script(steps, n_slots, g1, max_admit, max_tokens):
    """steps (dicts: kind, and argmax / slots, lens, max_news, prompts / slot, tokens) -> int32 [n_steps, rec], rk_debug_draft_steps' layout"""
    A = max(n_slots * g1, max_admit)
    o_adm, o_off, o_tok = 4 + A, 4 + A + 3 * max_admit, 4 + A + 3 * max_admit + max_admit + 1
    out = np.full((len(steps), record_len(n_slots, g1, max_admit, max_tokens)), -3, np.int32)
    for r, s in zip(out, steps):
        r[:4] = (s["kind"], 0, 0, 0)
        if s["kind"] == 0:
            r[4:4 + n_slots * g1] = s["argmax"]
        elif s["kind"] == 1:
            n = len(s["slots"])
            r[1] = n
            r[4:4 + n] = s["argmax"]
            r[o_adm:o_adm + 3 * n] = list(s["slots"]) + list(s["lens"]) + list(s["max_news"])
            off = 0
            for i, p in enumerate(s["prompts"]):
                r[o_off + i] = off
                r[o_tok + off:o_tok + off + len(p)] = p
                off += len(p)
            r[o_off + n] = off
        else:
            r[1], r[2] = (-1 if s["tokens"] is None else len(s["tokens"])), s["slot"]
            if s["tokens"] is not None:
                r[o_tok:o_tok + len(s["tokens"])] = s["tokens"]
    return out


def apply(m, s):
    if s["kind"] == 0:
        return m.step(s["argmax"])
    if s["kind"] == 1:
        return m.admit(s["slots"], s["lens"], s["max_news"], s["prompts"], s["argmax"])
    return m.set_table(s["slot"], s["tokens"])


def replay(steps, n_slots, g1, ngram, mut=None):
    """the states after every step of a machine (mut: a wrong one) fed the fixed script"""
    m = DraftMachine(n_slots, g1, MAX_LEN, CAP, EOS, PAD, ngram, mut=mut)
    return [apply(m, s).state() for s in steps], m


@functools.lru_cache(maxsize=None)
def build_script(n_slots, g1, ngram):
    """-> (steps, initial state, states after every step, events, max_admit, max_tokens).  Fixed by its parameters.  The generator
    runs the reference alongside: row j of an active slot repeats the slot's next draft with probability P_DRAFT (so row j + 1 is
    accepted), else draws from VOCAB; rows of slots other than the two that must reach their cap / max_new emit an EOS id with
    probability P_EOS; dead rows and idle slots get ids >= 90 that no accepted token may show."""
    S, nmax = n_slots, ngram[1]
    rs = np.random.RandomState(1000 * S + 10 * g1 + ngram[0] + 7 * nmax)
    m = DraftMachine(S, g1, MAX_LEN, CAP, EOS, PAD, ngram)
    init, steps, states = m.state(), [], []
    no_eos = {0, 2}

    def draw(n):
        return [int(t) for t in rs.choice(VOCAB, size=n)]

    def row(s, j, dl):
        u = rs.rand()
        if s not in no_eos and u < P_EOS:
            return int(rs.choice(EOS))
        if j < dl and u < P_EOS + P_DRAFT:
            return int(m.rnext[s, j + 1])
        return draw(1)[0]

    def do(s):
        steps.append(s)
        states.append(apply(m, s).state())

    def plain(n=1, forced=None):
        for _ in range(n):
            a = 90 + rs.randint(0, 9, size=S * g1)
            for s in np.flatnonzero(m.done == 0):
                dl = int(m.dlen[s])
                a[s * g1:s * g1 + dl + 1] = [row(s, j, dl) for j in range(dl + 1)]
                if forced and s in forced:
                    a[s * g1:s * g1 + dl + 1] = forced[s][:dl + 1]
            do({"kind": 0, "argmax": a.astype(np.int32)})

    def admit(slots, max_news, prompts, argmax):
        do({"kind": 1, "slots": slots, "lens": [len(p) for p in prompts], "max_news": max_news, "prompts": prompts, "argmax": argmax})

    # admit A: a periodic prompt that runs to the cap; 600 tokens that end in the first 7 of an 8-gram planted at 100 and at 400 with
    # other continuations (the admit's token completes it: the best match lies beyond 256, another below); an id out of range; one token
    X = draw(8)
    long_p = draw(600)
    long_p[100:116] = X + [5, 5, 6, 6, 7, 7, 5, 6]
    long_p[400:416] = X + [7, 6, 5, 7, 6, 5, 7, 7]
    long_p[-7:] = X[:7]
    admit([0, 1, S, S - 1], [CAP, 20, 3, 3], [[5, 6, 7] * 4, long_p, draw(4), [5]], [5, X[7], 6, 5])
    plain(2)                                                  # (the one-token request has its three tokens by now)
    # admit B beside running slots: 300 tokens up to its max_new below the cap; with 257 slots every other slot as well (more than 256
    # admit rows: the rows beyond 256 name real slots; slot 256 is active)
    slots, mns, prompts = [S + 3, -1, 2, 1 << 20], [4, 4, 9, 4], [draw(2), draw(3), draw(300), draw(1)]   # three more ids out of range
    for s in range(3, S - 1):
        slots.append(s), mns.append(int(rs.randint(2, 7))), prompts.append(draw(int(rs.randint(3, 9))))
    admit(slots, mns, prompts, [row(s, 0, 0) for s in slots])
    plain(1)
    do({"kind": 2, "slot": 0, "tokens": [7]})                 # a table shorter than the slot's column: no drafts
    plain(1)
    do({"kind": 2, "slot": 0, "tokens": draw(CAP)})           # a whole table
    plain(1)
    admit([], [], [], [])                                     # an empty admit touches nothing
    plain(1)
    do({"kind": 2, "slot": 0, "tokens": None})                # back to the lookup
    plain(1)
    while not m.done[S - 1]:
        plain(1)
    admit([S - 1], [CAP], [[6, 7] * 9], [6])                  # a finished slot again, beside running ones; runs to the cap too
    no_eos.add(S - 1)
    while (m.done == 0).any():
        plain(1)
    # three forced steps on periodic prompts that hold EOS ids (the drafts are the period's next tokens): the EOS id that IS the next
    # draft at row 0 with live drafts behind it, the same at row 1, and a row 0 that contradicts its draft with right rows behind it
    admit([0, 1, 2], [8, 8, 8], [[5, 1, 6] * 5, [5, 6, 2, 7] * 4, [5, 6, 7] * 5], [5, 5, 5])
    assert m.rnext[0, 1] == 1 and m.rnext[1, 1] == 6 and m.rnext[2, 1] == 6 and (g1 == 2 or (m.rnext[1, 2] == 2 and m.dlen[1] >= 2))
    plain(1, forced={0: [1, 6, 5, 1, 6, 5, 1, 6], 1: [6, 2, 7, 5, 6, 2, 7, 5], 2: [7, 7, 5, 6, 7, 5, 6, 7]})
    while (m.done == 0).any():
        plain(1)
    plain(2)                                                  # steps past the end change nothing but stay in bounds
    max_admit = max(len(s["slots"]) for s in steps if s["kind"] == 1)
    max_tokens = max([sum(s["lens"]) for s in steps if s["kind"] == 1] + [CAP])
    return steps, init, states, frozenset(m.events), max_admit, max_tokens
