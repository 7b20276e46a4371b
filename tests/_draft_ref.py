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
