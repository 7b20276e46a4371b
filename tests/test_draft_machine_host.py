"""The reference of the drafting session's state machine (tests/_draft_ref.py: DraftMachine) and the fixed scripts the GPU test
(tests/test_gpu_draft_machine.py) replays, checked without a GPU: the scripts meet every edge the kernels have, the record layout is
the header's, the machine agrees with the session-level reference, and a machine that is wrong in one way is told apart on these very
scripts."""
import os
import re

import numpy as np
import pytest

import _draft_ref as D
from conftest import REPO

CASES = [(S, g1, ng) for S in D.N_SLOTS for g1 in D.G1S for ng in D.NGRAMS]
EVERYWHERE = {"admit_beside_running_slots", "admit_slot_out_of_range", "empty_admit", "table_change", "table_shorter_than_col",
              "prompt_longer_than_256", "best_beyond_256_of_several", "overlapping_match", "match_at_nmax", "no_match",
              "ngram_longer_than_one_token_prompt", "lim_by_kd", "accept_t0_only", "eos_row0_live_drafts"}
SOMEWHERE = {"accept_all", "accept_some", "eos_middle", "end_max_new_middle", "end_cap_middle",
             "match_at_smaller_n", "continuation_clipped_by_n", "lim_by_remaining"}


def test_scripts_meet_every_edge():
    """Per script what a fixed scenario guarantees; over the scripts of one slot count what depends on the draws (a middle row needs
    g1 > 2, a smaller N needs ngram_min < ngram_max).  The cache's end never sets the draft limit: len + max_new <= max_len makes
    max_len - n larger than the request's remaining tokens (DraftMachine asserts it at every lookup)."""
    for S in D.N_SLOTS:
        union = set()
        for _, g1, ng in (c for c in CASES if c[0] == S):
            steps, init, states, ev, max_admit, max_tokens = D.build_script(S, g1, ng)
            union |= ev
            for want in EVERYWHERE:
                assert any(w in ev for w in want.split("|")), (S, g1, ng, want)
            assert len(steps) == len(states) and max_admit == (257 if S == 257 else 4)
            final = dict(zip(D.ARRAYS, states[-1]))
            assert final["done"].all() and all(np.array_equal(a, b) for a, b in zip(states[-1], states[-3])), "steps past the end change nothing"
            out = final["out"].reshape(S, D.CAP)
            assert (out < 90).all(), "a dead row's or an idle slot's arg-max was accepted"
            for slot in (0, S - 1):
                assert any(st[D.ARRAYS.index("done")][slot] == 1 and st[D.ARRAYS.index("col")][slot] == D.CAP for st in states), "the runs to the cap"
            assert "eos_middle" in ev or g1 == 2
            assert any(st[D.ARRAYS.index("done")][2] == 1 and st[D.ARRAYS.index("col")][2] == 9 for st in states), "the run to max_new = 9"
            assert max(int(st[D.ARRAYS.index("len")][1]) + int(st[D.ARRAYS.index("col")][1]) for st in states) > 512, "a history beyond 512 tokens"
            if S == 257:
                assert any(s["kind"] == 1 and len(s["slots"]) > 256 and 0 <= s["slots"][-1] < S for s in steps), "admit rows beyond 256"
                assert any(st[D.ARRAYS.index("done")][256] == 0 for st in states), "slot 256 decodes"
        assert SOMEWHERE <= union, (S, sorted(SOMEWHERE - union))


def test_script_records_have_the_headers_layout():
    header = open(os.path.join(REPO, "include", "rk_engine.h")).read()
    assert "rec = 4 + A + 3 max_admit + (max_admit + 1) + max_tokens, A = max(n_slots g1, max_admit)" in header
    assert "kind | n | slot | 0 | argmax[A] | admit[3 max_admit] | seq_off[max_admit + 1] | tokens[max_tokens]" in header
    order = re.search(r"in this order:\s*\n(.*?)bytes is exactly", header, re.S).group(1)
    assert re.findall(r"\b(st|len|col|max_new|done|out|rnext|rpos|rlive|dlen|nstep|tabn|tab|hist)\b(?= ?[\[,(])", order.replace(" * ", " ")) == list(D.ARRAYS)
    from llmrankers import _engine
    assert _engine.DRAFT_ARRAYS == D.ARRAYS and len(D.ARRAYS) == 14
    steps, *_, max_admit, max_tokens = D.build_script(3, 4, (1, 3))
    rec = D.pack_script(steps, 3, 4, max_admit, max_tokens)
    assert rec.shape == (len(steps), 4 + 12 + 3 * 4 + 5 + max_tokens)
    a = rec[0]                                               # admit A: four rows, 12 + 600 + 4 + 1 tokens
    assert a[:4].tolist() == [1, 4, 0, 0] and a[16:28].tolist() == [0, 1, 3, 2, 12, 600, 4, 1, D.CAP, 20, 3, 3]
    assert a[28:33].tolist() == [0, 12, 612, 616, 617] and a[33:45].tolist() == [5, 6, 7] * 4


def test_the_machine_agrees_with_the_session_reference():
    """One slot alone against run_machine (the function the whole-session tests use): the same tokens, steps and accepted counts."""
    rs = np.random.RandomState(5)
    for kd, ngram, max_new in ((1, (1, 3), 12), (3, (2, 4), 20), (7, (1, 8), 24)):
        prompt = [int(t) for t in rs.choice(D.VOCAB, size=40)]
        plain = [int(t) for t in rs.choice(D.VOCAB, size=max_new - 1)] + [D.EOS[0]]
        for _ in range(3):                                   # a plain output that repeats parts of the prompt: drafts get accepted
            at, frm = rs.randint(0, max_new - 8), rs.randint(0, 30)
            plain[at:at + 6] = prompt[frm:frm + 6]
        want_out, want_steps, want_acc = D.run_machine(prompt, plain, kd, ngram, max_new, D.EOS, D.MAX_LEN, cap=D.CAP)
        m = D.DraftMachine(1, kd + 1, D.MAX_LEN, D.CAP, D.EOS, D.PAD, ngram)
        m.admit([0], [len(prompt)], [max_new], [prompt], [plain[0]])
        acc = []
        while not m.done[0]:
            c, dl = int(m.col[0]), int(m.dlen[0])
            assert m.rnext[0, 0] == plain[c - 1] and m.rpos[0, :dl + 1].tolist() == list(range(len(prompt) + c - 1, len(prompt) + c + dl))
            rows = [plain[c]]                                # row j saw the plain tokens iff the drafts in front of it were right
            for j in range(1, dl + 1):
                rows.append(plain[c + j] if int(m.rnext[0, j]) == rows[j - 1] and c + j < len(plain) else 97)
            m.step(rows + [98] * (kd - dl))
            acc.append(int(m.col[0]) - c)
        assert m.out[0, :m.col[0]].tolist() == want_out and int(m.nstep[0]) == want_steps and acc == want_acc
        assert sum(acc) > len(acc), "some draft was accepted"


@pytest.mark.parametrize("mut", D.MUTANTS)
def test_mutants_fail(mut):
    """A machine wrong in one way leaves the reference's states on the GPU test's own scripts (wherever the mutation can show: a
    range of one N has no order of N; g1 = 2 has one draft row)."""
    for S, g1, ng in CASES:
        if S != 3 or (mut == "lookup_nmin_first" and ng[0] == ng[1]):
            continue
        steps, init, states, *_ = D.build_script(S, g1, ng)
        got, _ = D.replay(steps, S, g1, ng, mut=mut)
        assert any(not np.array_equal(a, b) for gs, ws in zip(got, states) for a, b in zip(gs, ws)), (mut, g1, ng)
        same, _ = D.replay(steps, S, g1, ng)
        assert all(np.array_equal(a, b) for gs, ws in zip(same, states) for a, b in zip(gs, ws)), "the replay itself"
