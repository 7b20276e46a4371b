"""csrc/decode_ints.h on the CPU: the one owner of the Llama decoders' device int block.  A stand-alone C++ program (its own main,
built with -Wall -Werror and the address / undefined-behaviour sanitizers, run as a plain executable) prints, for a set of shapes,
every array's offset and length, the total and the initial() vector; the assertions here are formulas written out from the stated
layout, not read back from the header:
  generate  head[16] | len[S] | done[S] | pos[S] | next[S] | out[n_seq][max_new]                       (S = max_seqs)
  session   head[16] | len | col | max_new | done | pos | next [S each] | admit[3 S] | out[S][cap]
            and with draft = Kd > 0, R = S (Kd + 1):  | rnext[R] | rpos[R] | rlive[R] | dlen[S] | nstep[S] | tabn[S] | tab[S][cap] | hist[S][max_len]
  head      generate {n, finished, pad, n_eos, max_new, max_total, P, 0}, session {finishes, pad, n_eos, max_len, cap, ngram_min,
            ngram_max, 0}, then eos[8]"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

SESSIONS = [(1, 1, 2, 0), (3, 5, 7, 0), (3, 5, 7, 7), (257, 16, 304, 3)]     # (n_slots, cap, max_len, draft)
GENERATES = [(16, 1, 1), (16, 3, 40)]                                      # (S, n_seq, max_new)
EOS, PAD, NGRAM, MAX_TOTAL, P = (7, 9, 11), 5, (2, 4), 77, 123
SES_ARRAYS = ("len", "col", "max_new", "done", "pos", "next", "admit", "out", "rnext", "rpos", "rlive", "dlen", "nstep", "tabn", "tab", "hist")
GEN_ARRAYS = ("len", "done", "pos", "next", "out")

PROGRAM = r"""
#include "decode_ints.h"
#include <cstdio>
static void span(const char* name, const IntSpan& a) { printf("%%s %%zu %%zu\n", name, a.off, a.n); }
static void vec(const std::vector<int>& v) { printf("init"); for (int x : v) printf(" %%d", x); printf("\n"); }
int main() {
  const int eos[3] = {%(eos)s};
  printf("words %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", INTS_EOS0, INTS_HEAD, GEN_N, GEN_FINISHED, GEN_PAD, GEN_N_EOS,
         GEN_MAX_NEW, GEN_MAX_TOTAL, GEN_P, SES_FINISHES, SES_PAD, SES_N_EOS, SES_MAX_LEN, SES_CAP, SES_NGRAM_MIN, SES_NGRAM_MAX);
  const int ses[][4] = {%(sessions)s};
  for (const auto& s : ses) {
    const SessionLayout L(s[0], s[1], s[2], s[3]);
    printf("session %%d %%d %%d %%d\n", s[0], s[1], s[2], s[3]);
%(ses_spans)s
    printf("total %%zu\n", L.total);
    vec(L.initial(eos, 3, %(pad)d, %(nmin)d, %(nmax)d));
    std::vector<int> block(L.total);                       // bind: every pointer inside the block, at its offset
    const SessionInts d = L.bind(block.data());
    printf("bound %%td %%td %%td %%d\n", d.len - d.st, d.out - d.st, d.hist ? d.hist - d.st : 0, d.rnext == nullptr);
  }
  const int gen[][3] = {%(generates)s};
  for (const auto& g : gen) {
    const GenLayout L(g[0], g[1], g[2]);
    printf("generate %%d %%d %%d\n", g[0], g[1], g[2]);
%(gen_spans)s
    printf("total %%zu\n", L.total);
    std::vector<int> off(g[1] + 1, 0);                     // prompt b: 10 + b tokens
    for (int b = 0; b < g[1]; ++b) off[b + 1] = off[b] + 10 + b;
    vec(L.initial(off.data(), %(max_total)d, %(P)d, eos, 3, %(pad)d));
    std::vector<int> block(L.total);
    const GenInts d = L.bind(block.data());
    printf("bound %%td %%td %%td %%d\n", d.len - d.st, d.out - d.st, d.next - d.st, 0);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("decode_ints")
    braces = lambda rows: ", ".join("{" + ", ".join(str(x) for x in r) + "}" for r in rows)   # noqa: E731
    src = tmp / "layout.cpp"
    src.write_text(PROGRAM % dict(eos=", ".join(map(str, EOS)), pad=PAD, nmin=NGRAM[0], nmax=NGRAM[1], max_total=MAX_TOTAL, P=P,
                                  sessions=braces(SESSIONS), generates=braces(GENERATES),
                                  ses_spans="\n".join(f'    span("{a}", L.{a});' for a in SES_ARRAYS),
                                  gen_spans="\n".join(f'    span("{a}", L.{a});' for a in GEN_ARRAYS)))
    exe = tmp / "layout"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "llm-rankers_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    blocks, words = {}, None
    for line in out:
        key, *rest = line.split()
        if key == "words":
            words = [int(x) for x in rest]
        elif key in ("session", "generate"):
            cur = blocks[(key,) + tuple(int(x) for x in rest)] = {"spans": {}}
        elif key in ("total", "init", "bound"):
            cur[key] = [int(x) for x in rest]
        else:
            cur["spans"][key] = (int(rest[0]), int(rest[1]))
    return words, blocks


def _contiguous(spans, want):
    """the arrays named in `want` = [(name, length)], in that order, one behind the other from int 16 on -> the end"""
    at = 16
    for name, n in want:
        assert spans[name] == (at, n), (name, spans[name], at, n)
        at += n
    return at


def test_header_words_keep_their_indices(printed):
    words, _ = printed
    assert words == [8, 16] + [0, 1, 2, 3, 4, 5, 6] + [0, 1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("shape", SESSIONS)
def test_session_block(printed, shape):
    S, cap, max_len, draft = shape
    b = printed[1][("session",) + shape]
    R = S * (draft + 1)
    plain = [(a, S) for a in SES_ARRAYS[:6]] + [("admit", 3 * S), ("out", S * cap)]
    extra = [("rnext", R), ("rpos", R), ("rlive", R), ("dlen", S), ("nstep", S), ("tabn", S), ("tab", S * cap), ("hist", S * max_len)]
    end = _contiguous(b["spans"], plain + (extra if draft else []))
    total = 16 + 9 * S + S * cap
    if draft:
        total += 3 * S * (draft + 1) + 3 * S + S * cap + S * max_len
    else:
        assert all(b["spans"][a][1] == 0 for a, _ in extra)           # not there
    assert b["total"] == [total] and end == total
    want = np.zeros(total, dtype=np.int64)
    want[1:5] = PAD, len(EOS), max_len, cap
    want[8:8 + len(EOS)] = EOS
    want[16 + 3 * S:16 + 4 * S] = 1                                   # done
    want[16 + 5 * S:16 + 6 * S] = PAD                                 # next
    want[16 + 9 * S:16 + 9 * S + S * cap] = PAD                       # out
    if draft:
        want[5:7] = NGRAM
        x = 16 + 9 * S + S * cap
        want[x:x + R] = PAD                                           # rnext; rpos stays 0
        want[x + 2 * R:x + 3 * R:draft + 1] = 1                       # rlive: row 0 of each slot
        want[x + 3 * R + 2 * S:x + 3 * R + 3 * S] = -1                # tabn; dlen and nstep stay 0
        want[x + 3 * R + 3 * S:] = PAD                                # tab, hist
    np.testing.assert_array_equal(np.array(b["init"]), want)
    assert b["bound"] == [16, 16 + 9 * S, total - S * max_len if draft else 0, int(not draft)]


@pytest.mark.parametrize("shape", GENERATES)
def test_generate_block(printed, shape):
    S, n_seq, max_new = shape
    b = printed[1][("generate",) + shape]
    end = _contiguous(b["spans"], [(a, S) for a in GEN_ARRAYS[:4]] + [("out", n_seq * max_new)])
    total = 16 + 4 * S + n_seq * max_new
    assert b["total"] == [total] and end == total
    want = np.zeros(total, dtype=np.int64)
    want[2:7] = PAD, len(EOS), max_new, MAX_TOTAL, P
    want[8:8 + len(EOS)] = EOS
    want[16:16 + n_seq] = 10 + np.arange(n_seq)                       # len; done, pos, next stay 0
    want[16 + 4 * S:] = PAD
    np.testing.assert_array_equal(np.array(b["init"]), want)
    assert b["bound"] == [16, 16 + 4 * S, 16 + 3 * S, 0]
