"""csrc/debug_bands.h on the CPU: the one owner of the guard bands of the rk_debug_* entry points.  A stand-alone C++ program (its
own main, built with -Wall -Werror and the address / undefined-behaviour sanitizers, run as a plain executable) prints, for a set
of (bytes, band) pairs, the total, the interior's offset and the verdict of the rule an rk_debug_rows_out must keep; the assertions
here are the formulas written out from the stated contract (include/rk_engine.h at rk_debug_rows), not read back from the header:
  allocation  [band | bytes | band]: total = bytes + 2 band, the interior starts at band
  row form    bands of band_rows rows of ld elements of elt bytes around n elements
  rule        interior and all present; 64 <= band <= 2^26, band a multiple of 16; then the call's own comparison of bytes with
              the need: rk_debug_rows need <= bytes <= 2^31, rk_debug_draft_steps need == bytes"""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

# (bytes, band, need, interior present, all present)
CASES = [(0, 64, 0, 1, 1), (1, 64, 1, 1, 1), (4096, 64, 4096, 1, 1), (4096, 1 << 26, 4096, 1, 1), (4096, 256, 1000, 1, 1),
         (4096, 48, 4096, 1, 1), (4096, 72, 4096, 1, 1), (4096, (1 << 26) + 16, 4096, 1, 1), (4096, 32, 4096, 1, 1),
         (4096, 64, 4096, 0, 1), (4096, 64, 4096, 1, 0), (4096, 64, 4100, 1, 1), (4096, 64, 4092, 1, 1),
         ((1 << 31) + 16, 64, 16, 1, 1), (1 << 31, 64, 16, 1, 1)]
ROW_FORMS = [(1000, 256, 40, 2), (7, 8, 1024, 4), (0, 1, 64, 2)]          # (n elements, band_rows, ld, elt bytes)

PROGRAM = r"""
#include "debug_bands.h"
#include <cstdio>
int main() {
  static char here[1];
  const long long cases[][5] = {%(cases)s};
  for (const auto& c : cases) {
    const BandSpan s{(size_t)c[0], (size_t)c[1]};
    const rk_debug_rows_out b{c[3] ? here : nullptr, (int64_t)c[0], (int64_t)c[1], c[4] ? here : nullptr};
    printf("case %%zu %%zu %%d %%d\n", s.all(), s.interior(), (int)band_out_ok(b, c[2], BAND_AT_LEAST), (int)band_out_ok(b, c[2], BAND_EXACT));
  }
  const long long rows[][4] = {%(rows)s};
  for (const auto& r : rows) {
    const BandSpan s = band_rows_span((size_t)r[0], (size_t)r[1], (size_t)r[2], (size_t)r[3]);
    printf("rows %%zu %%zu %%zu %%zu\n", s.bytes, s.band, s.all(), s.interior());
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("debug_bands")
    braces = lambda rows: ", ".join("{" + ", ".join(f"{x}LL" for x in r) + "}" for r in rows)   # noqa: E731
    src = tmp / "bands.cpp"
    src.write_text(PROGRAM % dict(cases=braces(CASES), rows=braces(ROW_FORMS)))
    exe = tmp / "bands"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "llm-rankers_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    cases = [[int(x) for x in line.split()[1:]] for line in out if line.startswith("case")]
    rows = [[int(x) for x in line.split()[1:]] for line in out if line.startswith("rows")]
    assert len(cases) == len(CASES) and len(rows) == len(ROW_FORMS)
    return dict(zip(CASES, cases)), dict(zip(ROW_FORMS, rows))


def _band_ok(band, interior, all_):
    return bool(interior) and bool(all_) and 64 <= band <= 2 ** 26 and band % 16 == 0


@pytest.mark.parametrize("case", CASES)
def test_band_arithmetic_and_rule(printed, case):
    nbytes, band, need, interior, all_ = case
    total, at, rows_ok, draft_ok = printed[0][case]
    assert (total, at) == (nbytes + 2 * band, band)
    assert rows_ok == int(_band_ok(band, interior, all_) and need <= nbytes <= 2 ** 31)      # rk_debug_rows: out_need[i] > bytes refuses
    assert draft_ok == int(_band_ok(band, interior, all_) and need == nbytes)                 # rk_debug_draft_steps: need[i] * 4 != bytes refuses


def test_the_cases_the_contract_names(printed):
    """accepted and refused, by name: the verdicts as plain numbers, so that a change of CASES cannot quietly drop one"""
    verdict = {c: tuple(v[2:]) for c, v in printed[0].items()}
    for c in [(0, 64, 0, 1, 1), (1, 64, 1, 1, 1), (4096, 64, 4096, 1, 1), (4096, 1 << 26, 4096, 1, 1)]:
        assert verdict[c] == (1, 1), c
    for c in [(4096, 48, 4096, 1, 1), (4096, 72, 4096, 1, 1), (4096, (1 << 26) + 16, 4096, 1, 1), (4096, 64, 4096, 0, 1), (4096, 64, 4096, 1, 0)]:
        assert verdict[c] == (0, 0), c
    assert verdict[(4096, 64, 4100, 1, 1)] == (0, 0)          # bytes below need: both forms refuse
    assert verdict[(4096, 64, 4092, 1, 1)] == (1, 0)          # bytes above need: the rows form takes it, the draft form wants equality
    assert verdict[(4096, 256, 1000, 1, 1)] == (1, 0)
    assert verdict[(1 << 31, 64, 16, 1, 1)] == (1, 0) and verdict[((1 << 31) + 16, 64, 16, 1, 1)] == (0, 0)


@pytest.mark.parametrize("form", ROW_FORMS)
def test_row_form(printed, form):
    n, band_rows, ld, elt = form
    assert printed[1][form] == [n * elt, band_rows * ld * elt, n * elt + 2 * band_rows * ld * elt, band_rows * ld * elt]
