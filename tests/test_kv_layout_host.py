"""csrc/kv_layout.h on the CPU: the one owner of a layer's layout in the Llama decoders' K / V cache.  A stand-alone C++ program (its
own main, built with -Wall -Werror and the address / undefined-behaviour sanitizers, run as a plain executable) prints, for a set
of shapes, every region's offset, the layer's size and pe; the assertions here are formulas written out from the stated layout,
not read back from the header (all in bytes from the layer's start):
  mode 0 (fp16) and 2 (dequantised fp16 values)   K [rows][n_kv][P][head_dim] fp16 | V                           no exponents, pe = 0
  mode 1 (FP8 bytes)                              K bytes [rows][n_kv][P][head_dim] | V bytes | K exponents [rows][n_kv][pe] int8 |
                                                  V exponents,   pe = P rounded up to 32
Every region starts on a multiple of 32 bytes - in every layer of a cache whose layers lie back to back - and no two overlap."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

# (rows, n_kv, head_dim, P): P a multiple of 32 and not, 1 and below 32; rows 1 and more; both head widths (mode 1 is 128 wide only)
SHAPES = [(1, 1, 128, 1), (1, 2, 128, 32), (3, 2, 128, 33), (8, 4, 128, 304), (5, 8, 128, 4096), (1, 1, 64, 1), (3, 2, 64, 33), (7, 4, 64, 300)]
CASES = [(m,) + s for s in SHAPES for m in (0, 1, 2) if m != 1 or s[2] == 128]

PROGRAM = r"""
#include "kv_layout.h"
#include <cstdio>
static_assert(kv_layer_layout(1, 3, 2, 128, 33).pe == 64, "a constant expression");
int main() {
  const int cases[][5] = {%(cases)s};
  for (const auto& c : cases) {
    const KvLayerLayout L = kv_layer_layout(c[0], c[1], c[2], c[3], c[4]);
    printf("%%d %%d %%d %%d %%d : %%zu %%zu %%zu %%zu %%zu %%d\n", c[0], c[1], c[2], c[3], c[4], L.k, L.v, L.ke, L.ve, L.bytes, L.pe);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("kv_layout")
    src, exe = tmp / "layout.cpp", tmp / "layout"
    src.write_text(PROGRAM % dict(cases=", ".join("{" + ", ".join(map(str, c)) + "}" for c in CASES)))
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "llm-rankers_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, val = line.split(":")
        out[tuple(int(x) for x in key.split())] = dict(zip(("k", "v", "ke", "ve", "bytes", "pe"), (int(x) for x in val.split())))
    assert sorted(out) == sorted(CASES)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "m%d-r%d-kv%d-d%d-P%d" % c)
def test_layer(printed, case):
    mode, rows, n_kv, hd, P = case
    L = printed[case]
    if mode == 1:
        pe = -(-P // 32) * 32
        plane, eplane = rows * n_kv * P * hd, rows * n_kv * pe                # one byte a value, one an exponent
        regions = [(0, plane), (plane, plane), (2 * plane, eplane), (2 * plane + eplane, eplane)]
        assert (L["k"], L["v"], L["ke"], L["ve"], L["pe"]) == (0, plane, 2 * plane, 2 * plane + eplane, pe)
        assert pe >= P and pe % 32 == 0 and pe - P < 32
    else:
        plane = rows * n_kv * P * hd * 2                                      # fp16
        regions = [(0, plane), (plane, plane)]
        assert (L["k"], L["v"], L["ke"], L["ve"], L["pe"]) == (0, plane, 0, 0, 0)
    total = sum(n for _, n in regions)
    assert L["bytes"] == total
    # back to back from 0 to the end: inside the layer, none overlapping; 32-byte aligned in every layer (layer l starts at l * bytes)
    at = 0
    for off, n in regions:
        assert off == at and n > 0, (regions, at)
        at += n
    assert at == total
    assert all(off % 32 == 0 for off, _ in regions) and total % 32 == 0, regions


def test_fp8_layer_against_the_fp16_layer(printed):
    """the byte layout of P = 4096 is (128 + 1) / 256 of the fp16 layout; modes 0 and 2 are one layout"""
    assert printed[(1, 5, 8, 128, 4096)]["bytes"] * 256 == printed[(0, 5, 8, 128, 4096)]["bytes"] * 129
    for s in SHAPES:
        assert printed[(0,) + s] == printed[(2,) + s]
