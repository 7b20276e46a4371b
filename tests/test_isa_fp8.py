"""Compile-time guards on the FP8 weight-streaming kernel's gfx950 ISA (no GPU needed: hipcc cross-compiles; as tests/test_isa_guards.py).

gemm_skinny_fp8_kernel<EPI, NT> is gemm_skinny_kernel's text (csrc/gemm_skinny.inc) with the weight fragments converted from e4m3
bytes.  Held here: no scratch; no more VGPRs than the fp16 instantiation of the same (epilogue, NT) - 56 / 76 / 74 against 56 / 76 /
76 when this was written - so the same workgroups per CU; the conversions are the hardware's (v_cvt_pk_f32_fp8 -> v_cvt_pk_f16_f32 ->
v_pk_mul_f16 by 2^e), a step's worth per MFMA; the same MFMAs as the fp16 instantiation; the weights arrive as 16-byte loads."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "llm-rankers_amd", "csrc", "rk_engine.hip")
FORMS = [(0, 1), (1, 1), (5, 2)]          # (epilogue, NT): store f16, residual f32, SwiGLU f16


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_fp8") / "rk.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-w", SRC, "-o", str(out)], check=True, timeout=600)
    return out.read_text().split("\n")


def _kernel(lines, mangled):
    start = next(i for i, l in enumerate(lines) if l.startswith(mangled + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = [l.split(";")[0] for l in lines[start:end + 1]]
    vgprs = int(re.search(r"NumVgprs: (\d+)", "\n".join(lines[end:end + 400])).group(1))
    return body, vgprs


def _waves_per_simd(vgprs):
    return min(8, 512 // (-(-vgprs // 8) * 8))


@pytest.mark.parametrize("epi,nt", FORMS)
def test_fp8_weight_streaming_kernel(isa, epi, nt):
    body, vgprs = _kernel(isa, f"_Z22gemm_skinny_fp8_kernelILi{epi}ELi{nt}EEv8GemmArgs6GemmW8")
    ref, ref_vgprs = _kernel(isa, f"_Z18gemm_skinny_kernelILi{epi}ELi{nt}EEv8GemmArgs")
    print(f"epilogue {epi}: {vgprs} VGPRs (fp16 form {ref_vgprs}), {_waves_per_simd(vgprs)} waves per SIMD (fp16 form {_waves_per_simd(ref_vgprs)})")
    assert not any("scratch_" in l for l in body), "the FP8 weight-streaming kernel spills"
    assert not any("scratch_" in l for l in ref)
    n_mfma = sum("v_mfma_f32_32x32x16_f16" in l for l in body)
    assert n_mfma == sum("v_mfma_f32_32x32x16_f16" in l for l in ref) == 5 * nt       # four steps of the main loop + the tail's
    # a step's fragment = 8 weights: four paired conversions each way, four paired multiplies by 2^e
    assert sum("v_cvt_pk_f32_fp8" in l for l in body) == 4 * n_mfma
    assert sum("v_cvt_pk_f16_f32" in l for l in body) >= 4 * n_mfma
    assert sum("v_pk_mul_f16" in l for l in body) == 4 * n_mfma
    assert not any("v_cvt_pk_f32_fp8" in l for l in ref)
    # the main loop's bytes: two 16-byte pieces per weight tile (two K steps each), addressed by a 32-bit lane offset from a scalar base
    assert sum(bool(re.search(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]", l)) for l in body) >= 2 * nt
    assert vgprs <= ref_vgprs, f"the FP8 form takes {vgprs} VGPRs, the fp16 form {ref_vgprs}"
    assert _waves_per_simd(vgprs) == _waves_per_simd(ref_vgprs), (vgprs, ref_vgprs)
