"""The 64-wide Llama attention kernels (csrc/llama_kernels_hd64.h) against the fp64 reference of tests/_attn_ref_hd64.py, through
rk_debug_attn kinds 4 and 5 on a 64-wide engine: the calls go through plan_llama_attn / launch_llama_attn and plan_llama_dec_attn /
launch_llama_dec_attn as llama_prefill's and llama_step_rows' do.

Tier S: selector operands and traps - bit for bit.  Tier R (N(0, 1)) and R-flat (queries / 16): within half an fp16 ulp + C E, C = 3
fixed on the CPU (tests/test_attn_ref_hd64_host.py).  Every case: the plan fields, guard bands and unowned columns untouched, a second
run the same bytes, every sequence (row) computed alone the same bytes as inside its batch (call).  The options that choose between
128-wide kernels (llama_attn_dma, llama_attn_nw) change neither the plan kind nor a byte; llama_dec_r 0 and 1 give the same bytes.
The cached step: exactly row pos of K and of V of every kv head is written and equals the reference's rotated key and value.

Measured on an MI355X, largest (error - half ulp) / E in tier R: the figures test_zz_ratios prints (DESIGN.md section 3 quotes them).

The module stops at the first device error: nothing more is started on a device that has faulted."""
import os
import re

import numpy as np
import pytest

import _attn_ref_hd64 as D
from conftest import REPO
from llmrankers import _synth
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu

BAND = 8
ERR_HIP = -3
KIND_HD64 = 2                       # rk_debug_attn kind 4: out_kind 0 / 1 = the 128-wide kernels, 2 = attn_causal_tile_kernel<64>
RATIOS = {}
HEADS = [(4, 2), (7, 1), (3, 3)]


def _const(header, name):
    src = open(os.path.join(REPO, "llm-rankers_amd", "csrc", header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


KSTR, VSTR, LDC_CHUNK = _const("llama_kernels_hd64.h", "ATC64_KSTR"), _const("llama_kernels_hd64.h", "ATC64_VSTR"), _const("llama_kernels.h", "LDC_CHUNK")
LDS = (64 * KSTR + 64 * VSTR) * 2


@pytest.fixture(scope="module")
def eng():
    from llmrankers._engine import RkLlamaEngine
    dims = _synth.TOY_LLAMA_HD64
    e = RkLlamaEngine(dims, device=0, max_tokens=2048, max_seqs=16).load_state(_synth.synth_state_dict(dims, seed=929).items())
    yield e
    e.close()


def _run(eng, kind, kw, what):
    try:
        return eng.debug_attn(kind, **kw)
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{what}: {err}", returncode=3)
        raise


def _sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == D.SENTINEL).all())


def _cdiv(a, b):
    return -(-a // b)


# ---- prefill (kind 4) ----------------------------------------------------------------------------------------------------------
def _pargs(p):
    return dict(n_seq=p.n_seq, H=p.H, n_kv=p.n_kv, q=p.q, out=p.out, band_rows=p.band, ldq=p.ldq, ldctx=p.ldctx, seq_off=p.seq_off)


def run_prefill(eng, p, what):
    lens = np.diff(p.seq_off)
    plan = eng.debug_attn(D.LLAMA, plan_only=True, **_pargs(p))
    want = dict(kind=KIND_HD64, tparam=0, grid=(_cdiv(int(lens.max()), 128), p.H, p.n_seq), lds=LDS)
    for k, v in want.items():
        assert plan[k] == v, f"{what}: plan field {k} = {plan[k]}, the shape should take {v}"
    out = _run(eng, D.LLAMA, _pargs(p), what)["out"]
    assert out.tobytes() == _run(eng, D.LLAMA, _pargs(p), what)["out"].tobytes(), f"{what}: a second run gives other bytes"
    assert _sentinel(out[:p.band]) and _sentinel(out[-p.band:]), f"{what}: a guard band of the output was written"
    inner = out[p.band:-p.band]
    r = D.judge(p, inner, what=what)
    RATIOS[what] = r
    print(f"{what}: ratio {r:.2f}")
    if p.n_seq > 1:                              # a sequence's bytes depend on its own tokens and length only
        for b in range(p.n_seq):
            s = D.alone(p, b)
            solo = _run(eng, D.LLAMA, _pargs(s), f"{what} sequence {b} alone")["out"][s.band:-s.band]
            lo, hi = int(p.seq_off[b]), int(p.seq_off[b + 1])
            assert solo.tobytes() == inner[lo:hi].tobytes(), f"{what}: sequence {b} alone gives other bytes than inside the batch"
    return inner.tobytes()


TIERS = {"S": dict(tier="S"), "R": dict(tier="R"), "Rflat": dict(tier="R", flat=True)}
BATCHES = [[1], [2, 1, 3], [63, 64, 65], [127, 129], [31, 200, 1, 64], [513]]


@pytest.mark.parametrize("heads", HEADS, ids=lambda v: f"{v[0]}on{v[1]}")
@pytest.mark.parametrize("lens", BATCHES, ids=lambda v: "-".join(map(str, v)))
def test_prefill_hd64(eng, heads, lens):
    H, n_kv = heads
    for n, (tname, kw) in enumerate(TIERS.items()):
        pad = (8, 64) if (n + H) % 2 else (0, 0)      # a padded ldq / ldctx variant of every shape and tier across the cases
        p = D.build_llama(900 + 10 * BATCHES.index(lens) + n, H, n_kv, lens, band=BAND, pad=pad, **kw)
        bits = run_prefill(eng, p, f"prefill64 {H}/{n_kv} {lens} {tname} pad={pad}")
        if tname == "R":                         # llama_attn_dma / llama_attn_nw choose between 128-wide kernels: not this plan's business
            for dma, nw in ((0, 0), (1, 4), (1, 8), (0, 8)):
                eng.set_option("llama_attn_dma", dma)
                eng.set_option("llama_attn_nw", nw)
                try:
                    plan = eng.debug_attn(D.LLAMA, plan_only=True, **_pargs(p))
                    assert plan["kind"] == KIND_HD64 and plan["lds"] == LDS, (dma, nw, plan)
                    got = _run(eng, D.LLAMA, _pargs(p), "options")["out"][p.band:-p.band].tobytes()
                finally:
                    eng.set_option("llama_attn_dma", 1)
                    eng.set_option("llama_attn_nw", 0)
                assert got == bits, f"llama_attn_dma={dma} llama_attn_nw={nw} changed the bytes of a 64-wide call"


# ---- cached step (kind 5) ------------------------------------------------------------------------------------------------------
P = 400                             # four chunks of LDC_CHUNK keys
STEP_POS = [0, 1, 2, 63, 64, 126, 127, 128, 129, 255, 256, 383, 398]


def _sargs(p):
    return dict(n_seq=p.n_seq, H=p.H, n_kv=p.n_kv, q=p.q, out=p.out, band_rows=p.band, P=p.P, ldq=p.ldq, ldctx=p.ldctx, pos=p.pos, cos=p.cos,
                sin=p.sin, qkv_bias=p.qkv_bias, cache=p.cache)


def run_step(eng, p, r_opt, what):
    G = p.H // p.n_kv
    R = 1 if r_opt == 1 else (8 if G % 8 == 0 else 4 if G % 4 == 0 else 2 if G % 2 == 0 else 1)
    nch = _cdiv(p.P, LDC_CHUNK)
    plan = eng.debug_attn(D.STEP, plan_only=True, **_sargs(p))
    want = dict(R=R, nch=nch, tparam=R, grid=(nch, p.H // R, p.n_seq), grid2=(p.H, p.n_seq, 1))
    for k, v in want.items():
        assert plan[k] == v, f"{what}: plan field {k} = {plan[k]}, the shape should take {v}"
    r1, r2 = _run(eng, D.STEP, _sargs(p), what), _run(eng, D.STEP, _sargs(p), what)
    out, c1, cb = r1["out"], r1["cache"], p.band * D.HD
    assert out.tobytes() == r2["out"].tobytes() and c1.tobytes() == r2["cache"].tobytes(), f"{what}: a second run gives other bytes"
    assert _sentinel(out[:p.band]) and _sentinel(out[-p.band:]), f"{what}: a guard band of the output was written"
    assert _sentinel(c1[:cb]) and _sentinel(c1[-cb:]), f"{what}: a guard band of the cache was written"
    r = D.judge(p, out[p.band:-p.band], what=what)
    D.judge_cache(p, c1[cb:-cb], what)
    RATIOS[what] = r
    print(f"{what}: ratio {r:.2f}")
    return out[p.band:-p.band], c1[cb:-cb]


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("heads", HEADS, ids=lambda v: f"{v[0]}on{v[1]}")
def test_step_hd64(eng, heads, bias):
    H, n_kv = heads
    assert _cdiv(P, LDC_CHUNK) == 4
    for n, tname in enumerate(("S", "R")):
        p = D.build_step(950 + 10 * HEADS.index(heads) + 2 * n + bias, H, n_kv, STEP_POS, P, tname, bias=bias, band=BAND)
        res = {}
        for r_opt in (0, 1, 2):                  # 2: no R = 7 instantiation at this width - the rule
            eng.set_option("llama_dec_r", r_opt)
            try:
                res[r_opt] = run_step(eng, p, r_opt, f"step64 {H}/{n_kv} bias={bias} {tname} llama_dec_r={r_opt}")
            finally:
                eng.set_option("llama_dec_r", 0)
        for r_opt in (1, 2):
            assert res[r_opt][0].tobytes() == res[0][0].tobytes() and res[r_opt][1].tobytes() == res[0][1].tobytes(), \
                f"step64 {H}/{n_kv} bias={bias} {tname}: llama_dec_r 0 and {r_opt} are documented as the same bytes and differ"
        out, cache = res[0]
        kc, vc = D.step_cache_views(p, cache)
        for b in range(p.n_seq):                 # a row alone gives the same bytes as inside the call
            s = D.row_alone(p, b)
            what = f"step64 {H}/{n_kv} bias={bias} {tname} row {b} (pos {int(p.pos[b])}) alone"
            r = _run(eng, D.STEP, _sargs(s), what)
            assert r["out"][s.band:-s.band].tobytes() == out[b:b + 1].tobytes(), f"{what}: other bytes than inside the call"
            skc, svc = D.step_cache_views(s, r["cache"][s.band * D.HD:-s.band * D.HD])
            assert skc.tobytes() == kc[b:b + 1].tobytes() and svc.tobytes() == vc[b:b + 1].tobytes(), f"{what}: another cache than inside the call"


def test_step_key_equals_the_prefill_key(eng):
    """the key a step writes is bit for bit the key the prefill's rotary kernel writes for that token: both call rope64_pairs.  Checked
    end to end where both run: tests/test_gpu_llama_hd64.py (tokens of generate == the greedy1 re-prefill loop, the session); here
    the step's appended key against the reference's fp32 form of that arithmetic, bit for bit in tier S."""
    p = D.build_step(990, 4, 2, [0, 5, 128], P, "S", bias=True, band=BAND)
    _, cache = run_step(eng, p, 0, "step64 appended key, tier S")
    assert cache.tobytes() == D.emulated_cache(p).tobytes()


def test_zz_ratios():
    pre = max([0.0] + [r for k, r in RATIOS.items() if k.startswith("prefill64") and (" R " in k or " Rflat " in k)])
    st = max([0.0] + [r for k, r in RATIOS.items() if k.startswith("step64") and " R " in k])
    print(f"largest (error - half ulp) / E, tier R: attn_causal64 {pre:.2f}, attn_dec_cached<64> + combine {st:.2f} (C = {D.C})")
