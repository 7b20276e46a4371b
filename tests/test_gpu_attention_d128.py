"""The 128-wide encoder self-attention (csrc/attention_d128.h) against the fp64 reference of tests/_attn_ref_d128.py, through
rk_debug_attn kind 1 on a 128-wide engine: the call goes through plan_enc_attn and launch_enc_attn as run_encoder's does.

Tier S: selector operands (winners at the first and the last key and on both sides of every 32-key edge, traps in the row before and
behind every sequence) and the bias-only spike case - bit for bit.  Tier R: N(0, 1) and flat operands - within half an fp16 ulp +
C E.  Every case: guard bands and unowned columns untouched, a second run the same bytes, every sequence computed alone the same
bytes as inside its ragged batch, and the plan is the 128-wide kind whatever attn_short / attn_long say."""
import os
import re

import numpy as np
import pytest

import _attn_ref_d128 as D
from conftest import REPO
from llmrankers import _synth
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu

BAND = 8
ERR_HIP, ERR_STATE = -3, -4
KIND_D128 = 3                       # EncAttnPlan::Kind: DMA 0, LONG 1, TILED 2, D128 3
RATIOS = {}


def _const(header, name):
    src = open(os.path.join(REPO, "llm-rankers_amd", "csrc", header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


NW = _const("attention_d128.h", "ATT128_NW")
KSTR, VSTR = _const("attention_d128.h", "ATT128_KSTR"), _const("attention_d128.h", "ATT128_VSTR")
LDS = 2 * 64 * KSTR * 2 + 2 * 128 * VSTR * 2 + (D.LUT_N + 3) * 4


@pytest.fixture(scope="module")
def eng():
    from llmrankers._engine import RkEngine
    dims = _synth.TOY_MONOT5_D128
    e = RkEngine(dims, device=0, max_tokens=2048, max_seqs=16, max_dec_len=8).load_state(_synth.synth_state_dict(dims, seed=7, gain=1.0).items())
    yield e
    e.close()


def _args(p):
    return dict(n_seq=p.n_seq, H=p.H, q=p.q, out=p.out, band_rows=p.band, ldq=p.ldq, ldctx=p.ldctx, seq_off=p.seq_off, bias_lut=p.lut)


def _run(eng, p, what):
    try:
        return eng.debug_attn(D.ENC, **_args(p))["out"]
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{what}: {err}", returncode=3)
        raise


def _sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == D.SENTINEL).all())


def run_case(eng, p, what):
    lens = np.diff(p.seq_off)
    plan = eng.debug_attn(D.ENC, plan_only=True, **_args(p))
    want = dict(kind=KIND_D128, tparam=NW, grid=(-(-int(lens.max()) // (32 * NW)), p.H, p.n_seq), lds=LDS)
    for k, v in want.items():
        assert plan[k] == v, f"{what}: plan field {k} = {plan[k]}, the shape should take {v}"
    assert LDS <= 160 * 1024 // 2
    out = _run(eng, p, what)
    assert out.tobytes() == _run(eng, p, what).tobytes(), f"{what}: a second run gives other bytes"
    assert _sentinel(out[:p.band]) and _sentinel(out[-p.band:]), f"{what}: a guard band of the output was written"
    inner = out[p.band:-p.band]
    r = D.judge(p, inner, what=what)
    RATIOS[what] = r
    print(f"{what}: ratio {r:.2f}")
    if p.n_seq > 1:                              # a sequence's bytes depend on its own tokens and length only
        for b in range(p.n_seq):
            s = D.alone(p, b)
            solo = _run(eng, s, f"{what} sequence {b} alone")[s.band:-s.band]
            lo, hi = int(p.seq_off[b]), int(p.seq_off[b + 1])
            assert solo.tobytes() == inner[lo:hi].tobytes(), f"{what}: sequence {b} alone gives other bytes than inside the batch"
    return inner.tobytes()


TIERS = {"S": dict(tier="S"), "spike": dict(tier="S", spike=[5, -7, 128, -128, 1, -1]), "R": dict(tier="R"), "Rflat": dict(tier="R", flat=True)}
BATCHES = [[1], [2, 1, 3], [63, 64, 65], [127, 129], [31, 200, 1, 64], [513]]


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("lens", BATCHES, ids=lambda v: "-".join(map(str, v)))
def test_encoder_d128(eng, H, lens):
    for n, (tname, kw) in enumerate(TIERS.items()):
        pad = (64, 8) if (n + H) % 2 else (0, 0)
        p = D.build_enc(300 + 10 * BATCHES.index(lens) + n, H, lens, band=BAND, pad=pad, **kw)
        bits = run_case(eng, p, f"enc128 H={H} {lens} {tname} pad={pad}")
        if tname == "R":                         # attn_short / attn_long choose between 64-wide kernels: not this plan's business
            for short, long_ in ((0, 1), (6, 0), (0, 0)):
                eng.set_option("attn_short", short)
                eng.set_option("attn_long", long_)
                try:
                    plan = eng.debug_attn(D.ENC, plan_only=True, **_args(p))
                    assert plan["kind"] == KIND_D128, (short, long_, plan)
                    got = _run(eng, p, "options")[p.band:-p.band].tobytes()
                finally:
                    eng.set_option("attn_short", 5)
                    eng.set_option("attn_long", 1)
                assert got == bits, f"attn_short={short} attn_long={long_} changed the bytes of a 128-wide call"


def test_decoder_kinds_are_refused(eng):
    """kind 2 (the 64-wide decoder kernels) on a 128-wide engine: RK_ERR_STATE, nothing launched"""
    q = np.zeros((2 * BAND + 2, 3 * 128), dtype=np.float16)
    out = D.A.sentinel16((2, 128))
    with pytest.raises(RkError) as ei:
        eng.debug_attn(2, n_seq=1, H=1, q=q, out=out, band_rows=BAND, Ld=2, ldq=3 * 128, ldctx=128, k_col=128, v_col=256)
    assert ei.value.code == ERR_STATE and "d_kv=128" in str(ei.value)


def test_query_side_kind_is_unchanged(eng):
    """kind 3 (the chunk kernel and the merge over raw encoder rows of the model's width) does not see the head width"""
    A = D.A
    for tier in ("S", "R"):
        p = A.build_xattn(77, 3, 128, 7, 1, [1, 64, 65, 200], tier, row_seq=[(3 * i) % 4 for i in range(7)], band=BAND)
        kw = dict(n_seq=p.n_seq, H=p.H, q=p.q, out=p.out, kv=p.kv, band_rows=p.band, Ld=p.Ld, M=p.M, row0=p.row0, d=p.d, ldq=p.ldq, ldkv=p.ldkv,
                  ldctx=p.ldctx, seq_off=p.seq_off, row_seq=p.row_seq)
        out = eng.debug_attn(A.XATTN, **kw)["out"]
        assert _sentinel(out[:p.band]) and _sentinel(out[-p.band:])
        A.judge(p, out[p.band:-p.band], what=f"query-side kind on a 128-wide engine, tier {tier}")


def test_zz_ratios():
    print("largest (error - half ulp) / E, tier R:", max([0.0] + [r for k, r in RATIOS.items() if " R" in k]))
