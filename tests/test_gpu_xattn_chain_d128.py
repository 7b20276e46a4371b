"""The decoder's query-side cross-attention chain on a 128-WIDE engine (wq / wk / wv [128 H, d]) against the stage-by-stage fp64
reference of tests/_attn_ref_d128.py, through rk_debug_xattn_chain: the call fills the engine's XAttnChain with the engine's head
width and runs run_xattn_chain as run_decoder does.  The fused kernels (dec_cross_qk_kernel, dec_cross_cv_kernel) are built for
64-wide heads: a 128-wide engine always runs the five-launch form, also when the caller asks for the fused one.

Every case: out_fused == 0 with fuse_asked = 1; the bands, the pad columns of ctx, the workspace rows behind a block's last row and
the chunks a row does not have hold what was put there (part / stat are filled with +inf); a second run gives the same bytes;
fuse_asked = 0 gives the same bytes; stages A (qk), B (merged partials), xctx and C (ctx) within half an fp16 ulp + C_CHAIN E + flip."""
import numpy as np
import pytest

import _attn_ref_d128 as D
from llmrankers import _synth
from llmrankers._engine import RkError

A = D.A
pytestmark = pytest.mark.gpu

BAND = 8
ERR_HIP = -3
FILL_BITS = 0x7F800000
LENS = [1, 64, 65, 200]
H, DM = 3, 128
# name -> (M, Ld, extra builder arguments): one row, a setwise-sized pass, more rows than sequences; row0 and row_seq variants
SHAPES = {
    "M1": (1, 1, {}),
    "M13-row_seq": (13, 1, dict(row_seq=[(5 * i + i // 3) % 4 for i in range(13)], ldo_pad=8)),
    "M40-row_seq": (40, 1, dict(row_seq=[(3 * i + i // 7) % 4 for i in range(40)])),
    "M13-row0": (13, 4, dict(row0=2, ldx_pad=8)),                              # rows 2 .. 14 at four positions per sequence: sequences 0 .. 3
    "M13-row0-row_seq": (13, 2, dict(row0=3, row_seq=[(7 * i + i // 5) % 4 for i in range(16)], ldo_pad=8)),
}
RATIOS = {}


@pytest.fixture(scope="module")
def eng():
    from llmrankers._engine import RkEngine
    dims = _synth.TOY_MONOT5_D128
    e = RkEngine(dims, device=0, max_tokens=2048, max_seqs=16, max_dec_len=8).load_state(_synth.synth_state_dict(dims, seed=7, gain=1.0).items())
    plan = e.debug_xattn_chain(M=1, Ld=1, H=1, d=128, seq_off=[0, 1], plan_only=True)
    assert plan["eps"] == np.float32(A.EPS) and plan["xs"] == A.XS, "the fixtures' eps / xs are not the engine's"
    yield e
    e.close()


def call_args(p):
    return dict(M=p.M, Ld=p.Ld, H=p.H, d=p.d, seq_off=p.seq_off, x=p.x, wq=p.wq, wk=p.wk, wv=p.wv, enc=p.enc, row0=p.row0, row_seq=p.row_seq,
                rowscale=p.rowscale, ssq_in=p.ssq, ctx=p.ctx0, ldo=p.ldo, band_rows=p.band, ws_fill=FILL_BITS)


def _sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == A.SENTINEL).all())


def _fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == FILL_BITS).all())


def unpack(p, r, what):
    """The one block's workspaces as [M, nch, ...]; asserts every band and every workspace row the block does not own."""
    B, Hd = p.band, p.H * p.d
    assert r["n_blocks"] == 1 and r["block_rows"] >= p.M
    R, nch = min(r["block_rows"], p.M), r["nch"]
    pk, sk, xk = r["part"][0], r["stat"][0], r["xctx"][0]
    assert _sentinel(pk[:B * Hd]) and _sentinel(pk[-B * Hd:]), f"{what}: a guard band of part was written"
    assert _sentinel(sk[:B * p.H * 2]) and _sentinel(sk[-B * p.H * 2:]), f"{what}: a guard band of stat was written"
    assert _sentinel(xk[:B]) and _sentinel(xk[-B:]), f"{what}: a guard band of xctx was written"
    assert _sentinel(r["qk"][:B]) and _sentinel(r["qk"][-B:]), f"{what}: a guard band of qk was written"
    assert _sentinel(r["ctx"][:B]) and _sentinel(r["ctx"][-B:]), f"{what}: a guard band of ctx was written"
    return dict(qk=r["qk"], part=pk[B * Hd:-B * Hd].reshape(R, nch, p.H, p.d), stat=sk[B * p.H * 2:-B * p.H * 2].reshape(R, nch, p.H, 2),
                xctx=xk[B:-B], ctx=r["ctx"][B:-B], fill_bits=FILL_BITS)


def _call(eng, p, fuse_asked, what):
    try:
        return eng.debug_xattn_chain(fuse_asked=fuse_asked, **call_args(p))
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{what}: {err}", returncode=3)
        raise


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("norm", ["rowscale", "none"])
def test_chain_d128(eng, shape, norm):
    M, Ld, kw = SHAPES[shape]
    p = D.build_chain(900 + sorted(SHAPES).index(shape), M, Ld, H, DM, LENS, norm=norm, band=BAND, **kw)
    assert p.wq.shape == (128 * H, DM) and p.ldo >= 128 * H
    what = f"chain128 {shape} {norm}"
    plan = eng.debug_xattn_chain(plan_only=True, fuse_asked=True, **call_args(p))
    assert plan["fused"] == 0 and plan["qk_R"] == (0, 0) and plan["fuse_cv"] == (0, 0), f"{what}: a 128-wide engine planned a fused kernel: {plan}"
    r1 = _call(eng, p, True, what)
    assert r1["fused"] == 0
    res = unpack(p, r1, what)
    for k, v in unpack(p, _call(eng, p, True, what), what + " (second run)").items():
        assert k == "fill_bits" or np.asarray(v).tobytes() == np.asarray(res[k]).tobytes(), f"{what}: a second run gives other bytes in {k}"
    for k, v in unpack(p, _call(eng, p, False, what), what + " (fuse_asked = 0)").items():
        assert k == "fill_bits" or np.asarray(v).tobytes() == np.asarray(res[k]).tobytes(), f"{what}: fuse_asked = 0 gives other bytes in {k}"
    ratios = D.judge_chain(p, res, what)
    for k, v in ratios.items():
        RATIOS[k] = max(RATIOS.get(k, -1e9), v)
    print(f"{what}: ratios {ratios}")


def test_zz_ratios():
    print("chain at head width 128, largest (error - half ulp - flip) / E per stage:", {k: round(v, 2) for k, v in RATIOS.items()})
