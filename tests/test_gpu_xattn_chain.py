"""The decoder's query-side cross-attention chain - dec_cross_qk_kernel, the chunk kernel, dec_cross_cv_kernel, and the five-launch
form behind the same host function - against the stage-by-stage fp64 reference of tests/_attn_ref.py, through rk_debug_xattn_chain:
the call fills the engine's XAttnChain and runs run_xattn_chain as run_decoder does (the fuse decision, the q projection, the loop
over blocks of rows, plan_xattn per block), every buffer of the chain comes back whole, between sentinel bands.

Every case: the reported plan is the plan a Python mirror of plan_xattn and of the block rule gives (constants read from the
sources); the bands, the pad columns of ctx, the workspace rows behind a block's last row and the chunks a row does not have hold
what was put there (the part / stat workspaces are filled with +inf, so a chunk that is read without being the row's own turns the
row into NaN); a second run gives the same bytes; tier S is bit for bit and tier R within tolerance at the three stages (qk; the
merged partials; ctx - and xctx where the unfused merge writes it).  The shapes are the smallest that reach each code path of the
two kernels of decoder_kernels.h and of the block loop (SHAPES); the widths come from the call, not from the engine's checkpoint.

Every shape runs all four norm forms (rowscale, block sums with nb a multiple of 4 and not, none) at the default options, and its
rowscale form also with xattn_mfma = 0 and as the five-launch form (fuse_asked = 0), its nb = 8 form as the five-launch form too: the
norm form reaches the first kernel only.

RATIOS (largest (error - half ulp - flip) / E per kernel, tier R) are collected for the record (printed by the last test); they
are not bounds."""
import os
import re

import numpy as np
import pytest

import _attn_ref as A
from conftest import REPO, load_state
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu

BAND = 8
RATIOS = {}
ERR_INVALID, ERR_HIP, ERR_STATE = -1, -3, -4
FILL_BITS = 0x7F800000
_PROBLEMS = {}


def _src(name):
    return open(os.path.join(REPO, "llm-rankers_amd", "csrc", name)).read()


def _const(header, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, _src(header)).group(1))


XA_MAX_ROWS, XA_MAX_CHUNKS, DECV_MAXCH = _const("rk_engine.hip", "XA_MAX_ROWS"), _const("rk_engine.hip", "XA_MAX_CHUNKS"), _const("decoder_kernels.h", "DECV_MAXCH")
XRAW_SCALE = float(re.search(r"#define\s+RK_XRAW_SCALE\s+([0-9.]+)f", _src("rk_engine.hip")).group(1))
XA_KERNEL = ["xattn_part_mfma<few>", "xattn_part_mfma", "xattn_part<16>", "xattn_part<4>"]
DEFAULTS = {"xattn_mfma": 1, "dec_fuse_rows": 0}

SHAPES = A.CHAIN_SHAPES
NORMS = {"rowscale": ("rowscale", 0), "ssq8": ("ssq", 8), "ssq5": ("ssq", 5), "none": ("none", 0)}


@pytest.fixture(scope="module")
def t5(ckpt_dirs):
    from llmrankers._engine import RkEngine
    dims, state = load_state(ckpt_dirs["ckpt_gated_untied"])
    e = RkEngine(dims, device=0, max_tokens=2048, max_seqs=16, max_dec_len=8).load_state(state.items())
    plan = e.debug_xattn_chain(M=1, Ld=1, H=1, d=128, seq_off=[0, 1], plan_only=True)
    e.n_cu = plan["n_cu"]
    assert plan["eps"] == np.float32(A.EPS) and plan["xs"] == XRAW_SCALE == A.XS, "the fixtures' eps / xs are not the engine's"
    yield e
    e.close()


class Options:
    def __init__(self, eng, **kw):
        self.eng, self.kw, self.now = eng, kw, dict(DEFAULTS, **kw)

    def __enter__(self):
        for k, v in self.kw.items():
            self.eng.set_option(k, v)
        return self.now

    def __exit__(self, *exc):
        for k in self.kw:
            self.eng.set_option(k, DEFAULTS[k])


def problem(shape, norm, tier):
    """A problem and its reference are built once, shared by every option variant, and left unchanged."""
    key = (shape, norm, tier)
    if key not in _PROBLEMS:
        p = A.build_chain_shape(shape, *NORMS[norm], tier, band=BAND)
        p.cache = {}
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


# ---- Python mirror of run_xattn_chain's block rule and of plan_xattn (csrc/rk_engine.hip) --------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def mirror_plan(o, n_cu, fused, nr, maxL, H, d):
    nch = _cdiv(maxL, 64)
    qk_R, qk_CS = 32, 1
    if fused:
        if o["dec_fuse_rows"] > 0:
            qk_R = min(32, o["dec_fuse_rows"])
        elif nr <= 16:
            qk_R = 16
        while qk_CS < 8 and (d // 64) % (2 * qk_CS) == 0 and _cdiv(nr, qk_R) * H * qk_CS < n_cu // 2:
            qk_CS *= 2
    wgs16 = nch * nr * _cdiv(H, 16)
    if o["xattn_mfma"] and d % 256 == 0:
        part = 0 if wgs16 <= 2 * n_cu else 1
    else:
        part = 2 if wgs16 >= 2 * n_cu else 3
    fuse_cv, cv_R = fused and nch <= DECV_MAXCH, 16
    while fuse_cv and cv_R > 2 and _cdiv(nr, cv_R) * H < n_cu // 2:
        cv_R >>= 1
    return dict(qk_R=qk_R if fused else 0, qk_CS=qk_CS if fused else 0, part_kind=part, part_grid=(nch, nr, _cdiv(H, 4 if part == 3 else 16)),
                fuse_cv=int(fuse_cv), cv_R=cv_R if fuse_cv else 0)


def mirror_chain(o, n_cu, M, H, d, lens, fuse_asked):
    maxL = int(max(lens))
    nch = _cdiv(maxL, 64)
    blk = max(1, min(XA_MAX_ROWS, XA_MAX_CHUNKS // nch))
    nb = _cdiv(M, blk)
    fused = bool(fuse_asked) and d % 128 == 0
    first, last = (mirror_plan(o, n_cu, fused, min(blk, M - r0), maxL, H, d) for r0 in (0, (nb - 1) * blk))
    m = dict(fused=int(fused), block_rows=blk, n_blocks=nb, nch=nch)
    m.update({k: (first[k], last[k]) for k in first})
    return m


def call_args(p, rows=None):
    """The call of a problem, or of rows [a, b) of it as a call of their own (one position per sequence: row0 moves with them)."""
    a, b = (0, p.M) if rows is None else rows
    return dict(M=b - a, Ld=p.Ld, H=p.H, d=p.d, seq_off=p.seq_off, x=p.x[a:b], wq=p.wq, wk=p.wk, wv=p.wv, enc=p.enc, row0=p.row0 + a, row_seq=p.row_seq,
                rowscale=None if p.rowscale is None else p.rowscale[a:b], ssq_in=None if p.ssq is None else p.ssq[a:b], ctx=p.ctx0[a:b], ldo=p.ldo,
                band_rows=p.band, ws_fill=FILL_BITS)


def _all_sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == A.SENTINEL).all())


def _all_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == FILL_BITS).all())


def unpack(p, r, M, what):
    """The per-block workspaces put together as [M, nch, ...]; asserts every band and every workspace row no block owns."""
    B, H, d, Hd = p.band, p.H, p.d, p.H * p.d
    R, nb, nch = min(r["block_rows"], M), r["n_blocks"], r["nch"]
    parts, stats, xcs = [], [], []
    for k in range(nb):
        nr = min(r["block_rows"], M - k * r["block_rows"])
        pk, sk, xk = r["part"][k], r["stat"][k], r["xctx"][k]
        assert _all_sentinel(pk[:B * Hd]) and _all_sentinel(pk[-B * Hd:]), f"{what}: block {k}: a guard band of part was written"
        assert _all_sentinel(sk[:B * H * 2]) and _all_sentinel(sk[-B * H * 2:]), f"{what}: block {k}: a guard band of stat was written"
        assert _all_sentinel(xk[:B]) and _all_sentinel(xk[-B:]), f"{what}: block {k}: a guard band of xctx was written"
        pi, si, xi = pk[B * Hd:-B * Hd].reshape(R, nch, H, d), sk[B * H * 2:-B * H * 2].reshape(R, nch, H, 2), xk[B:-B]
        assert _all_fill(pi[nr:]) and _all_fill(si[nr:]) and _all_sentinel(xi[nr:]), f"{what}: block {k}: a workspace row behind the block's {nr} rows was written"
        merged_here = not r["fuse_cv"][0 if k == 0 else 1]
        assert merged_here or _all_sentinel(xi), f"{what}: block {k}: xctx was written although the merge is fused"
        parts.append(pi[:nr]); stats.append(si[:nr]); xcs.append(xi[:nr] if merged_here else None)
    assert _all_sentinel(r["qk"][:B]) and _all_sentinel(r["qk"][-B:]), f"{what}: a guard band of qk was written"
    assert _all_sentinel(r["ctx"][:B]) and _all_sentinel(r["ctx"][-B:]), f"{what}: a guard band of ctx was written"
    xctx = None if any(x is None for x in xcs) else np.concatenate(xcs)
    return dict(qk=r["qk"], part=np.concatenate(parts), stat=np.concatenate(stats), xctx=xctx, ctx=r["ctx"][B:-B], fill_bits=FILL_BITS)


def run_chain(eng, p, o, fuse_asked, what):
    """One problem under the options in force: plan == mirror, a second run the same bytes, everything not owned untouched, the three
    stages judged.  Returns (qk interior, ctx interior, plan)."""
    kw = call_args(p)
    plan = eng.debug_xattn_chain(plan_only=True, fuse_asked=fuse_asked, **kw)
    for k, v in mirror_chain(o, eng.n_cu, p.M, p.H, p.d, np.diff(p.seq_off), fuse_asked).items():
        assert plan[k] == v, f"{what}: plan field {k} = {plan[k]}, the shape should take {v} (plan {plan})"
    try:
        r1 = eng.debug_xattn_chain(fuse_asked=fuse_asked, **kw)
        r2 = eng.debug_xattn_chain(fuse_asked=fuse_asked, **kw)
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{what}: {err}", returncode=3)
        raise
    for k in ("qk", "part", "stat", "xctx", "ctx"):
        assert r1[k].tobytes() == r2[k].tobytes(), f"{what}: a second run gives other bytes in {k}"
    res = unpack(p, r1, p.M, what)
    ratios = A.judge_chain(p, res, what=what, cache=p.cache)
    names = {"A": "dec_cross_qk" if plan["fused"] else "cq + ckT GEMMs", "B": XA_KERNEL[plan["part_kind"][0]] + " (chain)",
             "C": "dec_cross_cv" if plan["fuse_cv"][0] else "W_v GEMM behind combine", "xctx": "xattn_combine (chain)"}
    for k, v in ratios.items():
        RATIOS[names[k]] = max(RATIOS.get(names[k], -1.0), v)
        print(f"{what}: stage {k} ratio {v:.2f}")
    return res["qk"][p.band:-p.band].tobytes(), res["ctx"].tobytes(), plan


@pytest.mark.parametrize("tier", ["S", "R"])
@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_chain(t5, shape, norm, tier):
    p = problem(shape, norm, tier)
    M, Ld, H, d = SHAPES[shape][:4]
    variants = [(dict(), True)]
    if norm == "rowscale":
        variants += [(dict(xattn_mfma=0), True), (dict(), False)]
    if norm == "ssq8":            # the five-launch form's q GEMM forming the row factors from the block sums itself
        variants += [(dict(), False)]
    if shape in ("row0", "tree"):
        assert p.Ld > 1           # several positions: the engine asks for the fused form here only under dec_fuse = 2, which is this call
    for opts, fuse_asked in variants:
        with Options(t5, **opts) as o:
            run_chain(t5, p, o, fuse_asked, f"chain {shape} M={M} Ld={Ld} H={H} d={d} {norm} tier {tier} {opts} fuse_asked={int(fuse_asked)}")


def test_plans_cover_both_kernels(t5):
    """From the reported plans of the parameter set above: every path of the two fused kernels and of the block loop that the shapes
    were chosen for is taken on the device at hand."""
    plans = []
    for shape, (M, Ld, H, d, lens, kw) in SHAPES.items():
        off = np.concatenate([[0], np.cumsum(lens)])
        plans.append((shape, d, t5.debug_xattn_chain(M=M, Ld=Ld, H=H, d=d, seq_off=off, row0=kw.get("row0", 0), row_seq=kw.get("row_seq"), plan_only=True)))
    blocks = [(d, pl, i) for _, d, pl in plans if pl["fused"] for i in (0, 1)]
    assert any(pl["qk_CS"][i] == 1 for d, pl, i in blocks) and any(pl["qk_CS"][i] > 1 for d, pl, i in blocks), "qk_CS 1 and > 1"
    assert any((d // 64) // pl["qk_CS"][i] > 8 for d, pl, i in blocks), "more than eight column pairs per workgroup (the second round of a wave)"
    fine = {pl["cv_R"][i] * _cdiv(_cdiv(d, 256), 4) < 8 for d, pl, i in blocks if pl["fuse_cv"][i]}
    assert fine == {True, False}, "both item shapes of the fused merge"
    assert {2, 16} <= {pl["cv_R"][i] for d, pl, i in blocks if pl["fuse_cv"][i]}, "cv_R of 2 and of 16"
    assert {0, 1} <= {pl["fuse_cv"][i] for d, pl, i in blocks}, "the fused merge and, beyond DECV_MAXCH chunks, the unfused pair behind the fused qk"
    assert any(pl["n_blocks"] > 1 for _, _, pl in plans) and any(pl["block_rows"] < XA_MAX_ROWS and pl["n_blocks"] > 1 for _, _, pl in plans), "more than one block, by rows and by chunks"
    kinds = {pl["part_kind"][i] for _, _, pl in plans for i in (0, 1)}
    assert kinds & {0, 1} and kinds & {2, 3}, "the MFMA and the VALU chunk kernels behind the fused qk"


@pytest.mark.parametrize("shape", ["setwise", "valu"])
def test_rows_per_workgroup_give_the_same_bits(t5, shape):
    """dec_fuse_rows (the slab of dec_cross_qk_kernel) is documented as 'same bits'."""
    p = problem(shape, "rowscale", "R")
    seen = {}
    for rows in (0, 1, 7, 16, 32):
        with Options(t5, dec_fuse_rows=rows) as o:
            seen[rows] = run_chain(t5, p, o, True, f"chain {shape} dec_fuse_rows={rows}")[:2]
    assert all(v == seen[0] for v in seen.values()), f"dec_fuse_rows changes the bytes: {[k for k, v in seen.items() if v != seen[0]]}"


def test_a_row_does_not_depend_on_its_slab_or_batch(t5):
    """decoder_kernels.h: 'a row's result does not depend on which rows share its slab, so neither on the batch nor on the rows per
    workgroup the host picks': row 40 of the 257-row call alone, in a 9-row call and in the full call - three different qk_R, qk_CS,
    cv_R and merge item shapes - has the same qk and ctx bytes."""
    p = problem("large", "rowscale", "R")
    B = p.band
    full = t5.debug_xattn_chain(**call_args(p))
    plans = [(full["qk_R"][0], full["qk_CS"][0], full["cv_R"][0])]
    for a, b in ((40, 41), (40, 49)):
        sub = t5.debug_xattn_chain(**call_args(p, (a, b)))
        plans.append((sub["qk_R"][0], sub["qk_CS"][0], sub["cv_R"][0]))
        assert sub["qk"][B:B + b - a].tobytes() == full["qk"][B + a:B + b].tobytes(), f"rows {a}..{b - 1} alone: other qk bytes than in the full call"
        assert sub["ctx"][B:B + b - a].tobytes() == full["ctx"][B + a:B + b].tobytes(), f"rows {a}..{b - 1} alone: other ctx bytes than in the full call"
    assert len({pl[1] for pl in plans}) >= 2 and len({pl[2] for pl in plans}) >= 2, f"the three calls took the same plan: {plans}"


def test_refusals(t5):
    """A shape outside the chain's contract: the documented status, and nothing launched - the outputs hold the sentinel."""
    p = problem("one-chunk", "rowscale", "R")

    def refused(code, **kw):
        args = dict(call_args(p), **kw)
        with pytest.raises(RkError) as ei:
            t5.debug_xattn_chain(**args)
        assert ei.value.code == code, ei.value
        assert all(_all_sentinel(v) for v in ei.value.outputs.values()), "a refused call wrote an output"

    w100 = np.zeros((128, 100), dtype=np.float16)
    refused(ERR_INVALID, d=100, x=np.zeros((1, 104), dtype=np.float16), wq=w100, wk=w100, wv=w100, enc=np.zeros((64 + 2 * BAND, 100), dtype=np.float16))
    refused(ERR_STATE, seq_off=[0, 65537], enc=np.zeros((65537 + 2 * BAND, 128), dtype=np.float16))
    refused(ERR_INVALID, row0=1)                                              # row 1 of a one-sequence call: sequence 1 of 1
    refused(ERR_INVALID, row_seq=[0, 3], row0=1)                              # row_seq names sequence 3
    refused(ERR_INVALID, row_seq=[0], row0=1)                                 # row_seq shorter than the rows read
    refused(ERR_INVALID, enc=p.enc[:-1])                                      # the call reaches beyond enc
    refused(ERR_INVALID, x=p.x[:, :120])                                      # ldx < d
    # d % 128 != 0 with the fused form asked for: the five-launch form, reported
    off = [0, 5]
    plan = t5.debug_xattn_chain(M=1, Ld=1, H=2, d=160, seq_off=off, fuse_asked=True, plan_only=True)
    assert plan["fused"] == 0 and plan["qk_R"] == (0, 0) and plan["fuse_cv"] == (0, 0)


def test_zz_report_ratios():
    for k in sorted(RATIOS):
        print("chain ratio %-32s %.2f" % (k, RATIOS[k]))
