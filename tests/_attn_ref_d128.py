"""fp64 reference, fixtures and tolerance model of the T5 encoder self-attention with 128-WIDE heads (csrc/attention_d128.h; t5-3b),
and the stage references of the decoder's query-side chain at that width.  Everything that does not depend on the head width is
tests/_attn_ref.py's (attend64, emulate_item, the sample, the half ulp, the selector, the spike table, the sentinel, C and C_CHAIN);
what is written here is the ONE thing that does: how a call is cut into (sequence, head) pieces.

  P = softmax(Q K^T + lut[h, clamp(j - i, +-128)]), ctx = P V per sequence and head, no scaling; the packed rows hold q | k | v at
  columns 0 | I | 2I with I = 128 H, head h at columns 128 h .. 128 h + 128 of each.

Tolerance: half an fp16 ulp of the expected value + C E, C = 3 as for every other attention test, E = the largest error against fp64
of the chain emulation (fp32 k-ordered scores, exp2, probabilities rounded to fp16, one fp32 P V chain, one division) on the fixed
sample of the problem's rows.  Measured on the CPU with N(0, 1) and flat operands at lengths 1 to 300, in units of E: the honest
orders - the chain itself, online softmax per 32, 64 and 128 keys, a 64-key flash merge - stay at or below 1.21 at width 128 (1.08
at width 64); tests/test_attn_ref_d128_host.py recomputes the figure on this module's own fixtures (1.26 there) and fails above C.

The chain (rk_debug_xattn_chain on a 128-wide engine): wq / wk / wv are [128 H, d]; q_h = rowfactor (W_q,h x), qk_h = W_k,h^T q_h,
ctx' = the softmax-weighted sum of the raw encoder rows (width d: no head width in it), ctx_h = W_v,h ctx'.  Stages A / B / C as in
_attn_ref.judge_chain, with the per-head slices 128 wide."""
import numpy as np

import _attn_ref as A
from _attn_ref import C, C_CHAIN, LUT_N, LUT_R, SENTINEL, f16, f32, f64   # noqa: F401  (re-exported for the tests)

HD = 128
ENC = A.ENC


def items(p, mut=None):
    """The (sequence, head) pieces of a 128-wide encoder call (the dicts of _attn_ref.items).  Mutants: "stride64" (heads 64 columns
    apart), "bias_head" (another head's table row), "drop_last" (the last key missing), "next_seq" (the neighbour's first key admitted)."""
    B, H, out = p.band, p.H, []
    I, hs = HD * H, (64 if mut == "stride64" else HD)
    for b in range(p.n_seq):
        rows = np.arange(B + p.seq_off[b], B + p.seq_off[b + 1])
        lo, hi = B + p.seq_off[b], B + p.seq_off[b + 1]
        hi += (mut == "next_seq") - (mut == "drop_last")
        keys = np.arange(lo, max(hi, lo + 1))
        for h in range(H):
            c = h * hs
            out.append(dict(q=p.q[rows, c:c + HD], k=p.q[keys, I + c:I + c + HD], v=p.q[keys, 2 * I + c:2 * I + c + HD],
                            bias=A._lut_bias(p.lut, h, rows, keys, mut), mask=None, scale=1.0, out_rows=rows - B, out_col=h * HD, p16=True))
    return out


def expected64(p, mut=None):
    """fp64 context rows [out rows, ldctx], NaN where the call writes nothing."""
    out = np.full((p.out_rows, p.ldctx), np.nan)
    for it in items(p, mut):
        out[it["out_rows"], it["out_col"]:it["out_col"] + HD] = A.attend64(it)
    return out


def emulated(p, order="chain", tile=64, mut=None):
    """What a kernel of the documented arithmetic returns: fp16 [out rows, ldctx] over the pre-filled output."""
    out = p.out.copy()
    for it in items(p, mut):
        out[it["out_rows"], it["out_col"]:it["out_col"] + HD] = A.f16_sat(A.emulate_item(it, order, tile))
    return out


def yardstick(p):
    """E of the problem: the chain emulation's largest error against fp64 on the fixed sample (computed once per problem)."""
    if getattr(p, "_E128", None) is None:
        worst = 0.0
        for it in items(p):
            rows = A._sample(it["q"].shape[0])
            worst = max(worst, float(np.abs(A.emulate_item(it, rows=rows).astype(f64) - A.attend64(it)[rows]).max()))
        p._E128 = worst
    return p._E128


def judge(p, got, what=""):
    """_attn_ref.judge for a 128-wide encoder problem: exact rows bit for bit, the others within half an fp16 ulp + C E, everything
    the call does not own untouched.  Returns the largest (error - half ulp) / E (0.0 for a wholly exact problem)."""
    if getattr(p, "_want128", None) is None:
        p._want128 = expected64(p)
    want = p._want128
    written = ~np.isnan(want)
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == f16
    stale = ~written & (got.view(np.uint16) != p.out.view(np.uint16))
    assert not stale.any(), f"{what}: output element {tuple(np.argwhere(stale)[0])} is not the call's to write"
    assert np.isfinite(got[written].astype(f64)).all(), f"{what}: non-finite output"
    all_exact = p.tier == "S" and p.exact is None
    E = None if all_exact else yardstick(p)
    ratio = 0.0
    for n, it in enumerate(items(p)):
        r, c0 = it["out_rows"], it["out_col"]
        g, x = got[r, c0:c0 + HD], want[r, c0:c0 + HD]
        ex = np.ones(len(r), dtype=bool) if all_exact else (p.exact[r, c0 // HD] if p.exact is not None else np.zeros(len(r), dtype=bool))
        if ex.any():
            bad = g[ex].view(np.uint16) != A.f16_sat(x[ex]).view(np.uint16)
            if bad.any():
                i, j = np.argwhere(bad)[0]
                raise AssertionError(f"{what}: piece {n} (head column {c0}), output row {r[ex][i]}, column {c0 + j}: got {g[ex][i, j]}, the selected row has {x[ex][i, j]}")
        if (~ex).any():
            err = np.abs(g[~ex].astype(f64) - x[~ex])
            over = err - A.half_ulp16(x[~ex])
            ratio = max(ratio, float(over.max()) / E if E > 0 else 0.0)
            if (over > C * E).any():
                i, j = np.argwhere(over > C * E)[0]
                raise AssertionError(f"{what}: piece {n} (head column {c0}), output row {r[~ex][i]}, column {c0 + j}: got {g[~ex][i, j]}, fp64 {x[~ex][i, j]:.6g}, "
                                     f"error {err[i, j]:.3g} > half ulp {A.half_ulp16(x[~ex][i, j]):.3g} + {C} x E ({E:.3g})")
    return ratio


def build_enc(seed, H, lens, tier, band=8, pad=(0, 0), spike=None, flat=False):
    """_attn_ref.build_enc at head width 128.  tier "S": selector (winners at the first and the last key and on both sides of every
    32-key edge, a trap in the row before and in the row behind every sequence); spike: the bias-only case."""
    rs = np.random.RandomState(seed)
    I, off = HD * H, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, ldq, ldctx = int(off[-1]), 3 * I + pad[0], I + pad[1]
    q = A._rows_buffer(rs, T, ldq, band, tier)
    p = A.problem(ENC, H=H, n_seq=len(lens), seq_off=off, band=band, ldq=ldq, ldctx=ldctx, out_rows=T, tier=tier, p16=True)
    if tier == "S" and spike is None:
        p.lut = np.zeros((H, LUT_N), dtype=f32)
        q[:, 2 * I:3 * I] = A._int_values(rs, (T + 2 * band, I))
        for h in range(H):
            queries, traps = [], []
            for b, L in enumerate(lens):
                adm, sp = range(band + off[b], band + off[b + 1]), [band + off[b] + k for k in A.edges_of(L)]
                for i in range(L):
                    queries.append((adm, A._prefer(rs, adm, sp[h % len(sp):] + sp[:h % len(sp)], i)))
                traps += [(len(queries) - L + (h % L), adm.start - 1), (len(queries) - 1 - (h % L), adm.stop)]
            K, win, placed = A.selector(rs, T + 2 * band, HD, 4, queries, traps, what=f"enc128 head {h}")
            p.n_traps += len(placed)
            q[:, I + h * HD:I + h * HD + HD] = K
            q[band:band + T, h * HD:h * HD + HD] = K[win]
    elif tier == "S":
        p.lut = A.spike_lut(H, spike)
        q[:, :I] = 0
        q[:, 2 * I:3 * I] = A._int_values(rs, (T + 2 * band, I))
        p.exact = np.zeros((T, H), dtype=bool)
        for b, L in enumerate(lens):
            for h in range(H):
                p.exact[off[b]:off[b + 1], h] = A._spike_exact(p.lut, h, np.arange(L), L, False)
    else:
        p.lut = (2.0 * rs.standard_normal((H, LUT_N))).astype(f32)
        if flat:
            q[:, :I] = (q[:, :I].astype(f32) / 16).astype(f16)
    p.q, p.out = q, A.sentinel16((T, ldctx))
    return p


def alone(p, b):
    """Sequence b of the problem as a call of its own: the same rows (its neighbours become band rows), the same table."""
    lo, hi = int(p.seq_off[b]), int(p.seq_off[b + 1])
    s = A.problem(ENC, H=p.H, n_seq=1, seq_off=np.array([0, hi - lo], dtype=np.int32), band=p.band, ldq=p.ldq, ldctx=p.ldctx, out_rows=hi - lo,
                  tier=p.tier, p16=True, lut=p.lut)
    s.q = np.ascontiguousarray(p.q[lo:hi + 2 * p.band])
    s.out = A.sentinel16((hi - lo, p.ldctx))
    return s


# ---- the query-side chain at head width 128 ----------------------------------------------------------------------------------
# _attn_ref's chain problem, stage references and judge with the per-head slices 128 wide.  What does not see the head width is
# _attn_ref's own and is called, not copied: the row -> sequence map, the row factors, stage B (scores, softmax and weighted sums
# over raw encoder rows of the model's width: chain_ctxp64, chain_merge64, emul_merge, the XATTN yardstick), the sample, the
# flip window and the two comparison rules.  Tier R only: the selector needs disjoint column supports per head (128 H <= d), which
# the shapes of this test (H = 3, d = 128) do not have; which key, which head and which mask are the encoder test's and the 64-wide
# chain test's business, the head STRIDE is what a random operand catches here (test_attn_ref_d128_host.py: mutants).
def _heads(w, H):
    return w.reshape(H, HD, -1)


def build_chain(seed, M, Ld, H, d, lens, *, norm="rowscale", row0=0, row_seq=None, band=8, ldx_pad=0, ldo_pad=0):
    """One tier-R call of rk_debug_xattn_chain on a 128-wide engine: _attn_ref.build_chain's operands with wq / wk / wv [128 H, d]
    (its generator is asked for 2 H heads of 64: the same N(0, 1 / d) rows) and ldo = 128 H + pad."""
    p = A.build_chain(seed, M, Ld, 2 * H, d, lens, "R", norm=norm, row0=row0, row_seq=row_seq, band=band, ldx_pad=ldx_pad, ldo_pad=ldo_pad)
    p.H = H
    return p


def chain_qk64(p, mut=None):
    """Stage A in fp64: q [M, H, 128] before its rounding, qk [M, H, d] from the fp16-rounded q.  mut "stride64": heads 64 rows apart."""
    wq, wk = _heads(p.wq.astype(f64), p.H), _heads(p.wk.astype(f64), p.H)
    if mut == "stride64":
        wq = np.stack([p.wq[h * 64:h * 64 + HD].astype(f64) for h in range(p.H)])
        wk = np.stack([p.wk[h * 64:h * 64 + HD].astype(f64) for h in range(p.H)])
    q = A.chain_factor(p)[:, None, None] * np.einsum("hjc,mc->mhj", wq, p.x[:, :p.d].astype(f64))
    return q, np.einsum("hjc,mhj->mhc", wk, A.f16_sat(q).astype(f64))


def chain_ctx64(p, merged):
    """Stage C's product in fp64 from the fp16-rounded merged sums: [M, 128 H]."""
    return np.einsum("hnc,mhc->mhn", _heads(p.wv.astype(f64), p.H), A.f16_sat(merged).astype(f64)).reshape(p.M, HD * p.H)


def emul_q(p, rows):
    y = np.stack([A._dot32(_heads(p.wq, p.H)[h], p.x[rows, :p.d]) for h in range(p.H)], axis=1)
    return (y * A.chain_factor(p, None, f32)[rows, None, None]).astype(f32)


def emul_qk(p, q16):
    """qk [R, H, d] in fp32 before its rounding, from fp16 q [R, H, 128]: one chain over the 128 products."""
    wk = _heads(p.wk, p.H)
    return np.stack([A._chain(q16[:, h].astype(f32)[:, :, None] * wk[h].astype(f32)[None], 1) for h in range(p.H)], axis=1)


def emul_ctx(p, s16):
    return np.concatenate([A._dot32(_heads(p.wv, p.H)[h], s16[:, h]) for h in range(p.H)], axis=1)


def emulated_chain(p, mut=None):
    """What the five-launch form returns when kernels of the documented arithmetic run it (qk with sentinel bands, part, stat, ctx)."""
    rows = np.arange(p.M)
    if mut == "stride64":
        q64, qk64 = chain_qk64(p, mut)
        qk_in = A.f16_sat(qk64)
    else:
        qk_in = A.f16_sat(emul_qk(p, A.f16_sat(emul_q(p, rows))))
    qk = A.sentinel16((p.M + 2 * p.band, p.H, p.d))
    qk[p.band:p.band + p.M] = qk_in
    part, stat = A.emul_part(p, qk[p.band:p.band + p.M])
    merged32 = A.emul_merge(p, part, stat, rows)
    ctx = p.ctx0.copy()
    ctx[:, :HD * p.H] = A.f16_sat(emul_ctx(p, A.f16_sat(merged32)))
    return dict(qk=qk, part=part, stat=stat, xctx=A.f16_sat(merged32).reshape(p.M, -1), ctx=ctx)


def judge_chain(p, res, what=""):
    """_attn_ref.judge_chain's tier-R rules for a 128-wide chain result: chunks beyond a row's own never written, pad columns
    untouched, stages A / B / C each against fp64 of its own inputs as the device left them, within half an fp16 ulp + C_CHAIN E +
    flip.  Returns the largest ratios per stage."""
    H, d, M, B = p.H, p.d, p.M, p.band
    rows = A.chain_sample(p)
    qk = np.asarray(res["qk"])[B:B + M]
    part, stat, ctx = res["part"], res["stat"], np.asarray(res["ctx"])
    nv, nch = A.chain_nv(p), part.shape[1]
    dead = np.arange(nch)[None, :] >= nv[:, None]
    fill = res.get("fill_bits", A.WS_FILL.view(np.uint32))
    assert (part.view(np.uint32)[dead] == fill).all(), f"{what}: partial sums of a chunk beyond a row's own were written"
    mark = np.array(A.EMPTY_CHUNK, dtype=f32).view(np.uint32)
    assert (stat.view(np.uint32)[dead] == mark).all(), f"{what}: the statistics of a chunk beyond a row's own are not the chunk kernel's empty mark"
    assert np.isfinite(part[~dead]).all() and np.isfinite(stat[~dead]).all(), f"{what}: a chunk of a row was not written (or not finite)"
    assert ctx[:, HD * H:].tobytes() == p.ctx0[:, HD * H:].tobytes(), f"{what}: a pad column of ctx was written"
    ratios = {}
    # stage A
    q64, wantA = chain_qk64(p)
    Eq = float(np.abs(emul_q(p, rows).astype(f64) - q64[rows]).max())
    EA = float(np.abs(emul_qk(p, A.f16_sat(q64[rows])).astype(f64) - wantA[rows]).max())
    flipA = A._amb_flip(q64, Eq, np.abs(_heads(p.wk.astype(f64), H)).transpose(0, 2, 1))
    ratios["A"] = A._within(qk, wantA, EA, flipA, f"{what}: stage A (qk)")
    # stage B: from the device's qk bytes
    wantB = A.chain_ctxp64(p, qk)
    EB = A.yardstick(A.chain_xattn_problem(p, qk, rows))[True]
    merged = A.chain_merge64(p, part, stat)
    assert np.isfinite(merged).all(), f"{what}: stage B: non-finite merge of the partials"
    ratios["B"] = A._within(merged, wantB, EB, 0.0, f"{what}: stage B (merged partials)", half=False)
    # stage C: from the device's part / stat bytes
    wantC = chain_ctx64(p, merged)
    Em = float(np.abs(A.emul_merge(p, part, stat, rows).astype(f64) - merged[rows]).max())
    EC = float(np.abs(emul_ctx(p, A.f16_sat(merged[rows])).astype(f64) - wantC[rows]).max())
    flipC = A._amb_flip(merged, Em, np.abs(_heads(p.wv.astype(f64), H))).reshape(M, HD * H)
    if res.get("xctx") is not None:
        ratios["xctx"] = A._within(np.asarray(res["xctx"]).reshape(M, H, d), merged, Em, 0.0, f"{what}: xctx")
    ratios["C"] = A._within(ctx[:, :HD * H], wantC, EC, flipC, f"{what}: stage C (ctx)")
    return ratios
