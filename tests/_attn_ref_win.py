"""The sliding window on top of the fp64 attention references: tests/_attn_ref.py (128-wide heads) and tests/_attn_ref_hd64.py
(64-wide) cut a Llama call into (sequence or row, head) pieces; here every piece loses the keys below its window - in the prefill
(kind 4) query row i keeps keys max(0, i - W + 1) .. i, in the cached step (kind 5) the row at pos keeps the last W of its pos + 1
keys - and is then judged by those modules' own rule: within half an fp16 ulp of the fp64 value + C E, E = the chain emulation's
largest error against fp64 on the fixed sample of the problem's rows, C the modules' (3, fixed on the CPU).  Tier R problems only:
the selector designs of tier S place their winners without regard to a window.  `mod` is one of the two modules."""
import numpy as np

import _attn_ref as A


def items(mod, p, W, emul=False):
    out = []
    for it in mod.items(p, None, emul):
        it = dict(it)
        if p.kind == A.LLAMA:
            nq, nk = it["mask"].shape
            it["mask"] = it["mask"] & (np.arange(nk)[None, :] >= np.arange(nq)[:, None] - W + 1)
        else:
            assert it["mask"] is None
            it["k"], it["v"] = it["k"][-W:], it["v"][-W:]
        out.append(it)
    return out


def expected64(mod, p, W):
    out = np.full((p.out_rows, p.ldctx), np.nan)
    for it in items(mod, p, W):
        out[it["out_rows"], it["out_col"]:it["out_col"] + it["v"].shape[1]] = A.attend64(it)
    return out


def yardstick(mod, p, W):
    """E per probability format of the pieces ({p16: E})"""
    E = {}
    for ref, em in zip(items(mod, p, W), items(mod, p, W, emul=True)):
        rows = A._sample(em["q"].shape[0])
        e = float(np.abs(A.emulate_item(em, rows=rows).astype(A.f64) - A.attend64(ref)[rows]).max())
        E[em["p16"]] = max(E.get(em["p16"], 0.0), e)
    return E


def judge(mod, p, W, got, what=""):
    """`got` [out rows, ldctx] fp16, the interior of a windowed kernel's output -> the largest (error - half ulp) / E"""
    assert p.tier == "R"
    want, E = expected64(mod, p, W), yardstick(mod, p, W)
    written = ~np.isnan(want)
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == A.f16
    stale = ~written & (got.view(np.uint16) != p.out.view(np.uint16))
    assert not stale.any(), f"{what}: output element {tuple(np.argwhere(stale)[0])} is not the call's to write"
    assert np.isfinite(got[written].astype(A.f64)).all(), f"{what}: non-finite output"
    worst = 0.0
    for n, it in enumerate(items(mod, p, W)):
        r, c0, w, e = it["out_rows"], it["out_col"], it["v"].shape[1], E[it["p16"]]
        err = np.abs(got[r, c0:c0 + w].astype(A.f64) - want[r, c0:c0 + w])
        over = err - A.half_ulp16(want[r, c0:c0 + w])
        if (over > A.C * e).any():
            i, j = np.argwhere(over > A.C * e)[0]
            raise AssertionError(f"{what}: piece {n} (head column {c0}), output row {r[i]}, column {c0 + j}: got {got[r[i], c0 + j]}, fp64 "
                                 f"{want[r[i], c0 + j]:.6g}, error {err[i, j]:.3g} > half ulp + {A.C} x E ({e:.3g})")
        worst = max(worst, float(over.max()) / e if e > 0 else 0.0)
    return worst


def alone(p, b):
    """Sequence b of a prefill problem as a call of its own: the same rows (its neighbours become band rows)."""
    lo, hi = int(p.seq_off[b]), int(p.seq_off[b + 1])
    s = A.problem(A.LLAMA, H=p.H, n_kv=p.n_kv, n_seq=1, seq_off=np.array([0, hi - lo], dtype=np.int32), band=p.band, ldq=p.ldq, ldctx=p.ldctx,
                  out_rows=hi - lo, tier=p.tier, p16=p.p16)
    s.q = np.ascontiguousarray(p.q[lo:hi + 2 * p.band])
    s.out = A.sentinel16((hi - lo, p.ldctx))
    return s
