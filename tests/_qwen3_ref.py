"""Test-side Qwen3 references: the fp32 numpy oracle with the q / k head norm, outlier norm weights, an oracle-backed runtime double
with LlamaRuntime's `generate`, and the fp64 restatement of the norm-and-rotate arithmetic the two kernels share."""
from types import SimpleNamespace

import numpy as np

import _attn_ref as A
import _rows_ref as R
from oracle.llama_numpy import LlamaOracle
from _llama_gen_stub import OracleLlamaGenRuntime

f16, f32, f64 = np.float16, np.float32, np.float64


class Qwen3Oracle(LlamaOracle):
    """hf: models/qwen3/modeling_qwen3.py: the Llama forward with an RMSNorm over head_dim on every query and key head
    (Qwen3Attention.q_norm / k_norm), behind the projection and in front of the rotation.  A norm weight missing from the state is a
    norm left out (what tests drop to show what a bound is worth)."""

    def _lin(self, x, name):
        y = x @ self.w[name].T
        mod = name.split(".")[-2]
        if mod not in ("q_proj", "k_proj"):
            return y
        w = self.w.get(name[:-len("q_proj.weight")] + mod[0] + "_norm.weight")
        if w is None:
            return y
        hd = self.d.head_dim
        h = y.reshape(y.shape[0], -1, hd).astype(np.float32)
        var = np.mean(h * h, axis=-1, keepdims=True)
        return (w * (h * (1.0 / np.sqrt(var + np.float32(self.d.eps))))).reshape(y.shape).astype(np.float32)


OUTLIER_NORM_CH, OUTLIER_NORM_GAIN = (3, 41, 77, 100), 20.0


def with_norm_outliers(state):
    """Real Qwen3 checkpoints carry a few q_norm / k_norm channels far above the rest: 4 channels of every q_norm and k_norm weight
    x 20 (fp16-representable, like every synthetic value).  Returns a new dict."""
    out = dict(state)
    for name, w in state.items():
        if name.endswith("q_norm.weight") or name.endswith("k_norm.weight"):
            w = np.array(w, dtype=np.float32, copy=True)
            ch = list(OUTLIER_NORM_CH)
            w[ch] = (w[ch] * np.float32(OUTLIER_NORM_GAIN)).astype(np.float16).astype(np.float32)
            out[name] = w
    return out


class OracleQwen3GenRuntime(OracleLlamaGenRuntime):
    model_type = "qwen3"

    def __init__(self, dims, state, generation=None):
        super().__init__(dims, state, generation)
        self.orc = Qwen3Oracle(dims, state)


def norm_rope_fp64(x, w, eps, cos, sin):
    """One head [..., 128] (the fp16 GEMM output as float64) -> x * rsqrt(mean(x^2) + eps) * w rotated by the position's table row
    cos / sin [64] (element i pairs with i + 64), exact to float64."""
    x = np.asarray(x, dtype=np.float64)
    y = x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + float(eps)) * np.asarray(w, dtype=np.float64)
    a, b = y[..., :64], y[..., 64:]
    c, s = np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)


# ---- the two kernels: fp64 restatement, the documented fp32 arithmetic, the verdicts ------------------------------------------------------
# Judged by the rules of tests/_rows_ref.py (the prefill kernel) and tests/_attn_ref.py (the step), unchanged: an fp16 output may be off
# by half an fp16 ulp of the fp64 value plus C x E, E = the error against fp64 of the documented fp32 arithmetic on the very problem,
# before the final rounding.  The norm puts rmsnorm's chain (sum of squares, one rsqrt, two products) in front of rope's rotation -
# the two ops C_ROWS = 7.3 was measured on (3.62 and 0.16, doubled) - and E is the emulation of the WHOLE composed arithmetic, so the
# constant carries over; tests/test_qwen3_host.py recomputes the honest orders' figure on these fixtures (sum orders, rsqrt one ulp up
# and down, rotation fused and not) and fails above C_ROWS / 2, as tests/test_rows_ref_host.py does for the other row kernels.  E is
# taken per (row, head): a head's 128 values share one factor, and a row's heads differ in scale with their outlier weights.
OP_ROPE_QKN = 11


def head_weights(rs):
    """q | k head-norm weights [256] fp32: 1 + N(0, 0.1) with four channels of each x 20 (as with_norm_outliers)"""
    w = (1.0 + 0.1 * rs.standard_normal(256)).astype(f32)
    for base in (0, 128):
        w[base + np.asarray(OUTLIER_NORM_CH)] *= f32(OUTLIER_NORM_GAIN)
    return w


def qkn_head32(x16, w, eps, cos, sin, order="lanes", nudge=0):
    """One head in the kernels' fp32 arithmetic, before the fp16 rounding.  order "lanes" = as documented: per-lane chains over the
    lane's 16 values (elements 8 l .. 8 l + 7, then their partners at + 64), the xor butterfly 1, 2, 4 over the head's 8 lanes, the
    rotation fused at element 0 of a lane's eight; "chain" = one chain over the 128 squares, rotation unfused; "pairwise" = pairwise
    sum, rotation fused everywhere.  nudge: the rsqrt result moved by that many fp32 ulps (hardware rsqrt is good to one)."""
    x = np.asarray(x16, dtype=f16).astype(f32)
    sq = (x * x).astype(f32)                                      # exact: an fp16 value's square has 22 bits
    if order == "chain":
        ss = R._chain32(sq)
    elif order == "pairwise":
        ss = R._pairwise32(sq)
    else:
        lanes = np.array([R._chain32(np.concatenate([sq[8 * l:8 * l + 8], sq[64 + 8 * l:64 + 8 * l + 8]])) for l in range(8)], f32)
        idx = np.arange(8)
        for o in (1, 2, 4):
            lanes = (lanes + lanes[idx ^ o]).astype(f32)
        ss = lanes[0]
    rs = R._rsqrt32(f32(f32(ss / f32(128.0)) + f32(eps)), nudge)
    y = ((x * rs).astype(f32) * np.asarray(w, dtype=f32)).astype(f32)
    c, s = np.asarray(cos, dtype=f32), np.asarray(sin, dtype=f32)
    x1, x2 = y[:64], y[64:]
    lo_u = ((c * x1).astype(f32) - (s * x2).astype(f32)).astype(f32)
    hi_u = ((c * x2).astype(f32) + (s * x1).astype(f32)).astype(f32)
    lo_f = (c.astype(f64) * x1 - (s * x2).astype(f32).astype(f64)).astype(f32)
    hi_f = (c.astype(f64) * x2 + (s * x1).astype(f32).astype(f64)).astype(f32)
    fused = np.ones(64, bool) if order == "pairwise" else (np.arange(64) % 8 == 0 if order == "lanes" else np.zeros(64, bool))
    return np.concatenate([np.where(fused, lo_f, lo_u), np.where(fused, hi_f, hi_u)])


def build_qkn(seed, T, H, n_kv, pad=8, max_pos=9, eps=1e-6, zero_head=None):
    """The prefill kernel's problem: T rows of a fused q | k | v buffer (N(0, 4), pad columns behind), positions restarting at 0 with
    the table's last among them, outlier norm weights; zero_head = (row, head): that head is all zero."""
    rs = np.random.RandomState(seed)
    ld = (H + 2 * n_kv) * 128 + pad
    cos, sin = A.rope_tables(max_pos)
    qkv = (rs.standard_normal((T, ld)) * 4).astype(f16)
    if zero_head is not None:
        t, h = zero_head
        qkv[t, h * 128:(h + 1) * 128] = 0
    return SimpleNamespace(rows=T, H=H, n_kv=n_kv, ld=ld, max_pos=max_pos, eps=float(f32(eps)), pos=R.ragged_positions(T, max_pos), cos=cos, sin=sin,
                           w=head_weights(rs), qkv=qkv)


def qkn_expected(p):
    """fp64 [T, ld] and the mask of what the kernel writes: the H + n_kv query and key heads; value heads and pad columns stay"""
    out, touched = p.qkv.astype(f64).copy(), np.zeros(p.qkv.shape, bool)
    for t in range(p.rows):
        c, s = p.cos[int(p.pos[t])], p.sin[int(p.pos[t])]
        for h in range(p.H + p.n_kv):
            sl = slice(h * 128, (h + 1) * 128)
            out[t, sl] = norm_rope_fp64(out[t, sl], p.w[128:] if h >= p.H else p.w[:128], p.eps, c, s)
            touched[t, sl] = True
    return out, touched


def qkn_emulated(p, order="lanes", nudge=0):
    out = p.qkv.astype(f32).copy()
    for t in range(p.rows):
        c, s = p.cos[int(p.pos[t])], p.sin[int(p.pos[t])]
        for h in range(p.H + p.n_kv):
            sl = slice(h * 128, (h + 1) * 128)
            out[t, sl] = qkn_head32(p.qkv[t, sl], p.w[128:] if h >= p.H else p.w[:128], p.eps, c, s, order, nudge)
    return out


def qkn_miss(p, got):
    """largest (error - half ulp) / E over the normed heads, E per (row, head): tests/_rows_ref.py's rule for rope"""
    want, touched = qkn_expected(p)
    emu = qkn_emulated(p).astype(f64)
    n = (p.H + p.n_kv) * 128
    E = np.abs(emu - want)[:, :n].reshape(p.rows, -1, 128).max(axis=2, keepdims=True)
    g, w = np.asarray(got).astype(f64)[:, :n].reshape(p.rows, -1, 128), want[:, :n].reshape(p.rows, -1, 128)
    over = np.maximum(np.abs(g - w) - A.half_ulp16(w), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(over > 0, over / np.broadcast_to(E, over.shape), 0.0)
    return float(np.nan_to_num(r, nan=np.inf).max())


def qkn_judge(p, got, what=""):
    g = np.asarray(got)
    assert np.isfinite(g.astype(f64)).all(), f"{what}: non-finite output"
    r = qkn_miss(p, g)
    print(f"{what}: worst (error - half ulp) / E = {r:.3f} (C_ROWS {R.C_ROWS})")
    assert r <= R.C_ROWS, f"{what}: off by {r:.3f} E, C_ROWS = {R.C_ROWS}"
    return r


# ---- the step: tests/_attn_ref.py's STEP problem with the norm in front of the rotation ------------------------------------------------
def build_qkn_step(seed, H, n_kv, pos, P, band=8, eps=1e-6):
    p = A.build_step(seed, H, n_kv, pos, P, "R", band=band)
    p.qk_w, p.qk_eps = head_weights(np.random.RandomState(seed + 1)), float(f32(eps))
    return p


def qkn_step_items(p, emul=False):
    """A.items()' pieces of the step (its addressing rules, restated for the one kind), the new row's q and k normed and rotated:
    fp64, or with emul the documented fp32 arithmetic rounded once to fp16"""
    B, H, G, Q, KV = p.band, p.H, p.H // p.n_kv, 128 * p.H, 128 * p.n_kv
    kc, vc = A.step_cache_views(p, p.cache)
    out = []
    for b in range(p.n_seq):
        pos, row = int(p.pos[b]), p.q[B + b]
        c, s = p.cos[pos], p.sin[pos]
        if emul:
            rot = lambda x, w: A.f16_sat(qkn_head32(x, w, p.qk_eps, c, s))
        else:
            rot = lambda x, w: norm_rope_fp64(x, w, p.qk_eps, c, s)
        for h in range(H):
            g = h // G
            knew = rot(row[Q + g * 128:Q + g * 128 + 128], p.qk_w[128:])
            vnew = row[Q + KV + g * 128:Q + KV + g * 128 + 128].astype(f16 if emul else f64)
            k = np.concatenate([kc[b, g, :pos].astype(knew.dtype), knew[None]])
            v = np.concatenate([vc[b, g, :pos].astype(vnew.dtype), vnew[None]])
            out.append(dict(q=rot(row[h * 128:h * 128 + 128], p.qk_w[:128])[None], k=k, v=v, bias=None, mask=None, scale=128.0 ** -0.5,
                            out_rows=np.array([b]), out_col=h * 128, p16=False, new=(b, g, pos, knew, vnew)))
    return out


def qkn_step_judge(p, got, what=""):
    """A.judge's rule on the step's context rows [n_seq, H 128] fp16: half an fp16 ulp + A.C x E, E = the chain emulation's largest
    error against fp64 over the problem's pieces (every piece is one row: the sample is all of them)"""
    ref, em = qkn_step_items(p), qkn_step_items(p, emul=True)
    got = np.asarray(got)
    assert got.dtype == f16 and got.shape == (p.n_seq, p.H * 128) and np.isfinite(got.astype(f64)).all(), what
    want = [A.attend64(it) for it in ref]
    E = max(float(np.abs(A.emulate_item(e).astype(f64) - w).max()) for e, w in zip(em, want))
    worst = 0.0
    for it, w in zip(ref, want):
        g = got[it["out_rows"], it["out_col"]:it["out_col"] + 128].astype(f64)
        over = np.abs(g - w) - A.half_ulp16(w)
        worst = max(worst, float(over.max()) / E)
        assert (over <= A.C * E).all(), f"{what}: row {it['out_rows'][0]}, head column {it['out_col']}: off by {float(over.max()):.3g} beyond half an ulp, {A.C} x E = {A.C * E:.3g}"
    print(f"{what}: worst (error - half ulp) / E = {worst:.3f} (C {A.C})")
    return worst
