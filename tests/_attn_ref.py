"""fp64 reference of every attention call of the engine (csrc/attention.h, csrc/llama_kernels.h), the fixtures its tests run and
the tolerance model they use.  Plain numpy; everything is written from the HF semantics quoted at the top of the two kernel files -
never from a kernel:

  T5     P = softmax(Q K^T + lut[h, clamp(j - i, +-128)] + mask), ctx = P V per sequence and head (d_kv = 64, no scaling); the decoder's
         self-attention is causal (tree form: row r at position pos[r] sees the rows tree_keys[r][0 .. pos[r]]; ragged form: every
         sequence its own row count), its cross-attention has neither bias nor mask; the query-side form is the same cross-attention
         with K = V = the raw encoder rows of the model's width.
  Llama  scale 128**-0.5, causal, query head h reads kv head h // (n_heads // n_kv) (repeat_kv); the cached step rotates the new
         row's q and k (x[i] cos - x[i + 64] sin | x[i + 64] cos + x[i] sin), after the optional q | k | v bias, appends k and v at
         `pos` and attends to the keys 0 .. pos.

A call is a `Problem` (the host buffers rk_debug_attn takes, bands included); `items()` cuts it into (sequence, head) pieces - query
rows, key rows, bias, mask, scale - and is the ONE place the addressing rules above are written down.  `expected64` runs fp64
softmax over the items; `emulated` runs the documented fp32 arithmetic over the same items; the mutants of
tests/test_attn_ref_host.py break one rule of `items()` or of the emulation each.

Tier S (selector, bit for bit).  Integer-valued fp16 operands: key rows are random +-A sign rows (A = 4 at d = 64 and on the
query side, 8 at d = 128), a query is a copy of its winner's key row, so the winner leads every other admissible key by at least
128 in natural units (asserted in fp64 by the builder, no silent redraw): every other probability is exactly 0 in fp32 and in fp16,
the sum exactly 1 and the context row the winner's V row bit for bit in any summation order.  Winners go to the first and the last key
of a sequence and to both sides of every 32-key edge.  Traps: rows a kernel must not admit (the row in front of a sequence and the
one behind it - a neighbour's row or a band row -, key i + 1 of a causal row, the cache row behind `pos`, a sibling branch's row, a
longer neighbour's row) are COPIES of some query's winner with another V row: admitted, the copy ties with the winner and the row
comes out as the mean of two V rows.  On the query side K = V, so the copy is twice the winner's row and wins outright.  Bias-only
cases: Q = 0 and a table that is 0 except one spike of 256 per head, at a different relative position per head: the winner is key
i + rel_h; rows whose winner falls outside their sequence (or that see several keys at the clamp entry) are uniform averages and
judged by tier R's rule.

Tier R (random, toleranced).  N(0, 1) operands (unscaled T5 scores are then as peaked as real T5's; the flat variant scales Q by
1 / 16), the bias table N(0, 2).  The yardstick E is the largest error against fp64 of `emulated(order="chain")` - fp32 k-ordered
score chains, exp2 of the fp32 product with log2(e), probabilities rounded to fp16 (matrix-core kernels) or kept in fp32 (fma-chain
kernels), one fp32 key-ordered P V chain, one division - BEFORE the final rounding, on a fixed sample of the problem's rows (of every
(sequence, head) piece the first four rows and SAMPLE_ROWS spread evenly: `_sample`).  An output may be off by the fp16 half-ulp of the expected value plus C * E.

Why C = 3.  Kernels sum in other orders than the chain, and E is a maximum over a sample while an output is held to it element by
element.  Measured on the CPU, in units of E (largest (error - half ulp) / E over the WHOLE output):
  - the fixtures of tests/test_attn_ref_host.py, both probability formats, online softmax per 64- and 128-key tile, flash-decoding
    merge of 64- and 128-key chunks, four interleaved chains per wave share + tree, and the chain itself: 1.09 with fp16
    probabilities, 1.07 with fp32 probabilities - the same figure for every order, because the largest error sits in rows of two or
    three keys (a causal row's first positions, a one-token sequence's neighbour), where a rounded probability is not averaged away
    and every order is the same sum;
  - the chain emulation as the "kernel" of every problem of tests/test_gpu_attention.py (about 150 problems, each held to the E of
    its own sample): 1.49 at most (encoder, fp16 probabilities), 1.46 with fp32 probabilities (decoder rows).
(tests/test_attn_ref_host.py::test_honest_orders_pass recomputes the first and fails above C.)  The largest is 1.49; 3 is twice
that - room for what the CPU orders do not cover: hardware exp2 and division of 1 ulp where numpy's are correctly rounded, a
probability rounded against a tile's running maximum instead of the row's.  With fp32 probabilities C * E is a few 1e-6, far
below one fp16 half-ulp: such a kernel must deliver the correctly rounded result or its neighbour at a tie.  With fp16 probabilities
C * E is of the order of the half-ulp itself.  The mutants of the host test fail by orders of magnitude more: C is not what
separates them.
"""
from types import SimpleNamespace

import numpy as np

ENC, DEC, XATTN, LLAMA, STEP = 1, 2, 3, 4, 5
LUT_R, LUT_N = 128, 257
SENTINEL = 0xCD
C = 3.0
MARGIN = 128.0
SAMPLE_ROWS = 8
F16_MAX = 65504.0
LOG2E32 = np.float32(1.4426950408889634)
f32, f16, f64 = np.float32, np.float16, np.float64


def f16_sat(x):
    return np.clip(np.asarray(x, dtype=f64), -F16_MAX, F16_MAX).astype(f32).astype(f16)


def half_ulp16(x):
    """Half a unit in the last place of fp16 at |x| (subnormal spacing below 2^-14)."""
    a = np.maximum(np.abs(np.asarray(x, dtype=f64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 11)


# ---- a call and its pieces ---------------------------------------------------------------------------------------------------
def problem(kind, **kw):
    p = SimpleNamespace(kind=kind, kv=None, seq_off=None, row_off=None, tree_keys=None, tree_pos=None, row_seq=None, pos=None, lut=None,
                        cos=None, sin=None, qkv_bias=None, cache=None, cross=False, n_kv=0, Ld=0, M=0, row0=0, d=0, P=0, ldkv=0, k_col=0,
                        v_col=0, exact=None, tier="R", p16=False, n_traps=0)
    p.__dict__.update(kw)
    return p


def _lut_bias(lut, h, qpos, kpos, mut):
    H = lut.shape[0]
    rel = kpos[None, :] - qpos[:, None]
    if mut == "bias_sign":
        rel = -rel
    r = LUT_R - 1 if mut == "clamp127" else LUT_R
    rel = np.clip(rel, -r, r)
    return lut[(h + 1) % H if mut == "bias_head" else h][rel + LUT_R]


def rope64(x, cos, sin, bias=None):
    """hf: apply_rotary_pos_emb on one head [128] (rotate_half pairs i with i + 64), fp64, after the optional projection bias."""
    x = np.asarray(x, dtype=f64) + (0.0 if bias is None else np.asarray(bias, dtype=f64))
    c, s = np.asarray(cos, dtype=f64), np.asarray(sin, dtype=f64)
    return np.concatenate([x[:64] * c - x[64:] * s, x[64:] * c + x[:64] * s])


def rope32(x, cos, sin, bias=None):
    """The kernels' arithmetic: fp32 bias add, fp32 products and sum, ONE fp16 rounding."""
    x = np.asarray(x, dtype=f16).astype(f32)
    if bias is not None:
        x = x + np.asarray(bias, dtype=f32)
    c, s = np.asarray(cos, dtype=f32), np.asarray(sin, dtype=f32)
    return f16_sat(np.concatenate([x[:64] * c - x[64:] * s, x[64:] * c + x[:64] * s]))


def items(p, mut=None, emul=False):
    """The (sequence, head) pieces of a call: dicts with q [nq, d], k [nk, d], v [nk, dv], bias [nq, nk] or None, mask [nq, nk] or
    None, scale, out_rows [nq] (interior rows of the output), out_col, p16 (this piece's kernel rounds probabilities to fp16).
    Rows are indexed in the WHOLE allocations (bands included), so a broken rule reads what a broken kernel would read.
    emul: the step's rotated rows in the kernels' fp32 arithmetic (one fp16 rounding) instead of fp64."""
    B, H, out = p.band, p.H, []
    p16 = p.p16 if callable(p.p16) else (lambda nk, _v=bool(p.p16): _v)

    def key_range(b, off):
        lo, hi = B + off[b], B + off[b + 1]
        if mut == "drop_last":
            hi -= 1
        if mut == "next_seq":
            hi += 1
        return np.arange(lo, max(hi, lo + 1))

    if p.kind == ENC:
        I = 64 * H
        for b in range(p.n_seq):
            rows, keys = np.arange(B + p.seq_off[b], B + p.seq_off[b + 1]), key_range(b, p.seq_off)
            for h in range(H):
                out.append(dict(q=p.q[rows, h * 64:h * 64 + 64], k=p.q[keys, I + h * 64:I + h * 64 + 64], v=p.q[keys, 2 * I + h * 64:2 * I + h * 64 + 64],
                                bias=_lut_bias(p.lut, h, rows, keys, mut), mask=None, scale=1.0, out_rows=rows - B, out_col=h * 64, p16=p16(len(keys))))
    elif p.kind == DEC:
        longest = p.Ld
        for b in range(p.n_seq if p.tree_pos is None else len(p.tree_pos)):
            if p.tree_pos is not None:
                src = (b + 1) % len(p.tree_pos) if mut == "tree_neighbour" else b
                rows, pos = np.array([B + b]), np.array([p.tree_pos[b]])
                keys = B + np.asarray(p.tree_keys).reshape(-1, p.Ld)[src, :p.tree_pos[b] + 1]
                kpos, mask = np.arange(len(keys)), None
            else:
                if p.row_off is not None:
                    r0, n = p.row_off[b], (longest if mut == "ragged_longest" else p.row_off[b + 1] - p.row_off[b])
                else:
                    r0, n = b * p.Ld, p.Ld
                rows, pos = B + r0 + np.arange(n), np.arange(n)
                if p.cross:
                    keys, mask = key_range(b, p.seq_off), None
                else:
                    keys = B + r0 + np.arange(n + (1 if mut in ("causal_plus1", "next_seq") else 0) - (1 if mut == "drop_last" and n > 1 else 0))
                    kk = np.arange(len(keys))
                    mask = kk[None, :] <= pos[:, None] + (1 if mut == "causal_plus1" else 0)
                    if mut == "next_seq":
                        mask[-1, -1] = True
                kpos = np.arange(len(keys))
            kvbuf = p.kv if p.cross else p.q
            for h in range(H):
                out.append(dict(q=p.q[rows, h * 64:h * 64 + 64], k=kvbuf[keys, p.k_col + h * 64:p.k_col + h * 64 + 64],
                                v=kvbuf[keys, p.v_col + h * 64:p.v_col + h * 64 + 64],
                                bias=None if p.lut is None else _lut_bias(p.lut, h, pos, kpos, mut), mask=mask, scale=1.0,
                                out_rows=rows - B, out_col=h * 64, p16=p16(len(keys))))
    elif p.kind == XATTN:
        d = p.d
        seq = np.array([p.row_seq[p.row0 + m] if p.row_seq is not None else (p.row0 + m) // p.Ld for m in range(p.M)])
        for b in np.unique(seq):
            ms, keys = np.nonzero(seq == b)[0], key_range(b, p.seq_off)
            for h in range(H):
                out.append(dict(q=p.q[B + ms, h * d:h * d + d], k=p.kv[keys], v=p.kv[keys], bias=None, mask=None, scale=1.0, out_rows=ms, out_col=h * d,
                                p16=p16(len(keys))))
    elif p.kind == LLAMA:
        G, Q, KV = H // p.n_kv, 128 * H, 128 * p.n_kv
        scale = 1.0 if mut == "scale_nohd" else 128.0 ** -0.5
        for b in range(p.n_seq):
            rows = np.arange(B + p.seq_off[b], B + p.seq_off[b + 1])
            keys = key_range(b, p.seq_off) if mut in ("drop_last", "next_seq") else (np.append(rows, rows[-1] + 1) if mut == "causal_plus1" else rows)
            mask = np.arange(len(keys))[None, :] <= np.arange(len(rows))[:, None] + (1 if mut == "causal_plus1" else 0)
            if mut == "next_seq":
                mask[-1, -1] = True
            for h in range(H):
                g = h % p.n_kv if mut == "kv_mod" else h // G
                out.append(dict(q=p.q[rows, h * 128:h * 128 + 128], k=p.q[keys, Q + g * 128:Q + g * 128 + 128], v=p.q[keys, Q + KV + g * 128:Q + KV + g * 128 + 128],
                                bias=None, mask=mask, scale=scale, out_rows=rows - B, out_col=h * 128, p16=p16(len(keys))))
    else:
        G, Q, KV = H // p.n_kv, 128 * H, 128 * p.n_kv
        scale = 1.0 if mut == "scale_nohd" else 128.0 ** -0.5
        kc, vc = step_cache_views(p, p.cache)
        rope = rope32 if emul else rope64
        for b in range(p.n_seq):
            pos, row = int(p.pos[b]), p.q[B + b]
            bias = (lambda c0: None) if p.qkv_bias is None else (lambda c0: p.qkv_bias[c0:c0 + 128])
            for h in range(H):
                g = h % p.n_kv if mut == "kv_mod" else h // G
                knew = rope(row[Q + g * 128:Q + g * 128 + 128], p.cos[pos], p.sin[pos], bias(Q + g * 128))
                vnew = row[Q + KV + g * 128:Q + KV + g * 128 + 128].astype(f64) + (0.0 if p.qkv_bias is None else bias(Q + KV + g * 128).astype(f64))
                if emul:
                    vnew = f16_sat(row[Q + KV + g * 128:Q + KV + g * 128 + 128].astype(f32) + (f32(0) if p.qkv_bias is None else bias(Q + KV + g * 128).astype(f32)))
                old = pos - (1 if mut == "drop_last" and pos > 0 else 0)
                k = np.concatenate([kc[b, g, :old].astype(knew.dtype), knew[None]])
                v = np.concatenate([vc[b, g, :old].astype(vnew.dtype), vnew[None]])
                if mut in ("causal_plus1", "next_seq") and pos + 1 < p.P:
                    k, v = np.concatenate([k, kc[b, g, pos + 1:pos + 2].astype(k.dtype)]), np.concatenate([v, vc[b, g, pos + 1:pos + 2].astype(v.dtype)])
                out.append(dict(q=rope(row[h * 128:h * 128 + 128], p.cos[pos], p.sin[pos], bias(h * 128))[None], k=k, v=v, bias=None, mask=None, scale=scale,
                                out_rows=np.array([b]), out_col=h * 128, p16=p16(len(k)), new=(b, g, pos, knew, vnew)))
    return out


def step_cache_views(p, cache):
    half = p.n_seq * p.n_kv * p.P * 128
    c = np.asarray(cache).reshape(-1)
    return c[:half].reshape(p.n_seq, p.n_kv, p.P, 128), c[half:2 * half].reshape(p.n_seq, p.n_kv, p.P, 128)


def _scores64(it):
    s = it["q"].astype(f64) @ it["k"].astype(f64).T * it["scale"]
    if it["bias"] is not None:
        s = s + it["bias"].astype(f64)
    if it["mask"] is not None:
        s = np.where(it["mask"], s, -np.inf)
    return s


def attend64(it):
    s = _scores64(it)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)) @ it["v"].astype(f64)


def expected64(p, mut=None):
    """fp64 context rows [out rows, ldctx], NaN where the call writes nothing."""
    out = np.full((p.out_rows, p.ldctx), np.nan)
    for it in items(p, mut):
        keep = it["out_rows"] < p.out_rows
        out[it["out_rows"][keep], it["out_col"]:it["out_col"] + it["v"].shape[1]] = attend64(it)[keep]
    return out


def expected_cache(p, emul=False):
    """The cache after a step: the new key and value at pos, nothing else changed.  fp64 (emul: the kernels' fp16 rows)."""
    kc, vc = step_cache_views(p, p.cache.astype(f16 if emul else f64))
    kc, vc = kc.copy(), vc.copy()
    for it in items(p, None, emul):
        b, g, pos, knew, vnew = it["new"]
        kc[b, g, pos], vc[b, g, pos] = knew, vnew
    return np.concatenate([kc.reshape(-1), vc.reshape(-1)])


# ---- the documented fp32 arithmetic ------------------------------------------------------------------------------------------
def _chain(x, axis):
    """k-ordered fp32 chain along axis (np.cumsum with dtype float32 accumulates sequentially)."""
    return np.take(np.cumsum(x, axis=axis, dtype=f32), -1, axis=axis)


def _exp2(x):
    return np.exp2((x.astype(f32) * LOG2E32).astype(f32)).astype(f32)


def _pv(pp, v, order):
    """sum_j pp[:, j] v[j] in fp32: one key-ordered chain, or ("tree4") the decoder kernels' form: wave w takes keys w, w + 4, ... in
    four interleaved chains, (a0 + a1) + (a2 + a3) per wave and over the waves."""
    prod = pp[:, :, None] * v[None]
    if order != "tree4":
        return _chain(prod, 1)
    def four(parts):
        z = np.zeros_like(prod[:, 0])
        a = [x if x is not None else z for x in parts]
        return ((a[0] + a[1]).astype(f32) + (a[2] + a[3]).astype(f32)).astype(f32)
    waves = []
    for w in range(4):
        chains = [(_chain(prod[:, w + 4 * c::16], 1) if prod[:, w + 4 * c::16].shape[1] else None) for c in range(4)]
        waves.append(four(chains))
    return four(waves)


def emulate_item(it, order="chain", tile=64, mut=None, rows=None):
    """One piece in fp32 -> [nq, dv] fp32 BEFORE the final fp16 rounding.  order: "chain" (the yardstick), "online" (running maximum,
    rescaled accumulators per `tile` keys), "flash" (independent partials per `tile` keys merged in key order) or "tree4"."""
    q, k, v = it["q"].astype(f32), it["k"].astype(f32), it["v"].astype(f32)
    bias, mask, p16 = it["bias"], it["mask"], it["p16"]
    if rows is not None:
        q, bias, mask = q[rows], (None if bias is None else bias[rows]), (None if mask is None else mask[rows])
    nq, nk = q.shape[0], k.shape[0]
    s = np.empty((nq, nk), dtype=f32)
    for i0 in range(0, nq, 64):                                     # fp32 k-ordered chains of exact products
        s[i0:i0 + 64] = _chain(q[i0:i0 + 64, None, :] * k[None, :, :], 2)
    if it["scale"] != 1.0:
        s = (s * f32(it["scale"])).astype(f32)
    if bias is not None:
        s = (s + bias.astype(f32)).astype(f32)
    if mask is not None:
        s = np.where(mask, s, f32(-1e30))
    if mut == "p16_before_max":                                     # exp(s) straight into fp16: saturates above 11, flushes below -17
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            e = f16_sat(np.minimum(_exp2(s).astype(f64), 1e30)).astype(f32)
            return _pv(e, v, "chain") / _chain(e, 1)[:, None]
    rnd = (lambda x: x.astype(f16).astype(f32)) if p16 else (lambda x: x)
    if order in ("chain", "tree4"):
        e = _exp2(s - s.max(axis=1, keepdims=True))
        return _pv(rnd(e), v, order) / _chain(e, 1)[:, None]
    edges = list(range(0, nk, tile))
    if order == "online":
        m, l, acc = np.full(nq, -1e30, dtype=f32), np.zeros(nq, dtype=f32), np.zeros((nq, v.shape[1]), dtype=f32)
        for t0 in edges:
            st = s[:, t0:t0 + tile]
            mn = np.maximum(m, st.max(axis=1))
            a, e = _exp2(m - mn), _exp2(st - mn[:, None])
            if mask is not None:
                e = np.where(mask[:, t0:t0 + tile], e, f32(0))
            l = (l * a + _chain(e, 1)).astype(f32)
            acc = (acc * a[:, None] + _chain(rnd(e)[:, :, None] * v[None, t0:t0 + tile], 1)).astype(f32)
            m = mn
        return acc / l[:, None]
    parts = []
    for t0 in edges:                                                  # flash-decoding: per chunk (max, sum, accumulator)
        st = s[:, t0:t0 + tile]
        mc = st.max(axis=1)
        e = _exp2(st - mc[:, None])
        if mask is not None:
            e = np.where(mask[:, t0:t0 + tile], e, f32(0))
        parts.append((mc, _chain(e, 1), _chain(rnd(e)[:, :, None] * v[None, t0:t0 + tile], 1)))
    g = np.max([mc for mc, _, _ in parts], axis=0)
    den, acc = np.zeros(nq, dtype=f32), np.zeros((nq, v.shape[1]), dtype=f32)
    for i, (mc, lc, ac) in enumerate(parts):
        w = np.ones(nq, dtype=f32) if (mut == "merge_no_rescale" and i + 1 < len(parts)) else _exp2(mc - g)
        den, acc = (den + w * lc).astype(f32), (acc + w[:, None] * ac).astype(f32)
    return acc / den[:, None]


def emulated(p, order="chain", tile=64, mut=None):
    """What a kernel of the documented arithmetic returns: fp16 [out rows, ldctx] over the pre-filled output."""
    out = p.out.copy()
    imut = mut if mut not in ("p16_before_max", "merge_no_rescale") else None
    for it in items(p, imut, emul=True):
        keep = it["out_rows"] < p.out_rows
        out[it["out_rows"][keep], it["out_col"]:it["out_col"] + it["v"].shape[1]] = f16_sat(emulate_item(it, order, tile, mut))[keep]
    return out


def _sample(n, k=SAMPLE_ROWS):
    """Rows of a piece that go into E: the first four (a causal row with two or three keys has the least averaging) and k spread evenly."""
    return np.unique(np.concatenate([np.arange(min(n, 4)), np.linspace(0, n - 1, min(n, k)).round().astype(int)]))


def yardstick(p):
    """E of the problem: the chain emulation's largest error against fp64 on the fixed sample, one figure per probability format:
    {True: E with fp16 probabilities, False: E with fp32 probabilities} (only the formats the problem's pieces use)."""
    ref, em = items(p), items(p, emul=True)
    memo = p.__dict__.setdefault("_E", {})
    E = {}
    for fmt in (False, True):
        if fmt in memo:
            if any(it["p16"] == fmt for it in em):
                E[fmt] = memo[fmt]
            continue
        idx = [i for i, it in enumerate(em) if it["p16"] == fmt]
        worst = 0.0
        for i in idx:
            rows = _sample(em[i]["q"].shape[0])
            worst = max(worst, float(np.abs(emulate_item(em[i], rows=rows).astype(f64) - attend64(ref[i])[rows]).max()))
        if idx:
            E[fmt] = memo[fmt] = worst
    return E


def judge(p, got, E=None, what=""):
    """Holds `got` [out rows, ldctx] fp16 (the interior of a kernel's output) to the problem: rows flagged exact bit for bit, the
    others within half an fp16 ulp + C E; what the call does not write must be what the caller put there.  Returns the largest
    (error - half ulp) / E per probability format (for the record); raises AssertionError with the first offending (sequence or
    row group, head, row, column)."""
    if getattr(p, "_want", None) is None:                           # a problem is built once and left unchanged: computed once
        p._want = expected64(p)
    want = p._want
    written = ~np.isnan(want)
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == f16
    stale = ~written & (got.view(np.uint16) != p.out.view(np.uint16))
    assert not stale.any(), f"{what}: output element {tuple(np.argwhere(stale)[0])} is not the call's to write"
    assert np.isfinite(got[written].astype(f64)).all(), f"{what}: non-finite output"
    ratios = {}
    if E is None and (p.tier != "S" or (p.exact is not None and not p.exact.all())):
        E = yardstick(p)
    for n, it in enumerate(items(p)):
        r, c0, w = it["out_rows"], it["out_col"], it["v"].shape[1]
        g, x = got[r, c0:c0 + w], want[r, c0:c0 + w]
        ex = np.ones(len(r), dtype=bool) if p.tier == "S" and p.exact is None else (p.exact[r, c0 // w] if p.exact is not None else np.zeros(len(r), dtype=bool))
        if ex.any():
            bad = g[ex].view(np.uint16) != f16_sat(x[ex]).view(np.uint16)
            if bad.any():
                i, j = np.argwhere(bad)[0]
                raise AssertionError(f"{what}: piece {n} (head column {c0}), output row {r[ex][i]}, column {c0 + j}: got {g[ex][i, j]}, the selected row has {x[ex][i, j]}")
        if (~ex).any():
            e = E[it["p16"]]
            err = np.abs(g[~ex].astype(f64) - x[~ex])
            over = err - half_ulp16(x[~ex])
            ratios[it["p16"]] = max(ratios.get(it["p16"], 0.0), float(over.max()) / e if e > 0 else 0.0)
            if (over > C * e).any():
                i, j = np.argwhere(over > C * e)[0]
                raise AssertionError(f"{what}: piece {n} (head column {c0}), output row {r[~ex][i]}, column {c0 + j}: got {g[~ex][i, j]}, fp64 {x[~ex][i, j]:.6g}, "
                                     f"error {err[i, j]:.3g} > half ulp {half_ulp16(x[~ex][i, j]):.3g} + {C} x E ({e:.3g})")
    return ratios


def judge_cache(p, got, what=""):
    """The cache after a step (interior, flat fp16): untouched rows bit for bit; the appended key within half an ulp of the fp64
    rotation + C x the fp32 rotation's own error (exactly it with identity tables), the appended value likewise."""
    want, em = expected_cache(p), expected_cache(p, emul=True).astype(f64)
    got = np.asarray(got).reshape(-1)
    new = np.zeros(got.size, dtype=bool)
    half = got.size // 2
    for it in items(p):
        b, g, pos, _, _ = it["new"]
        o = ((b * p.n_kv + g) * p.P + pos) * 128
        new[o:o + 128] = new[half + o:half + o + 128] = True
    stale = ~new & (got.view(np.uint16) != p.cache.reshape(-1).view(np.uint16))
    assert not stale.any(), f"{what}: cache element {np.argwhere(stale)[0][0]} changed and is not an appended row"
    if p.tier == "S":
        assert (got[new].view(np.uint16) == f16_sat(want[new]).view(np.uint16)).all(), f"{what}: the appended key / value rows are not the new row's"
        return
    e = float(np.abs(em[new] - want[new]).max())          # includes the emulation's own fp16 rounding: at least what a kernel may add
    err = np.abs(got[new].astype(f64) - want[new])
    assert (err <= half_ulp16(want[new]) + e).all(), f"{what}: appended row off by {err.max():.3g}"


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def sentinel16(shape):
    return np.frombuffer(bytes([SENTINEL]) * (2 * int(np.prod(shape))), dtype=f16).reshape(shape).copy()


def edges_of(L, step=32):
    """Keys a winner map should visit: the first, the last, both sides of every `step`-key edge."""
    ks = {0, L - 1}
    for e in range(step, L, step):
        ks.update((e - 1, e))
    return sorted(k for k in ks if 0 <= k < L)


def selector(rs, n, d, amp, queries, traps, strict=False, scale=1.0, what=""):
    """Key rows and the winner of every query in one key space of n rows.  queries: list of (admissible rows: a range or a tuple,
    preferred winners in order); traps: list of (query index, forbidden row).  Returns K [n, d] (+-amp sign rows; a trap row is a
    copy of its query's winner - twice it if strict), winners [len(queries)], the trap rows placed.  Asserts the margin in fp64."""
    K = (rs.randint(0, 2, size=(n, d)) * 2 - 1).astype(f64) * amp
    win = [None] * len(queries)
    group = {}                                                      # row -> rows holding the same key direction (itself included)

    def free(r, adm):
        return all(x == r or x not in adm for x in group.get(r, (r,)))

    def pick(qi):
        adm, prefer = queries[qi]
        for r in list(prefer) + [adm[int(x)] for x in rs.randint(0, len(adm), size=64)]:
            if r in adm and free(r, adm):
                return r
        raise AssertionError(f"{what}: no free winner for query {qi}")

    copies, placed = set(), []
    for qi, t in traps:
        adm = queries[qi][0]
        if t in adm or t in group or t in win or not 0 <= t < n:
            continue
        if win[qi] is not None:
            w = win[qi]
        elif queries[qi][1]:                                        # a query with preferences takes one of them or goes without a trap
            w = next((r for r in queries[qi][1] if r in adm and r not in group), None)
        else:
            w = pick(qi)
        if w is None or w in group:                                 # one copy per original
            continue
        win[qi] = w
        K[t] = K[w] * (2 if strict else 1)
        group[w] = group[t] = (w, t)
        copies.add(t)
        placed.append(t)
    for qi in range(len(queries)):
        if win[qi] is None:
            win[qi] = pick(qi)
    win = np.array(win)
    # the margin, in fp64, in natural units: the winner against every other admissible key (ranges that start together in one product)
    starts = {}
    for qi, (adm, _) in enumerate(queries):
        starts.setdefault(adm.start if isinstance(adm, range) else ("t", qi), []).append(qi)
    for key, qs in starts.items():
        if isinstance(key, tuple):
            rows, stops = np.asarray(queries[qs[0]][0]), None
        else:
            stops = np.array([queries[qi][0].stop for qi in qs])
            rows = np.arange(key, stops.max())
        s = K[rows] @ K[win[qs]].T * scale                            # [keys, queries of the group]
        if stops is not None:
            s[rows[:, None] >= stops[None, :]] = -np.inf
        s[rows[:, None] == win[qs][None, :]] = -np.inf
        lead = np.einsum("qd,qd->q", K[win[qs]], K[win[qs]]) * scale - s.max(axis=0)
        bad = np.nonzero(lead < MARGIN)[0]
        assert not len(bad), f"{what}: query {qs[bad[0]]}: margin {lead[bad[0]]:.0f} < {MARGIN:.0f}"
    return K, win, placed


def _rows_buffer(rs, rows, ld, band, tier, amp=4):
    """[band + rows + band, ld] fp16 of finite poison: integer sign rows (tier S) or N(0, 1) (tier R), pad columns and bands included."""
    n = rows + 2 * band
    if tier == "S":
        return ((rs.randint(0, 2, size=(n, ld)) * 2 - 1) * amp).astype(f16)
    return rs.standard_normal((n, ld)).astype(f16)


def _int_values(rs, shape):
    """Integer V entries, never 0: the fp64 softmax leaves 1e-300 of the losers in the row, which would decide the SIGN of a zero."""
    return (rs.randint(1, 513, size=shape) * (rs.randint(0, 2, size=shape) * 2 - 1)).astype(f16)


def _prefer(rs, adm, special, i):
    """Every second query visits the special keys in turn, the others a random admissible key."""
    sp = [int(k) for k in special if int(k) in adm]        # (int: a numpy integer `in range` walks the range)
    return [sp[(i // 2) % len(sp)]] if sp and i % 2 == 0 else []


def spike_lut(H, rels):
    lut = np.zeros((H, LUT_N), dtype=f32)
    for h in range(H):
        lut[h, rels[h % len(rels)] + LUT_R] = 256.0
    return lut


def _spike_exact(lut, h, qpos, nkeys, causal):
    """Rows of a bias-only case with exactly one key at the spike."""
    k = np.arange(nkeys)
    rel = np.clip(k[None, :] - np.asarray(qpos)[:, None], -LUT_R, LUT_R)
    hit = lut[h][rel + LUT_R] > 0
    if causal:
        hit &= k[None, :] <= np.asarray(qpos)[:, None]
    return hit.sum(axis=1) == 1


def build_enc(seed, H, lens, tier, band=8, pad=(0, 0), spike=None, flat=False):
    """T5 encoder call.  tier "S": selector; spike = list of relative positions (one per head, cyclic): the bias-only case."""
    rs = np.random.RandomState(seed)
    I, off = 64 * H, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, ldq, ldctx = int(off[-1]), 3 * I + pad[0], I + pad[1]
    q = _rows_buffer(rs, T, ldq, band, tier)
    p = problem(ENC, H=H, n_seq=len(lens), seq_off=off, band=band, ldq=ldq, ldctx=ldctx, out_rows=T, tier=tier, p16=True)
    if tier == "S" and spike is None:
        p.lut = np.zeros((H, LUT_N), dtype=f32)
        q[:, 2 * I:3 * I] = _int_values(rs, (T + 2 * band, I))
        for h in range(H):
            queries, traps = [], []
            for b, L in enumerate(lens):
                adm, sp = range(band + off[b], band + off[b + 1]), [band + off[b] + k for k in edges_of(L)]
                for i in range(L):
                    queries.append((adm, _prefer(rs, adm, sp[h % len(sp):] + sp[:h % len(sp)], i)))
                traps += [(len(queries) - L + (h % L), adm.start - 1), (len(queries) - 1 - (h % L), adm.stop)]
            K, win, placed = selector(rs, T + 2 * band, 64, 4, queries, traps, what=f"enc head {h}")
            p.n_traps += len(placed)
            q[:, I + h * 64:I + h * 64 + 64] = K
            q[band:band + T, h * 64:h * 64 + 64] = K[win]
    elif tier == "S":
        p.lut = spike_lut(H, spike)
        q[:, :I] = 0
        q[:, 2 * I:3 * I] = _int_values(rs, (T + 2 * band, I))
        p.exact = np.zeros((T, H), dtype=bool)
        for b, L in enumerate(lens):
            for h in range(H):
                p.exact[off[b]:off[b + 1], h] = _spike_exact(p.lut, h, np.arange(L), L, False)
    else:
        p.lut = (2.0 * rs.standard_normal((H, LUT_N))).astype(f32)
        if flat:
            q[:, :I] = (q[:, :I].astype(f32) / 16).astype(f16)
    p.q, p.out = q, sentinel16((T, ldctx))
    return p


def build_dec(seed, H, tier, *, Ld=0, n_seq=0, rows=None, key_lens=None, tree=None, band=8, pad=(0, 0), spike=None, flat=False, with_lut=True, ldkv_pad=0, spare=0):
    """T5 decoder call.  Self (key_lens None): fused rows q | k | v, causal, bias table (with_lut); rows = ragged row counts; tree =
    (tree_keys [R, Ld], tree_pos [R]).  Cross (key_lens given): q rows and a kv buffer (k | v), no bias, no mask.  spare: output rows
    behind the call's last row, pre-filled like the rest: a sequence that runs to the pass's longest row count lands there."""
    rs = np.random.RandomState(seed)
    I, cross = 64 * H, key_lens is not None
    if tree is not None:
        tk, tp = np.asarray(tree[0], dtype=np.int32), np.asarray(tree[1], dtype=np.int32)
        Ld, n_rows, counts, n_seq = tk.shape[1], len(tp), None, max(n_seq, 1)
    elif rows is not None:
        counts, n_seq, Ld = list(rows), len(rows), max(rows)
        n_rows = sum(counts)
    else:
        counts, n_rows = [Ld] * n_seq, n_seq * Ld
    roff = None if counts is None else np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ldq, ldctx = (I if cross else 3 * I) + pad[0], I + pad[1]
    q = _rows_buffer(rs, n_rows, ldq, band, tier)
    p = problem(DEC, H=H, n_seq=n_seq, Ld=Ld, band=band, ldq=ldq, ldctx=ldctx, out_rows=n_rows, tier=tier, cross=cross,
                row_off=roff if rows is not None else None, k_col=0 if cross else I, v_col=I if cross else 2 * I)
    if tree is not None:
        p.tree_keys, p.tree_pos = tk, tp
    if cross:
        koff = np.concatenate([[0], np.cumsum(key_lens)]).astype(np.int32)
        Tk, p.ldkv = int(koff[-1]), 2 * I + ldkv_pad
        kv = _rows_buffer(rs, Tk, p.ldkv, band, tier)
        p.seq_off = koff
    if tier == "S" and spike is None:
        p.lut = np.zeros((H, LUT_N), dtype=f32) if (with_lut and not cross) else None
        vbuf = kv if cross else q
        vbuf[:, p.v_col:p.v_col + I] = _int_values(rs, (vbuf.shape[0], I))
        nkeys = (Tk if cross else n_rows) + 2 * band
        for h in range(H):
            queries, traps = [], []
            if tree is not None:
                for r in range(n_rows):
                    adm = tuple(int(band + x) for x in tk[r, :tp[r] + 1])
                    queries.append((adm, [adm[-1]] if r % 2 == 0 else [adm[0]]))   # its own row | the root
                    # a sibling branch's own row: a row that does not descend from this one and that this one does not see
                    sib = [int(band + tk[s, tp[s]]) for s in list(range(r + 1, n_rows)) + list(range(r))
                           if band + tk[s, tp[s]] not in adm and adm[-1] not in [band + x for x in tk[s, :tp[s] + 1]]]
                    traps += [(r, t) for t in sib[:1] if r % 2 == 0]
            else:
                for b in range(n_seq):
                    n = counts[b]
                    if cross:
                        adm, sp = range(band + koff[b], band + koff[b + 1]), [band + koff[b] + k for k in edges_of(key_lens[b])]
                        for i in range(n):
                            queries.append((adm, _prefer(rs, adm, sp[h % len(sp):] + sp[:h % len(sp)], i)))
                        traps += [(len(queries) - n, adm.start - 1), (len(queries) - 1, adm.stop)]
                    else:
                        r0 = band + int(roff[b])
                        for i in range(n):
                            adm = range(r0, r0 + i + 1)
                            trap = (i >= 1 or n == 1) and ((i + h) % 3 == 0 or i == n - 1 or (i + 1) % 32 == 0)
                            queries.append((adm, [r0 + i] if trap else [[r0 + i], [r0], [r0 + i - 1], []][(i + h) % 4]))
                            if trap:                                               # key i + 1 (the last row's: the neighbour's or a band row);
                                traps.append((len(queries) - 1, r0 + i + 1))      # its query takes the diagonal: row 0 stays free for all
                        traps.append((len(queries) - n, r0 - 1))
            K, win, placed = selector(rs, nkeys, 64, 4, queries, traps, what=f"dec head {h}")
            p.n_traps += len(placed)
            vbuf[:, p.k_col + h * 64:p.k_col + h * 64 + 64] = K
            q[band:band + n_rows, h * 64:h * 64 + 64] = K[win]
    elif tier == "S":
        assert not cross and tree is None
        p.lut = spike_lut(H, spike)
        q[:, :I] = 0
        q[:, 2 * I:3 * I] = _int_values(rs, (q.shape[0], I))
        p.exact = np.zeros((n_rows, H), dtype=bool)
        for b in range(n_seq):
            for h in range(H):
                p.exact[roff[b]:roff[b + 1], h] = _spike_exact(p.lut, h, np.arange(counts[b]), counts[b], True)
    else:
        p.lut = (2.0 * rs.standard_normal((H, LUT_N))).astype(f32) if (with_lut and not cross) else None
        if flat:
            q[:, :I] = (q[:, :I].astype(f32) / 16).astype(f16)
    p.q, p.out, p.out_rows = q, sentinel16((n_rows + spare, ldctx)), n_rows + spare
    if cross:
        p.kv = kv
    return p


def build_xattn(seed, H, d, M, Ld, lens, tier, *, row0=0, row_seq=None, band=8, flat=False):
    """Query-side cross-attention: qk [M, H, d], enc [T, d]; query m belongs to sequence row_seq[row0 + m] or (row0 + m) // Ld."""
    rs = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(off[-1])
    q, kv = _rows_buffer(rs, M, H * d, band, tier), _rows_buffer(rs, T, d, band, tier)
    p = problem(XATTN, H=H, n_seq=len(lens), d=d, M=M, Ld=Ld, row0=row0, seq_off=off, band=band, ldq=H * d, ldkv=d, ldctx=H * d, out_rows=M, tier=tier,
                p16=True, row_seq=None if row_seq is None else np.asarray(row_seq, dtype=np.int32))
    seq = [int(p.row_seq[row0 + m]) if row_seq is not None else (row0 + m) // Ld for m in range(M)]
    if tier == "S":
        queries, traps = [], []
        for m in range(M):
            for h in range(H):
                b = seq[m]
                adm, sp = range(band + off[b], band + off[b + 1]), [band + off[b] + k for k in edges_of(lens[b], 64)]
                queries.append((adm, _prefer(rs, adm, sp[(m + h) % len(sp):] + sp[:(m + h) % len(sp)], m * H + h + (m & 1))))
                if h == m % H:
                    traps.append((len(queries) - 1, adm.stop if m % 2 else adm.start - 1))
        K, win, placed = selector(rs, T + 2 * band, d, 4, queries, traps, strict=True, what="xattn")
        p.n_traps += len(placed)
        kv[:] = K
        q[band:band + M] = K[win].reshape(M, H * d)
    elif flat:
        q[:] = (q.astype(f32) / 16).astype(f16)
    if tier == "R":                                                   # N(0, 1) rows of width d: scores of std sqrt(d); keep them T5-like
        q[:] = (q.astype(f32) * (8.0 / np.sqrt(d))).astype(f16)
    p.q, p.kv, p.out = q, kv, sentinel16((M, H * d))
    return p


def build_llama(seed, H, n_kv, lens, tier, *, band=8, pad=(0, 0), qscale=1.0):
    """Llama causal prefill: already-rotated qkv [T, (H + 2 n_kv) 128].  qscale (tier R): the queries times this - N(0, 1) rows give
    scores of N(0, 1) under the 128**-0.5 scale; 4 makes them as peaked as a trained model's."""
    rs = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, Q, KV, G = int(off[-1]), 128 * H, 128 * n_kv, H // n_kv
    ldq, ldctx = Q + 2 * KV + pad[0], Q + pad[1]
    q = _rows_buffer(rs, T, ldq, band, tier, amp=8)
    p = problem(LLAMA, H=H, n_kv=n_kv, n_seq=len(lens), seq_off=off, band=band, ldq=ldq, ldctx=ldctx, out_rows=T, tier=tier, p16=True)
    if tier == "S":
        q[:, Q + KV:Q + 2 * KV] = _int_values(rs, (T + 2 * band, KV))
        for g in range(n_kv):
            queries, traps = [], []
            for b, L in enumerate(lens):
                r0 = band + int(off[b])
                for r in range(G):
                    for i in range(L):
                        adm = range(r0, r0 + i + 1)
                        trap = (i >= 1 or L == 1) and ((i + r) % 5 == 0 or i == L - 1 or (i + 1) % 64 == 0)
                        queries.append((adm, [r0 + i] if trap else [[r0 + i], [r0], [r0 + i - 1], [r0 + (i // 64) * 64], []][(i + r + g) % 5]))
                        if trap:
                            traps.append((len(queries) - 1, r0 + i + 1))
                    traps.append((len(queries) - L, r0 - 1))
            K, win, placed = selector(rs, T + 2 * band, 128, 8, queries, traps, scale=128.0 ** -0.5, what=f"llama kv head {g}")
            p.n_traps += len(placed)
            q[:, Q + g * 128:Q + g * 128 + 128] = K
            n = 0
            for b, L in enumerate(lens):
                for r in range(G):
                    h = g * G + r
                    q[band + off[b]:band + off[b + 1], h * 128:h * 128 + 128] = K[win[n:n + L]]
                    n += L
    elif qscale != 1.0:
        q[:, :Q] = (q[:, :Q].astype(f32) * qscale).astype(f16)
    p.q, p.out = q, sentinel16((T, ldctx))
    return p


def rope_tables(max_pos, theta=10000.0):
    inv = theta ** (-np.arange(64, dtype=f64) / 64.0)
    ang = np.arange(max_pos, dtype=f64)[:, None] * inv[None, :]
    return np.cos(ang).astype(f32), np.sin(ang).astype(f32)


def build_step(seed, H, n_kv, pos, P, tier, *, bias=False, band=8):
    """Llama cached step: one new row per sequence at pos[b] over a cache of P positions.  Tier S: identity rotary tables."""
    rs = np.random.RandomState(seed)
    n_seq, Q, KV, G = len(pos), 128 * H, 128 * n_kv, H // n_kv
    ldq = Q + 2 * KV
    q = _rows_buffer(rs, n_seq, ldq, band, tier, amp=8)
    p = problem(STEP, H=H, n_kv=n_kv, n_seq=n_seq, P=P, pos=np.asarray(pos, dtype=np.int32), band=band, ldq=ldq, ldctx=Q, out_rows=n_seq, tier=tier, p16=False)
    if tier == "S":
        p.cos, p.sin = np.ones((P, 64), dtype=f32), np.zeros((P, 64), dtype=f32)
        kc = np.zeros((n_seq, n_kv, P, 128), dtype=f16)
        vc = _int_values(rs, (n_seq, n_kv, P, 128))
        q[:, Q + KV:] = _int_values(rs, (q.shape[0], KV))
        for b in range(n_seq):
            for g in range(n_kv):
                t = int(pos[b])
                sp = [k for k in [t, 0, t - 1] + edges_of(t + 1, 128) if 0 <= k <= t]
                queries = [(range(0, t + 1), [sp[(r + g + b) % len(sp)]]) for r in range(G)]
                K, win, placed = selector(rs, P, 128, 8, queries, [(0, t + 1)], scale=128.0 ** -0.5, what=f"step row {b} kv head {g}")
                p.n_traps += len(placed)
                kc[b, g] = K
                q[band + b, Q + g * 128:Q + g * 128 + 128] = K[t]           # the new key comes from the row ...
                kc[b, g, t] = -K[t]                                        # ... the stale cache row at pos would lose
                for r in range(G):
                    q[band + b, (g * G + r) * 128:(g * G + r) * 128 + 128] = K[win[r]]
        if bias:                                                          # integer bias, row entries shifted so that row + bias is the design
            p.qkv_bias = rs.randint(-3, 4, size=ldq).astype(f32)
            q[band:band + n_seq] = (q[band:band + n_seq].astype(f32) - p.qkv_bias).astype(f16)
        p.cache = np.concatenate([kc.reshape(-1), vc.reshape(-1)])
    else:
        p.cos, p.sin = rope_tables(P)
        p.cache = rs.standard_normal(2 * n_seq * n_kv * P * 128).astype(f16)
        if bias:                                                          # Qwen2: q / k biases of a few units, outliers among them
            p.qkv_bias = (rs.standard_normal(ldq) * np.where(rs.rand(ldq) < 0.02, 8.0, 0.5)).astype(f32)
    p.q, p.out = q, sentinel16((n_seq, Q))
    return p
