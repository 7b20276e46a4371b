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

The decoder's query-side chain (csrc/decoder_kernels.h; build_chain / judge_chain below, rk_debug_xattn_chain on the device).
hf: T5LayerCrossAttention as restated at the top of decoder_kernels.h, per decoder row m and head h:
  q_h = rowfactor_m (W_q,h x_m);  qk_h = W_k,h^T q_h;  ctx' = sum_t softmax_t(qk_h . e_t) e_t over the row's sequence;  ctx_h = W_v,h ctx'
with fp16 roundings at q, qk, ctx' (the merged sums) and ctx.  Each STAGE is judged against fp64 of its own inputs as the device
left them (rk_debug_xattn_chain returns every intermediate buffer), so an early rounding flip never sets a later tolerance:
  A  qk   from the host x, W_q, W_k and the row factor            (two roundings: q inside, qk at the end)
  B  part / stat merged in fp64, from the device's qk bytes and enc (fp32 partials, no rounding of their own); of a chunk that a
     shorter row does not have, part is never written and stat holds the kernels' empty mark (EMPTY_CHUNK)
  C  ctx  from the device's part / stat bytes and W_v              (two roundings: the merged sums inside, ctx at the end)
Tolerance of an fp16 output: half an fp16 ulp of the expected value + C_CHAIN E + flip.  E is the largest error against fp64 of
the stage's LAST product in fp32 (one k-ordered chain) given the reference's own inner fp16 values, on the sample rows.  flip bounds the
inner rounding element by element: an inner value (q_j, a merged sum) whose fp64 value lies within C_CHAIN E_inner
of an fp16 rounding boundary (E_inner = the fp32 emulation's largest error of the inner values on the sample) may be delivered as
either neighbour, and each such value moves output n by at most ulp(inner) |W[n, j]|: flip[n] = the sum of that over the ambiguous
inner values of the very (row, head) - per element, computed for every row, nothing chosen in advance and 0 for most elements.
The fp32 partials of stage B get C_CHAIN E alone, E = `yardstick` of the XATTN problem made of the device's qk bytes.

C_CHAIN, measured on the CPU as C was (tests/test_attn_ref_host.py::test_chain_honest_orders_pass recomputes it and fails above
it): the honest summation orders stand in for the kernel on the chain fixtures of that file and on the GPU test's own shapes
(CHAIN_SHAPES, but the two widest) - K in contiguous eighths with the fixed tree ((w0 + w4) + (w2 + w6)) + ((w1 + w5) + (w3 + w7)),
16-steps interleaved over four accumulators, one sequential chain; the chunk merge as an fma chain and with 4 and with 16 chunk
products summed before they meet the accumulator.  Largest (error - half ulp - flip) / E over whole outputs, and largest inner
error / E_inner (what the flip window is made of):
  stage A (qk) 0.05   inner q 1.00   stage B (merged partials) 1.95   inner merged sums 2.06   xctx 0.22   stage C (ctx) 0.21
(a stage's last product is one short chain on exact fp16 inputs: what is left beyond the half ulp and the flips is next to nothing.
E is a maximum over SAMPLE rows - `chain_sample`: rows of every key length - while an output is held to it element by element,
hence figures above 1 where the error grows with the chunk count: 23 and 65 chunks.)  The largest is 2.06; C_CHAIN is twice that,
rounded up to a tenth.  The mutants of the host test fail by orders of magnitude more: C_CHAIN is not what separates them.
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


# ---- the decoder's query-side chain: q projection -> W_k^T q -> chunk kernel -> merge -> W_v (csrc/decoder_kernels.h) ------------
# (what is judged, the tolerance and the measured C_CHAIN: the module docstring)
C_CHAIN = 4.2
XS, EPS = 0.0625, 1e-6            # RK_XRAW_SCALE and the toy checkpoints' layer_norm_epsilon (the GPU test checks both against the engine)
WS_FILL = np.array([0x7F800000], dtype=np.uint32).view(f32)[0]   # +inf: what the test puts into the part / stat workspaces - a chunk a
                                                                    # kernel must not read turns the row into NaN if it is read


EMPTY_CHUNK = (-1e30, 0.0)        # what the chunk kernels leave in stat for a chunk of the call's grid that a shorter row does not have
                                  # (attention.h: "mark the chunk empty for the combine step"); its partial sums are never written


def _perm_heads(rs, d, H):
    """H disjoint 64-column supports of the d columns."""
    return rs.permutation(d)[:H * 64].reshape(H, 64)


def build_chain(seed, M, Ld, H, d, lens, tier, *, norm="none", nb=0, row0=0, row_seq=None, band=8, ldx_pad=0, ldo_pad=0):
    """One call of rk_debug_xattn_chain.  norm: "none" (factor 1), "rowscale" or "ssq" (nb block sums per row).  Tier S: selection
    matrices with disjoint column supports per head (needs 64 H <= d), x = the winner's +-4 entries / a power-of-two row factor that
    differs from row to row; winners and traps per head as build_dec's cross form places them (first and last key, both sides of every
    64-key edge, the row in front of the sequence and the one behind it as a doubled copy); margin asserted by `selector`."""
    rs = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, I = int(off[-1]), 64 * H
    p = SimpleNamespace(M=M, Ld=Ld, H=H, d=d, n_seq=len(lens), seq_off=off, row0=row0, band=band, ldx=d + ldx_pad, ldo=I + ldo_pad, tier=tier,
                        norm=norm, nb=nb, eps=EPS, xs=XS, rowscale=None, ssq=None, n_traps=0,
                        row_seq=None if row_seq is None else np.asarray(row_seq, dtype=np.int32))
    p.seq = chain_seq(p)
    assert p.seq.min() >= 0 and p.seq.max() < p.n_seq
    enc = _rows_buffer(rs, T, d, band, tier)
    x = _rows_buffer(rs, M, p.ldx, 0, tier)
    if tier == "S":
        assert I <= d, "tier S needs disjoint column supports per head: 64 H <= d"
        rf = 2.0 ** ((np.arange(M) * 3) % 5 - 2.0)                                      # 1/4 .. 4, neighbours differ
        sq, sk, sv = _perm_heads(rs, d, H), _perm_heads(rs, d, H), _perm_heads(rs, d, H)
        wq, wk, wv = np.zeros((I, d), dtype=f16), np.zeros((I, d), dtype=f16), np.zeros((I, d), dtype=f16)
        for h in range(H):
            wq[h * 64 + np.arange(64), sq[h]] = 1
            wk[h * 64 + np.arange(64), sk[h]] = 1
            wv[h * 64 + np.arange(64), sv[h]] = 1
            queries, traps = [], []
            for m in range(M):
                b = int(p.seq[m])
                adm, sp = range(band + off[b], band + off[b + 1]), [band + off[b] + k for k in edges_of(lens[b], 64)]
                queries.append((adm, _prefer(rs, adm, sp[(m + h) % len(sp):] + sp[:(m + h) % len(sp)], 2 * (m + h) + (m & 1))))
                traps.append((m, adm.stop if (m + h) % 2 else adm.start - 1))
            K, win, placed = selector(rs, T + 2 * band, 64, 4, queries, traps, strict=True, what=f"chain head {h}")
            p.n_traps += len(placed)
            enc[:, sk[h]] = K
            x[:, sq[h]] = K[win] / rf[:, None]
    else:
        wq = (rs.standard_normal((I, d)) / np.sqrt(d)).astype(f16)
        wk = (rs.standard_normal((I, d)) / np.sqrt(d)).astype(f16)       # 1 / sqrt(64) for K = 64, and 8 / sqrt(d): T5-like scores (build_xattn)
        wv = (rs.standard_normal((I, d)) / np.sqrt(d)).astype(f16)
        amp = np.where(np.arange(M) % 5 == 3, 2e-3, np.exp(rs.uniform(-1, 2, size=M)))    # every fifth row: a mean square of a few eps
        raw = (rs.standard_normal((M, d)) * amp[:, None]).astype(f32)
        ms = (raw.astype(f64) ** 2).mean(axis=1)
        if norm == "none":
            rf = np.ones(M)
            x[:, :d] = (raw / np.sqrt(ms + EPS)[:, None]).astype(f16)
        else:
            x[:, :d] = (raw * f32(XS)).astype(f16)
            if norm == "ssq":
                p.ssq = np.stack([(b.astype(f32) ** 2).sum(axis=1, dtype=f32) for b in np.array_split(raw, nb, axis=1)], axis=1).astype(f32)
            else:
                rf = (1.0 / np.sqrt(ms + EPS) / XS).astype(f32).astype(f64)
    if norm == "rowscale":
        p.rowscale = rf.astype(f32)
    elif norm == "ssq" and tier == "S":       # block sums that give (about) the power of two: the fp16 rounding of q absorbs the fp32 rsqrt
        tot = d * ((rf * XS) ** -2.0 - EPS)
        p.ssq = (tot[:, None] * rs.dirichlet(np.ones(nb), size=M)).astype(f32)
    elif norm == "none" and tier == "S":
        x[:] = (x.astype(f64) * np.repeat(rf[:, None], p.ldx, axis=1)).astype(f16)        # factor 1: x carries the entries themselves
    p.x, p.wq, p.wk, p.wv, p.enc = x, wq, wk, wv, enc
    p.ctx0 = sentinel16((M, p.ldo))
    return p


_MIX = [1, 63, 64, 65, 129, 200, 7, 130, 128, 33, 2, 127, 70]
_SHORT = [1, 64, 130, 65, 7, 128, 33, 129, 63, 100, 2]
# The shapes of tests/test_gpu_xattn_chain.py, name -> (M, Ld, H, d, key lengths, extra builder arguments): the smallest that reach each
# path of the two kernels of decoder_kernels.h and of the block loop ("How the decoder's chain is tested")
CHAIN_SHAPES = {
    "one-key": (1, 1, 2, 128, [1], {}),
    "one-chunk": (1, 1, 2, 128, [64], {}),
    "setwise": (13, 1, 6, 512, [1450, 1, 64, 65, 700, 1409, 128, 129, 63, 1000, 23, 1450, 333], {}),
    "valu": (33, 1, 6, 384, [_MIX[i % 13] for i in range(33)], {}),
    "large": (257, 1, 16, 1024, [_SHORT[i % 11] for i in range(257)], {}),
    "wide": (130, 1, 16, 1280, [_MIX[i % 13] for i in range(130)], {}),
    "row0": (33, 4, 6, 512, [130, 64, 5, 200, 1, 65, 63, 129, 70], dict(row0=3)),
    "tree": (33, 4, 6, 512, [130, 64, 5, 200, 1, 65, 63, 129, 70], dict(row0=3, row_seq=[(7 * i + i // 5) % 9 for i in range(36)])),
    "long": (70, 1, 2, 128, [4100, 70], dict(row_seq=[(i % 3 == 1) * 1 for i in range(70)])),
    "rows": (520, 1, 2, 128, [1, 5, 33, 63, 64, 64, 17, 50], dict(row_seq=[(5 * i + i // 8) % 8 for i in range(520)])),
}


def build_chain_shape(name, norm, nb, tier, band=8):
    M, Ld, H, d, lens, kw = CHAIN_SHAPES[name]
    return build_chain(700 + sorted(CHAIN_SHAPES).index(name), M, Ld, H, d, lens, tier, norm=norm, nb=nb, band=band, ldx_pad=8 if name == "valu" else 0,
                       ldo_pad=8 if name in ("valu", "one-key", "tree") else 0, **kw)


def chain_seq(p, mut=None):
    m = np.arange(p.M)
    if mut == "seq_ignores_row0":
        return m // p.Ld if p.row_seq is None else p.row_seq[m]
    if p.row_seq is None or mut == "row_seq_ignored":
        return (p.row0 + m) // p.Ld
    return p.row_seq[p.row0 + m]


def chain_factor(p, mut=None, dt=f64):
    """Row factors [M]: rowscale, or rsqrt(sum of the block sums / d + eps) / xs, or 1.  dt = f32: the kernels' arithmetic."""
    if mut == "no_factor" or p.norm == "none":
        rf = np.ones(p.M, dtype=dt)
    elif p.norm == "rowscale":
        rf = p.rowscale.astype(dt)
    else:
        s = p.ssq[:, :p.nb - 1] if mut == "ssq_nb_minus1" else p.ssq
        s = _chain(s, 1).astype(dt) if dt == f32 else s.astype(f64).sum(axis=1)
        rf = (dt(1) / np.sqrt(s / dt(p.d) + (dt(0) if mut == "no_eps" else dt(p.eps))) / dt(p.xs)).astype(dt)
    return np.roll(rf, -1) if mut == "factor_next_row" else rf


def _heads(w, H):
    return w.reshape(H, 64, -1)


def chain_qk64(p):
    """Stage A in fp64: q [M, H, 64] before its rounding, and qk [M, H, d] from the fp16-rounded (saturated) q."""
    q = chain_factor(p)[:, None, None] * np.einsum("hjc,mc->mhj", _heads(p.wq.astype(f64), p.H), p.x[:, :p.d].astype(f64))
    return q, np.einsum("hjc,mhj->mhc", _heads(p.wk.astype(f64), p.H), f16_sat(q).astype(f64))


def chain_ctxp64(p, qk):
    """Stage B in fp64: ctx' [M, H, d] = sum_t softmax_t(qk_h . e_t) e_t over the keys of every row's own sequence, from qk [M, H, d]."""
    out = np.empty((p.M, p.H, p.d))
    for m in range(p.M):
        e = p.enc[p.band + p.seq_off[p.seq[m]]:p.band + p.seq_off[p.seq[m] + 1]].astype(f64)
        s = qk[m].astype(f64) @ e.T
        w = np.exp(s - s.max(axis=1, keepdims=True))
        out[m] = (w / w.sum(axis=1, keepdims=True)) @ e
    return out


def chain_xattn_problem(p, qk, rows):
    """Stage B's inputs for the rows given as an XATTN problem of their own (the yardstick's sample): the device's qk rows and the
    encoder rows."""
    B = p.band
    pb = problem(XATTN, H=p.H, n_seq=p.n_seq, d=p.d, M=len(rows), Ld=1, row0=0, seq_off=p.seq_off, band=B, ldq=p.H * p.d, ldkv=p.d,
                 ldctx=p.H * p.d, out_rows=len(rows), tier=p.tier, p16=True, row_seq=p.seq[rows].astype(np.int32))
    pb.q = np.zeros((len(rows) + 2 * B, p.H * p.d), dtype=f16)
    pb.q[B:B + len(rows)] = np.asarray(qk)[rows].reshape(len(rows), -1)
    pb.kv, pb.out = p.enc, sentinel16((len(rows), p.H * p.d))
    return pb


def chain_sample(p):
    """Rows that go into E: `_sample` of the rows and the first two rows of every distinct key length (the error of the softmax stage
    depends on the number of keys first of all: a row of two keys has the least averaging)."""
    L = np.diff(p.seq_off)[p.seq]
    return np.unique(np.concatenate([_sample(p.M)] + [np.nonzero(L == v)[0][:2] for v in np.unique(L)]))


def chain_nv(p):
    """64-key chunks of every row's own sequence."""
    return (np.diff(p.seq_off)[p.seq] + 63) // 64


def chain_merge64(p, part, stat, mut=None):
    """The normalised merge of part [M, nch, H, d] / stat [M, nch, H, 2] over every row's own chunks, fp64 -> [M, H, d]."""
    nch = part.shape[1]
    valid = (np.arange(nch)[None, :] < (nch if mut == "merge_call_nch" else chain_nv(p)[:, None]))[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.where(valid, stat[..., 0].astype(f64), -np.inf)
        w = np.ones_like(mx) * valid if mut == "merge_no_rescale" else np.exp(mx - mx.max(axis=1, keepdims=True))
        w = np.where(valid, w, 0.0)
        den = (w * np.where(valid, stat[..., 1].astype(f64), 0.0)).sum(axis=1)
        return (w[..., None] * np.where(valid[..., None], part.astype(f64), 0.0)).sum(axis=1) / den[..., None]


def chain_ctx64(p, merged):
    """Stage C's product in fp64 from the fp16-rounded merged sums: [M, 64 H]."""
    return np.einsum("hnc,mhc->mhn", _heads(p.wv.astype(f64), p.H), f16_sat(merged).astype(f64)).reshape(p.M, 64 * p.H)


# the documented fp32 arithmetic of the chain's products, in the orders a kernel may take
def _dot32(w, x, order="chain"):
    """x [R, K] . w [N, K]^T in fp32 -> [R, N].  chain: one k-ordered chain; eighths: K in eight contiguous ranges, one chain each,
    the fixed tree of dec_tree_reduce2; inter16: 16-steps dealt in turn to four accumulators, (a0 + a1) + (a2 + a3)."""
    prod = x.astype(f32)[:, None, :] * w.astype(f32)[None, :, :]
    K = prod.shape[2]
    if order == "chain" or K < 128:
        return _chain(prod, 2)
    if order == "eighths":
        a = [_chain(prod[:, :, i * K // 8:(i + 1) * K // 8], 2) for i in range(8)]
        return (((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]))).astype(f32)
    st = prod.reshape(prod.shape[0], prod.shape[1], K // 16, 16)
    a = [_chain(st[:, :, i::4].reshape(prod.shape[0], prod.shape[1], -1), 2) for i in range(4)]
    return ((a[0] + a[1]) + (a[2] + a[3])).astype(f32)


def emul_q(p, rows, order="chain", mut=None):
    """q [R, H, 64] in fp32 BEFORE its rounding."""
    H = p.H
    wq = np.roll(_heads(p.wq, H), -1, axis=0) if mut == "wq_head" else _heads(p.wq, H)
    y = np.stack([_dot32(wq[h], p.x[rows, :p.d], order) for h in range(H)], axis=1)
    rf = chain_factor(p, mut, f32)[rows, None, None]
    if mut == "factor_after_round":
        return f16_sat(y).astype(f32) * rf
    return (y * rf).astype(f32)


def emul_qk(p, q16, mut=None):
    """qk [R, H, d] in fp32 BEFORE its rounding, from fp16 q [R, H, 64] (K = 64: one chain)."""
    wk = _heads(p.wk, p.H)
    if mut == "wk_untransposed":                                    # the head's block read as [d][64] without the regrouping
        return np.stack([_chain(q16[:, h].astype(f32)[:, None, :] * wk[h].reshape(p.d, 64).astype(f32)[None], 2) for h in range(p.H)], axis=1)
    return np.stack([_chain(q16[:, h].astype(f32)[:, :, None] * wk[h].astype(f32)[None], 1) for h in range(p.H)], axis=1)


def emul_part(p, qk16, mut=None):
    """The chunk kernel in fp32: part [M, nch, H, d], stat [M, nch, H, 2]; chunks beyond a row's own stay WS_FILL."""
    nch = int((np.diff(p.seq_off).max() + 63) // 64)
    part, stat = np.full((p.M, nch, p.H, p.d), WS_FILL, dtype=f32), np.full((p.M, nch, p.H, 2), WS_FILL, dtype=f32)
    stat[:] = EMPTY_CHUNK
    seq = chain_seq(p, mut)
    for m in range(p.M):
        e = p.enc[p.band + p.seq_off[seq[m]]:p.band + p.seq_off[seq[m] + 1]].astype(f32)
        s = _chain(qk16[m].astype(f32)[:, None, :] * e[None], 2)                                  # [H, L]
        for ck in range((len(e) + 63) // 64):
            sc, ec = s[:, ck * 64:ck * 64 + 64], e[ck * 64:ck * 64 + 64]
            mc = sc.max(axis=1)
            pr = _exp2(sc - mc[:, None])
            stat[m, ck, :, 0], stat[m, ck, :, 1] = mc, _chain(pr, 1)
            part[m, ck] = _chain(pr.astype(f16).astype(f32)[:, :, None] * ec[None], 1)
    return part, stat


def emul_merge(p, part, stat, rows, merge="fma", mut=None):
    """The merge of dec_cross_cv_kernel / xattn_combine_kernel in fp32 -> merged [R, H, d] BEFORE its rounding.  merge: "fma" (one
    fused chain in chunk order), 4 or 16 (that many chunk products summed first, then added)."""
    out = np.zeros((len(rows), p.H, p.d), dtype=f32)
    nvs = chain_nv(p)
    for i, m in enumerate(rows):
        nv = part.shape[1] if mut == "merge_call_nch" else int(nvs[m])
        mx, sm = stat[m, :nv, :, 0], stat[m, :nv, :, 1]
        with np.errstate(invalid="ignore", over="ignore"):
            w = np.ones_like(mx) if mut == "merge_no_rescale" else np.exp((mx - mx.max(axis=0)).astype(f32)).astype(f32)
            den = _chain(w * sm, 0)
            if merge == "fma":
                acc = np.zeros((p.H, p.d), dtype=f32)
                for ck in range(nv):
                    acc = (w[ck].astype(f64)[:, None] * part[m, ck].astype(f64) + acc.astype(f64)).astype(f32)
            else:
                acc = np.zeros((p.H, p.d), dtype=f32)
                for c0 in range(0, nv, merge):
                    acc = (acc + _chain(w[c0:c0 + merge, :, None] * part[m, c0:min(c0 + merge, nv)], 0)).astype(f32)
            out[i] = acc * (f32(1) / den)[:, None]
    return out


def emul_ctx(p, s16, order="chain", mut=None):
    """ctx [R, 64 H] in fp32 BEFORE its rounding, from merged sums [R, H, d] (fp16, or fp32 for the mutant that skips the rounding)."""
    wv = np.roll(_heads(p.wv, p.H), -1, axis=0) if mut == "wv_head" else _heads(p.wv, p.H)
    return np.concatenate([_dot32(wv[h], s16[:, h], order) for h in range(p.H)], axis=1)


def emulated_chain(p, order="chain", merge="fma", mut=None, fused=True):
    """What rk_debug_xattn_chain returns when kernels of the documented arithmetic run it: dict of qk (whole allocation, sentinel
    bands), part, stat, xctx (None when fused), ctx [M, ldo], and the inner values q32 / merged32 for the host test's record."""
    rows = np.arange(p.M)
    q32 = emul_q(p, rows, order, mut)
    qk = sentinel16((p.M + 2 * p.band, p.H, p.d))
    qk[p.band:p.band + p.M] = f16_sat(emul_qk(p, f16_sat(q32), mut))
    part, stat = emul_part(p, qk[p.band:p.band + p.M], mut)
    merged32 = emul_merge(p, part, stat, rows, merge, mut)
    with np.errstate(invalid="ignore"):
        inner = merged32 if mut == "no_inner_round" else f16_sat(merged32)
        ctx = p.ctx0.copy()
        val = f16_sat(emul_ctx(p, inner, order, mut))
    if mut == "ctx_slab_later":
        ctx[2:, :64 * p.H] = val[:-2]
    else:
        ctx[:, :64 * p.H] = val
    return dict(qk=qk, part=part, stat=stat, xctx=None if fused else f16_sat(merged32).reshape(p.M, -1), ctx=ctx, q32=q32, merged32=merged32)


def _amb_flip(v64, E_inner, wabs):
    """flip [R, H, N]: v64 [R, H, K] inner values in fp64, wabs [H, N, K] = |W|.  An inner value within C_CHAIN E_inner of an fp16 rounding
    boundary may be either neighbour: each moves output n by at most one ulp of it times |W[n, k]|."""
    hu = half_ulp16(v64)
    dist = hu - np.abs(v64 - f16_sat(v64).astype(f64))
    amb = (dist <= C_CHAIN * E_inner) * 2.0 * hu
    return np.einsum("rhk,hnk->rhn", amb, wabs)


def chain_reference(p, res, cache=None):
    """Everything judge_chain holds a result to, from the problem and the DEVICE's intermediate bytes.  cache: dict shared by the
    runs of one problem - stage A depends on the host operands only, stages B and C on the bytes of qk and of part / stat."""
    import hashlib
    cache = {} if cache is None else cache
    H, d, M, B = p.H, p.d, p.M, p.band
    rows = chain_sample(p)
    if "A" not in cache:
        q64, want = chain_qk64(p)
        a = dict(want=want)
        if p.tier != "S":
            qs = emul_q(p, rows)
            a["Eq"] = float(np.abs(qs.astype(f64) - q64[rows]).max())
            a["E"] = float(np.abs(emul_qk(p, f16_sat(q64[rows])).astype(f64) - want[rows]).max())
            a["flip"] = _amb_flip(q64, a["Eq"], np.abs(_heads(p.wk.astype(f64), H)).transpose(0, 2, 1))
            a["q64"] = q64
        cache["A"] = a
    out = dict(A=cache["A"])
    qk = np.asarray(res["qk"])[B:B + M]
    key = ("B", hashlib.sha1(qk.tobytes()).hexdigest())
    if key not in cache:
        cache[key] = dict(want=chain_ctxp64(p, qk), E=None if p.tier == "S" else yardstick(chain_xattn_problem(p, qk, rows))[True])
    out["B"] = cache[key]
    part, stat = res["part"], res["stat"]
    key = ("C", hashlib.sha1(part.tobytes() + stat.tobytes()).hexdigest())
    if key not in cache:
        merged = chain_merge64(p, part, stat)
        c = dict(merged=merged, want=chain_ctx64(p, merged))
        if p.tier != "S" and np.isfinite(merged).all():
            c["Em"] = float(np.abs(emul_merge(p, part, stat, rows).astype(f64) - merged[rows]).max())
            c["E"] = float(np.abs(emul_ctx(p, f16_sat(merged[rows])).astype(f64) - c["want"][rows]).max())
            c["flip"] = _amb_flip(merged, c["Em"], np.abs(_heads(p.wv.astype(f64), H))).reshape(M, 64 * H)
        cache[key] = c
    out["C"] = cache[key]
    return out


def _bits_equal(got, want64, what):
    bad = np.asarray(got).view(np.uint16) != f16_sat(want64).view(np.uint16)
    assert not bad.any(), f"{what}: element {tuple(np.argwhere(bad)[0])}: got {np.asarray(got)[tuple(np.argwhere(bad)[0])]}, the selection gives {want64[tuple(np.argwhere(bad)[0])]}"


def _within(got, want64, E, flip, what, half=True):
    """(error - half ulp - flip) / E over the whole output; asserts it stays within C_CHAIN."""
    assert np.isfinite(np.asarray(got, dtype=f64)).all(), f"{what}: non-finite output"
    over = np.abs(np.asarray(got, dtype=f64) - want64) - (half_ulp16(want64) if half else 0.0) - flip
    if (over > C_CHAIN * E).any():
        i = tuple(np.argwhere(over > C_CHAIN * E)[0])
        raise AssertionError(f"{what}: element {i}: got {np.asarray(got)[i]}, fp64 {want64[i]:.6g}, beyond the tolerance by {over[i]:.3g} > {C_CHAIN} x E ({E:.3g}); "
                             f"{int((over > C_CHAIN * E).sum())} of {over.size} elements fail")
    return float(over.max()) / E if E > 0 else 0.0


def judge_chain(p, res, what="", cache=None):
    """Holds one result of the chain (device or emulation) to the three stages.  res: qk [band + M + band, H, d] fp16, part [M, nch,
    H, d] / stat [M, nch, H, 2] fp32 (the rows' blocks put together), xctx [M, H d] fp16 or None, ctx [M, ldo] fp16.  Returns the
    largest ratios per stage (tier R)."""
    ref = chain_reference(p, res, cache)
    H, d, M, B = p.H, p.d, p.M, p.band
    qk = np.asarray(res["qk"])[B:B + M]
    part, stat, ctx = res["part"], res["stat"], np.asarray(res["ctx"])
    ratios = {}
    # the chunks a row does not have: never written
    nv, nch = chain_nv(p), part.shape[1]
    dead = np.arange(nch)[None, :] >= nv[:, None]
    fill = res.get("fill_bits", WS_FILL.view(np.uint32))
    assert (part.view(np.uint32)[dead] == fill).all(), f"{what}: partial sums of a chunk beyond a row's own were written"
    mark = np.array(EMPTY_CHUNK, dtype=f32).view(np.uint32)
    assert (stat.view(np.uint32)[dead] == mark).all(), f"{what}: the statistics of a chunk beyond a row's own are not the chunk kernel's empty mark"
    assert np.isfinite(part[~dead]).all() and np.isfinite(stat[~dead]).all(), f"{what}: a chunk of a row was not written (or not finite)"
    pad = ctx[:, 64 * H:]
    assert pad.tobytes() == p.ctx0[:, 64 * H:].tobytes(), f"{what}: a pad column of ctx was written"
    A_, B_, C_ = ref["A"], ref["B"], ref["C"]
    if p.tier == "S":
        _bits_equal(qk, A_["want"], f"{what}: stage A (qk)")
        assert np.isfinite(C_["merged"]).all(), f"{what}: stage B: non-finite merge"
        gap = np.abs(C_["merged"] - B_["want"]).max()
        assert gap <= 2.0 ** -40, f"{what}: stage B: the merged partials are not the winner's row (off by {gap:.3g})"
        if res.get("xctx") is not None:
            _bits_equal(np.asarray(res["xctx"]).reshape(M, H, d), C_["merged"], f"{what}: xctx")
        _bits_equal(ctx[:, :64 * H], C_["want"], f"{what}: stage C (ctx)")
        return ratios
    ratios["A"] = _within(qk, A_["want"], A_["E"], A_["flip"], f"{what}: stage A (qk)")
    assert np.isfinite(C_["merged"]).all(), f"{what}: stage B: non-finite merge of the partials"
    ratios["B"] = _within(C_["merged"], B_["want"], B_["E"], 0.0, f"{what}: stage B (merged partials)", half=False)
    if res.get("xctx") is not None:
        ratios["xctx"] = _within(np.asarray(res["xctx"]).reshape(M, H, d), C_["merged"], C_["Em"], 0.0, f"{what}: xctx")
    ratios["C"] = _within(ctx[:, :64 * H], C_["want"], C_["E"], C_["flip"], f"{what}: stage C (ctx)")
    if "q32" in res:                                             # (the emulation's inner values: the host test's record)
        ratios["q"] = float(np.abs(res["q32"].astype(f64) - A_["q64"]).max()) / max(A_["Eq"], 1e-300)
        ratios["merged"] = float(np.abs(res["merged32"].astype(f64) - C_["merged"]).max()) / max(C_["Em"], 1e-300)
    return ratios
