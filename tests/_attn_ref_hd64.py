"""fp64 reference, fixtures and tolerance model of the Llama-family attention calls at head_dim = 64 (csrc/llama_kernels_hd64.h):
the Llama kinds of tests/_attn_ref.py restated at that width.  Everything that does not depend on the head width is _attn_ref's
and is called, not copied (attend64, emulate_item, the sample, the half ulp, the selector, the sentinel, C); what is written here is
what does: how a call is cut into (sequence or row, head) pieces, the rotation, the cache layout.  Written from the HF semantics
(hf: models/llama/modeling_llama.py apply_rotary_pos_emb, eager_attention_forward, repeat_kv; models/qwen2: the q / k / v bias):

  prefill (kind 4)  q = already-rotated qkv [T, (H + 2 n_kv) 64]: query heads, then key heads, then value heads; per sequence and
                    head P = softmax(64**-0.5 Q K^T + causal mask), ctx = P V; query head h reads kv head h // (H // n_kv).
  step (kind 5)     q = one NOT rotated row per sequence; the row's q and k heads get the bias (fp32), then the rotation at pos[b]
                    (rotate_half pairs element i with i + 32; tables [max_pos][32]), ONE fp16 rounding; the value head gets its bias
                    and one rounding; keys / values 0 .. pos - 1 come from the cache [n_seq][n_kv][P][64] (K, then V), the new ones
                    are used and written at pos; nothing else of the cache changes.

The documented fp32 arithmetic (the yardstick's, not a bit-exact model of a kernel): the rotation is rope_rot's fused form in
rope64_pairs - x = fp32(fp16 row) + fp32 bias (+ 0 without one), lo = fma(cos, x1, -fl(sin x2)), hi = fma(cos, x2, fl(sin x1)), then
fp16 - and attention is _attn_ref.emulate_item's chain: fp32 k-ordered scores, one multiply by the scale, exp2, fp16 probabilities in
the prefill (they are an MFMA operand) and fp32 ones in the step, one fp32 P V chain, one division.

Tolerance: half an fp16 ulp of the expected value + C E, E = the chain emulation's largest error against fp64 on the fixed sample of
the problem's rows.  C = 3, the project's: tests/test_attn_ref_hd64_host.py recomputes the largest (error - half ulp) / E of the
honest summation orders - the chain, online softmax per 64-key tile (the prefill kernel), merge of 128-key chunks, four wave shares
of 32 keys merged in wave order inside every 128-key chunk (the step kernels) - on this module's own fixtures and keeps C = 3 only
while that figure is at most 1.5 (0.99 when this was written).  C was fixed on the CPU before
any kernel ran and is not a function of what a kernel returns."""
import numpy as np

import _attn_ref as A
from _attn_ref import C, SENTINEL, f16, f32, f64   # noqa: F401  (re-exported for the tests)

HD, HALF = 64, 32
LLAMA, STEP = A.LLAMA, A.STEP
SCALE = 64.0 ** -0.5
MUTANTS_PREFILL = ("scale128", "kv_mod", "causal_plus1")
MUTANTS_STEP = ("pair_i64", "scale128", "kv_mod", "stale_pos", "bias_after_rot")


def _rot64(x1, x2, c, s):
    return np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s])


def rope_head(row, c0, cos, sin, bias=None, mut=None, emul=False):
    """Head [64] at column c0 of a step's row after bias and rotation.  fp64, or (emul) the kernels' fp32 form with its ONE fp16
    rounding.  Mutants: "pair_i64" (element i paired with the element 64 further in the row - the 128-wide rule), "bias_after_rot"."""
    w = c0 + (64 if mut == "pair_i64" else HALF)
    late = mut == "bias_after_rot" and bias is not None
    if not emul:
        x = np.asarray(row, dtype=f64).copy()
        if bias is not None and not late:
            x = x + np.asarray(bias, dtype=f64)
        c, s = np.asarray(cos, dtype=f64), np.asarray(sin, dtype=f64)
        y = _rot64(x[c0:c0 + HALF], x[w:w + HALF], c, s)
        return y + np.asarray(bias, dtype=f64)[c0:c0 + HD] if late else y
    x = np.asarray(row, dtype=f16).astype(f32) + (np.asarray(bias, dtype=f32) if bias is not None and not late else f32(0))
    c, s = np.asarray(cos, dtype=f32), np.asarray(sin, dtype=f32)
    x1, x2 = x[c0:c0 + HALF], x[w:w + HALF]
    # fma(c, x1, -fl(s x2)): the product c x1 is exact in fp64, one rounding to fp32 of the sum
    lo = (c.astype(f64) * x1.astype(f64) - (s * x2).astype(f32).astype(f64)).astype(f32)
    hi = (c.astype(f64) * x2.astype(f64) + (s * x1).astype(f32).astype(f64)).astype(f32)
    y = np.concatenate([lo, hi])
    if late:
        y = y + np.asarray(bias, dtype=f32)[c0:c0 + HD]
    return A.f16_sat(y)


def step_cache_views(p, cache):
    half = p.n_seq * p.n_kv * p.P * HD
    c = np.asarray(cache).reshape(-1)
    return c[:half].reshape(p.n_seq, p.n_kv, p.P, HD), c[half:2 * half].reshape(p.n_seq, p.n_kv, p.P, HD)


def items(p, mut=None, emul=False):
    """The (sequence or row, head) pieces of a 64-wide Llama call: the dicts of _attn_ref.items.  Rows are indexed in the WHOLE
    allocation (bands included), so a broken rule reads what a broken kernel would read.  Mutants, each breaking ONE rule:
    "scale128" (128**-0.5), "kv_mod" (kv head h % n_kv), "causal_plus1" (key i + 1 admitted), and for the step "pair_i64",
    "bias_after_rot", "stale_pos" (the cache row behind pos admitted)."""
    B, H, out = p.band, p.H, []
    G, Q, KV = H // p.n_kv, HD * H, HD * p.n_kv
    scale = 128.0 ** -0.5 if mut == "scale128" else SCALE
    if p.kind == LLAMA:
        for b in range(p.n_seq):
            rows = np.arange(B + p.seq_off[b], B + p.seq_off[b + 1])
            keys = np.append(rows, rows[-1] + 1) if mut == "causal_plus1" else rows
            mask = np.arange(len(keys))[None, :] <= np.arange(len(rows))[:, None] + (1 if mut == "causal_plus1" else 0)
            for h in range(H):
                g = h % p.n_kv if mut == "kv_mod" else h // G
                out.append(dict(q=p.q[rows, h * HD:h * HD + HD], k=p.q[keys, Q + g * HD:Q + g * HD + HD], v=p.q[keys, Q + KV + g * HD:Q + KV + g * HD + HD],
                                bias=None, mask=mask, scale=scale, out_rows=rows - B, out_col=h * HD, p16=True))
        return out
    assert p.kind == STEP
    kc, vc = step_cache_views(p, p.cache)
    for b in range(p.n_seq):
        pos, row = int(p.pos[b]), p.q[B + b]
        for h in range(H):
            g = h % p.n_kv if mut == "kv_mod" else h // G
            knew = rope_head(row, Q + g * HD, p.cos[pos], p.sin[pos], p.qkv_bias, mut, emul)
            v0 = Q + KV + g * HD
            if emul:
                vnew = A.f16_sat(row[v0:v0 + HD].astype(f32) + (f32(0) if p.qkv_bias is None else p.qkv_bias[v0:v0 + HD].astype(f32)))
            else:
                vnew = row[v0:v0 + HD].astype(f64) + (0.0 if p.qkv_bias is None else p.qkv_bias[v0:v0 + HD].astype(f64))
            k = np.concatenate([kc[b, g, :pos].astype(knew.dtype), knew[None]])
            v = np.concatenate([vc[b, g, :pos].astype(vnew.dtype), vnew[None]])
            if mut == "stale_pos" and pos + 1 < p.P:
                k, v = np.concatenate([k, kc[b, g, pos + 1:pos + 2].astype(k.dtype)]), np.concatenate([v, vc[b, g, pos + 1:pos + 2].astype(v.dtype)])
            out.append(dict(q=rope_head(row, h * HD, p.cos[pos], p.sin[pos], p.qkv_bias, mut, emul)[None], k=k, v=v, bias=None, mask=None, scale=scale,
                            out_rows=np.array([b]), out_col=h * HD, p16=False, new=(b, g, pos, knew, vnew)))
    return out


def expected64(p, mut=None):
    """fp64 context rows [out rows, ldctx], NaN where the call writes nothing."""
    out = np.full((p.out_rows, p.ldctx), np.nan)
    for it in items(p, mut):
        out[it["out_rows"], it["out_col"]:it["out_col"] + HD] = A.attend64(it)
    return out


def expected_cache(p, emul=False, mut=None):
    """The cache after a step: the new key and value at pos, nothing else changed.  fp64 (emul: the kernels' fp16 rows).
    Mutant "write_pos1": the new key and value written at pos + 1."""
    kc, vc = step_cache_views(p, p.cache.astype(f16 if emul else f64))
    kc, vc = kc.copy(), vc.copy()
    for it in items(p, None, emul):
        b, g, pos, knew, vnew = it["new"]
        at = min(pos + 1, p.P - 1) if mut == "write_pos1" else pos
        kc[b, g, at], vc[b, g, at] = knew, vnew
    return np.concatenate([kc.reshape(-1), vc.reshape(-1)])


def _waves(it, chunk=128, share=32):
    """The step kernels' order in fp32: per 128-key chunk four wave shares of 32 keys, each with its own maximum, sum and accumulator,
    merged in wave order under the chunk's maximum (fma), then the chunks merged in key order under the row's maximum (fma)."""
    assert it["mask"] is None and not it["p16"]           # the step's pieces: every key a row holds is admitted
    q, k, v = it["q"].astype(f32), it["k"].astype(f32), it["v"].astype(f32)
    s = (A._chain(q[:, None, :] * k[None, :, :], 2) * f32(it["scale"])).astype(f32)
    nq, nk = s.shape

    def merge(parts):
        g = np.max([m for m, _, _ in parts], axis=0)
        den, acc = np.zeros(nq, dtype=f32), np.zeros((nq, v.shape[1]), dtype=f32)
        for m, l, a in parts:
            w = A._exp2(m - g)
            den = (l.astype(f64) * w.astype(f64) + den.astype(f64)).astype(f32)
            acc = (a.astype(f64) * w[:, None].astype(f64) + acc.astype(f64)).astype(f32)
        return g, den, acc

    chunks = []
    for c0 in range(0, nk, chunk):
        shares = []
        for t0 in range(c0, min(c0 + chunk, nk), share):
            st = s[:, t0:t0 + share]
            m = st.max(axis=1)
            e = A._exp2(st - m[:, None])
            shares.append((m, A._chain(e, 1), A._chain(e[:, :, None] * v[None, t0:t0 + share], 1)))
        chunks.append(merge(shares))
    _, den, acc = merge(chunks)
    return acc / den[:, None]


def emulated(p, order="chain", tile=64, mut=None):
    """What a kernel of the documented arithmetic returns: fp16 [out rows, ldctx] over the pre-filled output.  order: _attn_ref's
    "chain" / "online" / "flash", or "waves" (the step kernels' two-level merge)."""
    out = p.out.copy()
    for it in items(p, mut, emul=True):
        y = _waves(it) if order == "waves" else A.emulate_item(it, order, tile)
        out[it["out_rows"], it["out_col"]:it["out_col"] + HD] = A.f16_sat(y)
    return out


def emulated_cache(p, mut=None):
    return expected_cache(p, emul=True, mut=mut).astype(f16)


def yardstick(p):
    """E of the problem: the chain emulation's largest error against fp64 on the fixed sample (computed once per problem)."""
    if getattr(p, "_E64", None) is None:
        worst = 0.0
        for ref, em in zip(items(p), items(p, emul=True)):
            rows = A._sample(em["q"].shape[0])
            worst = max(worst, float(np.abs(A.emulate_item(em, rows=rows).astype(f64) - A.attend64(ref)[rows]).max()))
        p._E64 = worst
    return p._E64


def miss(p, got):
    """The largest (error - half ulp) / E of `got` over the elements the call owns, without judging (inf for a non-finite one)."""
    if getattr(p, "_want64", None) is None:
        p._want64 = expected64(p)
    want = p._want64
    written = ~np.isnan(want)
    g = np.asarray(got)[written].astype(f64)
    if not np.isfinite(g).all():
        return float("inf")
    E = yardstick(p)
    return float((np.abs(g - want[written]) - A.half_ulp16(want[written])).max()) / E if E > 0 else float("inf")


def judge(p, got, what=""):
    """Holds `got` [out rows, ldctx] fp16 (the interior of a kernel's output) to the problem: tier S bit for bit, tier R within half
    an fp16 ulp + C E; what the call does not own must be what the caller put there.  Returns the largest (error - half ulp) / E
    (0.0 for tier S)."""
    if getattr(p, "_want64", None) is None:
        p._want64 = expected64(p)
    want = p._want64
    written = ~np.isnan(want)
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == f16
    stale = ~written & (got.view(np.uint16) != p.out.view(np.uint16))
    assert not stale.any(), f"{what}: output element {tuple(np.argwhere(stale)[0])} is not the call's to write"
    assert np.isfinite(got[written].astype(f64)).all(), f"{what}: non-finite output"
    if p.tier == "S":
        bad = written & (got.view(np.uint16) != A.f16_sat(np.where(written, want, 0.0)).view(np.uint16))
        if bad.any():
            i, j = np.argwhere(bad)[0]
            raise AssertionError(f"{what}: output row {i}, column {j} (head {j // HD}): got {got[i, j]}, the selected row has {want[i, j]}")
        return 0.0
    E = yardstick(p)
    err = np.where(written, np.abs(got.astype(f64) - np.where(written, want, 0.0)), 0.0)
    over = err - np.where(written, A.half_ulp16(np.where(written, want, 1.0)), 0.0)
    if (over > C * E).any():
        i, j = np.argwhere(over > C * E)[0]
        raise AssertionError(f"{what}: output row {i}, column {j} (head {j // HD}): got {got[i, j]}, fp64 {want[i, j]:.6g}, error {err[i, j]:.3g} > "
                             f"half ulp {A.half_ulp16(want[i, j]):.3g} + {C} x E ({E:.3g})")
    return float(over.max()) / E if E > 0 else 0.0


def judge_cache(p, got, what=""):
    """The cache after a step (interior, flat fp16): exactly row pos of K and of V of every kv head may differ from what the caller
    put there, everything else bit for bit; the appended key within half an ulp of the fp64 rotation + the fp32 rotation's own
    error (exactly it in tier S: identity tables, integer operands), the appended value likewise."""
    want, em = expected_cache(p), expected_cache(p, emul=True).astype(f64)
    got = np.asarray(got).reshape(-1)
    assert got.size == want.size and got.dtype == f16
    new = np.zeros(got.size, dtype=bool)
    half = got.size // 2
    for b in range(p.n_seq):
        for g in range(p.n_kv):
            o = ((b * p.n_kv + g) * p.P + int(p.pos[b])) * HD
            new[o:o + HD] = new[half + o:half + o + HD] = True
    stale = ~new & (got.view(np.uint16) != p.cache.reshape(-1).view(np.uint16))
    assert not stale.any(), f"{what}: cache element {np.argwhere(stale)[0][0]} changed and is not an appended row"
    if p.tier == "S":
        assert (got[new].view(np.uint16) == A.f16_sat(want[new]).view(np.uint16)).all(), f"{what}: the appended key / value rows are not the new row's"
        return
    e = float(np.abs(em[new] - want[new]).max())          # includes the emulation's own fp16 rounding: at least what a kernel may add
    err = np.abs(got[new].astype(f64) - want[new])
    assert (err <= A.half_ulp16(want[new]) + e).all(), f"{what}: appended row off by {err.max():.3g}"


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def build_llama(seed, H, n_kv, lens, tier, *, band=8, pad=(0, 0), flat=False):
    """Causal prefill: already-rotated qkv [T, (H + 2 n_kv) 64 + pad].  Tier S: _attn_ref.build_llama's selector design at width 64 (a
    query is a copy of its winner's key row: winners at the query's own key, the first key, the key before, the first key of the
    query's 64-key tile; traps - copies of the winner - in the row behind the query, at the diagonal, at the sequence end and at
    every 64-key edge, and in the row before every sequence).  Tier R: N(0, 1); flat: the queries / 16 (long flat averages)."""
    rs = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, Q, KV, G = int(off[-1]), HD * H, HD * n_kv, H // n_kv
    ldq, ldctx = Q + 2 * KV + pad[0], Q + pad[1]
    q = A._rows_buffer(rs, T, ldq, band, tier, amp=8)
    p = A.problem(LLAMA, H=H, n_kv=n_kv, n_seq=len(lens), seq_off=off, band=band, ldq=ldq, ldctx=ldctx, out_rows=T, tier=tier, p16=True)
    if tier == "S":
        q[:, Q + KV:Q + 2 * KV] = A._int_values(rs, (T + 2 * band, KV))
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
            K, win, placed = A.selector(rs, T + 2 * band, HD, 8, queries, traps, scale=SCALE, what=f"llama64 kv head {g}")
            p.n_traps += len(placed)
            q[:, Q + g * HD:Q + g * HD + HD] = K
            n = 0
            for b, L in enumerate(lens):
                for r in range(G):
                    h = g * G + r
                    q[band + off[b]:band + off[b + 1], h * HD:h * HD + HD] = K[win[n:n + L]]
                    n += L
    elif flat:
        q[:, :Q] = (q[:, :Q].astype(f32) / 16).astype(f16)
    p.q, p.out = q, A.sentinel16((T, ldctx))
    return p


def alone(p, b):
    """Sequence b of a prefill problem as a call of its own: the same rows (its neighbours become band rows)."""
    lo, hi = int(p.seq_off[b]), int(p.seq_off[b + 1])
    s = A.problem(LLAMA, H=p.H, n_kv=p.n_kv, n_seq=1, seq_off=np.array([0, hi - lo], dtype=np.int32), band=p.band, ldq=p.ldq, ldctx=p.ldctx,
                  out_rows=hi - lo, tier=p.tier, p16=True)
    s.q = np.ascontiguousarray(p.q[lo:hi + 2 * p.band])
    s.out = A.sentinel16((hi - lo, p.ldctx))
    return s


def rope_tables(max_pos, theta=10000.0):
    inv = theta ** (-np.arange(HALF, dtype=f64) / HALF)
    ang = np.arange(max_pos, dtype=f64)[:, None] * inv[None, :]
    return np.cos(ang).astype(f32), np.sin(ang).astype(f32)


def build_step(seed, H, n_kv, pos, P, tier, *, bias=False, band=8):
    """Cached step: one new row per sequence at pos[b] over a cache of P positions.  Tier S: identity rotary tables, integer operands
    (_attn_ref.build_step's design at width 64: winners at the new key, the first key, the key before and both sides of every
    128-key chunk edge; the stale cache row at pos would lose, the row behind pos is a trap)."""
    rs = np.random.RandomState(seed)
    n_seq, Q, KV, G = len(pos), HD * H, HD * n_kv, H // n_kv
    ldq = Q + 2 * KV
    q = A._rows_buffer(rs, n_seq, ldq, band, tier, amp=8)
    p = A.problem(STEP, H=H, n_kv=n_kv, n_seq=n_seq, P=P, pos=np.asarray(pos, dtype=np.int32), band=band, ldq=ldq, ldctx=Q, out_rows=n_seq, tier=tier, p16=False)
    if tier == "S":
        p.cos, p.sin = np.ones((P, HALF), dtype=f32), np.zeros((P, HALF), dtype=f32)
        kc = np.zeros((n_seq, n_kv, P, HD), dtype=f16)
        vc = A._int_values(rs, (n_seq, n_kv, P, HD))
        q[:, Q + KV:] = A._int_values(rs, (q.shape[0], KV))
        for b in range(n_seq):
            for g in range(n_kv):
                t = int(pos[b])
                sp = [k for k in [t, 0, t - 1] + A.edges_of(t + 1, 128) if 0 <= k <= t]
                queries = [(range(0, t + 1), [sp[(r + g + b) % len(sp)]]) for r in range(G)]
                K, win, placed = A.selector(rs, P, HD, 8, queries, [(0, t + 1)], scale=SCALE, what=f"step64 row {b} kv head {g}")
                p.n_traps += len(placed)
                kc[b, g] = K
                q[band + b, Q + g * HD:Q + g * HD + HD] = K[t]              # the new key comes from the row ...
                kc[b, g, t] = -K[t]                                        # ... the stale cache row at pos would lose
                for r in range(G):
                    q[band + b, (g * G + r) * HD:(g * G + r) * HD + HD] = K[win[r]]
        if bias:                                                          # integer bias, row entries shifted so that row + bias is the design
            p.qkv_bias = rs.randint(-3, 4, size=ldq).astype(f32)
            q[band:band + n_seq] = (q[band:band + n_seq].astype(f32) - p.qkv_bias).astype(f16)
        p.cache = np.concatenate([kc.reshape(-1), vc.reshape(-1)])
    else:
        p.cos, p.sin = rope_tables(P)
        p.cache = rs.standard_normal(2 * n_seq * n_kv * P * HD).astype(f16)
        if bias:                                                          # Qwen2: q / k biases of a few units, outliers among them
            p.qkv_bias = (rs.standard_normal(ldq) * np.where(rs.rand(ldq) < 0.02, 8.0, 0.5)).astype(f32)
    p.q, p.out = q, A.sentinel16((n_seq, Q))
    return p


def row_alone(p, b):
    """Row b of a step problem as a call of its own: its row (the neighbours become band rows), its cache rows, its position."""
    s = A.problem(STEP, H=p.H, n_kv=p.n_kv, n_seq=1, P=p.P, pos=p.pos[b:b + 1].copy(), band=p.band, ldq=p.ldq, ldctx=p.ldctx, out_rows=1, tier=p.tier,
                  p16=False, cos=p.cos, sin=p.sin, qkv_bias=p.qkv_bias)
    s.q = np.ascontiguousarray(p.q[b:b + 1 + 2 * p.band])
    kc, vc = step_cache_views(p, p.cache)
    s.cache = np.concatenate([kc[b].reshape(-1), vc[b].reshape(-1)])
    s.out = A.sentinel16((1, p.ldctx))
    return s
