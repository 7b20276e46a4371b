"""fp64 reference of the row kernels and device state machines (csrc/misc_kernels.h, the rope and cache-fill kernels of
csrc/llama_kernels.h and csrc/llama_kernels_hd64.h), the fixtures their tests run and the tolerance model they use.  Plain numpy;
everything is written from the HF semantics the kernel comments quote - never from a kernel:

  embed          hidden[t] = (fp32) E[ids[t]]; folded-norm form: the row also as fp16 x 2^-4 and its factor rsqrt(mean(x^2) + eps) / xs
  rowscale       the same factor from block sums of squares: rsqrt(sum_j ssq[j] / d + eps) / xs
  rmsnorm        y = w x rsqrt(mean(x^2) + eps) out_scale (T5LayerNorm / LlamaRMSNorm), fp16 result saturating at +-65504; out row r
                 reads x row row_map[r]
  head_rows      out[b][j] = x[b] . head[out_ids[j]]
  pair_verdict   logits of (false, true) per sequence, P(true) = two-way softmax, verdict P(true)[2p] > P(true)[2p + 1] (a tie is 0)
  argmax_blocks  torch.argmax over (block maximum, its first column) pairs: the smallest column among the maxima
  qlm_lse        out[b] = -sum_t (logsumexp_t - xlab[b, t]), logsumexp_t = M + log(sum_blocks s exp(m - M))
  rope           apply_rotary_pos_emb on the H + n_kv query and key heads of a fused q | k | v row (rotate_half pairs i with
                 i + hd / 2), after the optional Qwen2 bias, which the value heads get too; ONE fp16 rounding
  kv_fill        cache K [row][kv head][t][hd] (then V) = the key (value) heads of token t of the sequence the row belongs to
  advance        the three greedy state machines (`GreedyMachine`, `LlamaMachine`, `SessionMachine` below)

A call is a `Problem` (SimpleNamespace: the operands as the debug entry takes them).  `expected(p)` is the fp64 (or exact) result,
`emulated(p, order)` the documented fp32 arithmetic in one honest order; the mutants of tests/test_rows_ref_host.py break one
rule of `expected` each (`expected(p, mut=...)`).

Exact tiers (bit for bit).  embed: out is the fp16 row widened, xraw the row times 2^-4 - one exact scaling, correctly rounded
where the product is subnormal in fp16.  kv_fill, argmax_blocks, advance: everything.  head_rows / pair_verdict logits: small
integer operands, exact in any summation order; the verdict kernel's logits equal head_rows' bytes.  rmsnorm: eps = 1 / 2 and rows
of integers whose mean square is 4^k - 1 / 2 (k = 0, 1, 2 by row), power-of-two weights that differ by column and a power-of-two
out_scale: rsqrt(4^k) is exact and so is every product.  rope: tables from {(1, 0), (0, 1), (0, -1), (-1, 0)} chosen per position
and column, integer inputs and biases: a signed permutation.

Random tier, against fp64.  An fp16 output may be off by half an fp16 ulp of the expected value plus C_ROWS x E; an fp32 output
by C_ROWS x E.  E is the error against fp64 of `emulated(p, "lanes")` - the arithmetic the kernel comments document: per-lane
chains in the kernel's column order, the xor-butterfly over 64 lanes, correctly rounded rsqrt / exp / log - on the very problem,
BEFORE the final fp16 rounding:
  rope (fp16): absolute, the largest error of the output row (a rotated element is a difference: no relative figure holds);
  rmsnorm (fp16): relative, the largest |error / expected| of the output row - its elements share one factor and differ in
    scale by orders of magnitude with the weights - and never less than 2^-24;
  fp32 outputs (row factors, qlm scores): relative, the largest |error / expected| of the problem, and never less than 2^-24 - the
    rounding of the result itself, which a single-row problem may happen to get exactly right.
Head logits on N(0, 1) operands keep the tau = 4 E32 of tests/_gemm_ref.py, P(true) the 1e-6 of tests/test_gpu_pair_verdict.py
(derived there), judged against the fp64 softmax of the device's own logits.

C_ROWS, measured on the CPU (tests/test_rows_ref_host.py::test_honest_orders_pass_and_c_rows recomputes it and fails when it
differs): the honest orders stand in for the kernel on the fixtures of tests/test_gpu_rows.py (`FIXTURES`) - "lanes" itself, one
plain chain, pairwise, each also with the rsqrt / log result moved one fp32 ulp up and down (hardware rsqrt and log are good to one
ulp, numpy's are correctly rounded), the rotation fused (one fma over a rounded product) and unfused, qlm's block merge lane-strided,
chained and pairwise.  Largest (error - half ulp) / E over whole outputs:
  embed rowscale 3.54     rowscale 2.19   rmsnorm 3.62   rope 0.16   qlm_lse 2.67
(the row factors are dominated by the one-ulp rsqrt on top of a result whose own rounding is the floor of E; rope by its
half ulp, next to which the fp32 orders hardly differ).  The largest is 3.62; C_ROWS is twice that, rounded up to
a tenth: 7.3.  The mutants of the host test fail by orders of magnitude
more: C_ROWS is not what separates them.
"""
from types import SimpleNamespace

import numpy as np

import _attn_ref as A
import _gemm_ref as G

f16, f32, f64 = np.float16, np.float32, np.float64
f16_sat, half_ulp16, SENTINEL, F16_MAX, XS = A.f16_sat, A.half_ulp16, A.SENTINEL, A.F16_MAX, G.XS
U24 = 2.0 ** -24
C_ROWS = 7.3
P_TOL = 1e-6                      # tests/test_gpu_pair_verdict.py: two expf, one add, one divide on values <= 1, doubled
OPS = {"embed": 1, "rowscale": 2, "rmsnorm": 3, "head_rows": 4, "pair_verdict": 5, "argmax_blocks": 6, "qlm_lse": 7, "rope": 8,
       "kv_fill": 9, "advance": 10}
INT_MAX = 0x7FFFFFFF


def problem(op, **kw):
    p = SimpleNamespace(op=op, tier="R", row_map=None, row_off=None, out_idx=None, bias=None, slots=None, n_slots=0, fold=1)
    p.__dict__.update(kw)
    for k in ("eps", "xs", "out_scale"):                     # the call carries them as fp32: the reference reads the same numbers
        if k in p.__dict__:
            setattr(p, k, float(f32(getattr(p, k))))
    return p


# ---- plans: the grid / template rule of every launcher, restated -----------------------------------------------------------------
def plan(p):
    """(grid, tparam, variant) the launcher of the op must choose."""
    op = p.op
    if op == "embed":
        return ((p.rows + 3) // 4, 1, 1), 0, int(bool(p.fold))
    if op == "rowscale":
        return ((p.rows + 255) // 256, 1, 1), 0, 0
    if op == "rmsnorm":
        return ((p.rows + 3) // 4, 1, 1), 4 if p.d <= 1024 else (8 if p.d <= 2048 else 16), 0
    if op == "head_rows":
        return ((p.rows * p.n_out + 3) // 4, 1, 1), 0, 0
    if op == "pair_verdict":
        return (p.rows // 2, 1, 1), 0, 0
    if op in ("argmax_blocks", "qlm_lse"):
        return (p.rows, 1, 1), 0, 0
    if op == "rope":
        return (p.rows, 1, 1), p.hd, int(p.bias is not None)
    if op == "kv_fill":
        return (int(np.diff(p.seq_off).max()), p.rows, 1), p.hd, int(p.slots is not None)
    return (1, 1, 1), 0, p.kind


# ---- fp32 building blocks of the emulation ------------------------------------------------------------------------------------------
def _chain32(v):
    return np.cumsum(np.asarray(v, dtype=f32), dtype=f32)[-1] if len(v) else f32(0)


def _pairwise32(v):
    v = np.asarray(v, dtype=f32)
    if len(v) == 0:
        return f32(0)
    while len(v) > 1:
        if len(v) % 2:
            v = np.concatenate([v, np.zeros(1, f32)])
        v = (v[0::2] + v[1::2]).astype(f32)
    return v[0]


def _butterfly32(lanes):
    """wave_sum: v += shfl_xor(v, o) for o = 32, 16, ... 1 over 64 lanes; every lane ends with the same sum."""
    v = np.asarray(lanes, dtype=f32).copy()
    idx = np.arange(64)
    o = 32
    while o:
        v = (v + v[idx ^ o]).astype(f32)
        o >>= 1
    return v[0]


def _sum32(terms, order, lane_of):
    """Sum of fp32 terms: "lanes" = per-lane chains (lane_of[i] = the lane of term i, terms in the lane's order) + butterfly."""
    terms = np.asarray(terms, dtype=f32)
    if order == "chain":
        return _chain32(terms)
    if order == "pairwise":
        return _pairwise32(terms)
    lanes = np.zeros(64, f32)
    for l in range(64):
        lanes[l] = _chain32(terms[lane_of == l])
    return _butterfly32(lanes)


def _nudge(x, ulps):
    x = f32(x)
    for _ in range(abs(ulps)):
        x = np.nextafter(x, f32(np.inf if ulps > 0 else -np.inf), dtype=f32)
    return x


def _rsqrt32(x, nudge=0):
    return _nudge(f32(1.0 / np.sqrt(f64(f32(x)))), nudge)


# ---- embed ----------------------------------------------------------------------------------------------------------------------
def _embed_ids(p, mut=None):
    return np.clip(p.ids, 0, p.vocab - 1)


def embed_expected(p, mut=None):
    rows = p.table[_embed_ids(p)]                         # fp16 [rows, d]
    x = rows.astype(f64)
    ms = (x * x).mean(axis=1)
    if mut == "no_eps":
        fac = 1.0 / np.sqrt(np.where(ms > 0, ms, 1.0)) / p.xs
    elif mut == "times_xs":
        fac = 1.0 / np.sqrt(ms + p.eps) * p.xs
    else:
        fac = 1.0 / np.sqrt(ms + p.eps) / p.xs
    return {"out": rows.astype(f32), "xraw": (rows.astype(f32) * f32(p.xs)).astype(f16), "rowscale": fac}


def embed_emulated(p, order="lanes", nudge=0):
    x = p.table[_embed_ids(p)].astype(f32)
    c = np.arange(p.d)
    lane_of = (c % 512) // 8                               # lane l takes columns l*8 .. l*8+7 of every 512-column pass
    out = np.zeros(p.rows, f32)
    for r in range(p.rows):
        ss = _sum32(x[r] * x[r], order, lane_of)
        out[r] = f32(_rsqrt32(f32(f32(ss / f32(p.d)) + f32(p.eps)), nudge) / f32(p.xs))
    return {"rowscale": out}


# ---- rowscale -------------------------------------------------------------------------------------------------------------------
def rowscale_expected(p, mut=None):
    s = p.ssq.astype(f64).sum(axis=1)
    return {"out": 1.0 / np.sqrt(s / p.d + p.eps) / p.xs}


def rowscale_emulated(p, order="lanes", nudge=0):
    out = np.zeros(p.rows, f32)
    for r in range(p.rows):
        s = _pairwise32(p.ssq[r]) if order == "pairwise" else _chain32(p.ssq[r])     # the kernel: blocks added in increasing order
        out[r] = f32(_rsqrt32(f32(f32(s / f32(p.d)) + f32(p.eps)), nudge) / f32(p.xs))
    return {"out": out}


# ---- rmsnorm --------------------------------------------------------------------------------------------------------------------
def rmsnorm_expected(p, mut=None):
    src = np.arange(p.rows) if (p.row_map is None or mut == "row_map_ignored") else np.asarray(p.row_map)
    x = p.x[src].astype(f64)
    w = p.w.astype(f64)
    if mut == "weight_c4":
        w = np.roll(w, -4)
    ms = (x[:, :4096] ** 2).sum(axis=1) / p.d if mut == "first_4096" else (x * x).mean(axis=1)
    rs = 1.0 / np.sqrt(ms + p.eps)
    if mut == "round_before_scale":
        y = f16_sat(x * rs[:, None] * w).astype(f64) * p.out_scale
    else:
        y = x * (rs * p.out_scale)[:, None] * w
    if mut == "first_4096":
        y[:, 4096:] = np.nan                                 # never written
    if mut == "inf":
        y = np.where(y > F16_MAX, np.inf, np.where(y < -F16_MAX, -np.inf, y))
    return {"out": y}


def rmsnorm_emulated(p, order="lanes", nudge=0):
    src = np.arange(p.rows) if p.row_map is None else np.asarray(p.row_map)
    x = p.x[src].astype(f32)
    c = np.arange(p.d)
    lane_of = (c % 256) // 4
    out = np.zeros((p.rows, p.d), f32)
    for r in range(p.rows):
        ss = _sum32(x[r] * x[r], order, lane_of)
        rs = f32(_rsqrt32(f32(f32(ss / f32(p.d)) + f32(p.eps)), nudge) * f32(p.out_scale))
        out[r] = (x[r] * rs).astype(f32) * p.w.astype(f32)
    return {"out": out}


# ---- head rows and the pair verdict -----------------------------------------------------------------------------------------------
def head_expected(p, mut=None):
    ids = np.asarray(p.out_ids)
    if mut == "next_id":
        ids = np.roll(ids, -1)
    x, h = p.x.astype(f64), p.head[ids].astype(f64)
    if mut == "first_512":
        x, h = x[:, :512], h[:, :512]
    return {"out": x @ h.T}


def softmax_true(logits, mut=None):
    """P(true) of [n, 2] = (false, true) logits, max-subtracted two-way softmax in fp64."""
    lg = np.asarray(logits, dtype=f64)
    m = lg.max(axis=1)
    ef, et = np.exp(lg[:, 0] - m), np.exp(lg[:, 1] - m)
    return (ef if mut == "swapped" else et) / (ef + et)


def verdict_expected(p, logits=None, p_true=None, mut=None):
    """logits [n_seq, 2] fp64 (or the given ones), P(true), verdict per pair from the given P(true) (the device's own bytes when
    judging: the comparison is exact) - strict: a tie is 0."""
    if logits is None:
        logits = head_expected(problem("head_rows", x=p.x, head=p.head, out_ids=[p.false_id, p.true_id]))["out"]
    n = p.rows // 2 * 2
    pt = softmax_true(logits[:n], mut) if p_true is None else np.asarray(p_true)[:n]
    win = (pt[0::2] >= pt[1::2]) if mut == "tie_ge" else (pt[0::2] > pt[1::2])
    return {"logits": logits[:n], "p_true": pt, "verdict": win.astype(f32)}


# ---- argmax over blocks ------------------------------------------------------------------------------------------------------------
def argmax_expected(p, mut=None):
    out = np.zeros(p.rows, np.int32)
    for r in range(p.rows):
        v, i = p.bval[r], p.bidx[r]
        if mut == "wave_order":
            best, bi = f32(-np.inf), INT_MAX
            for w in range(4):                               # per wave the right rule, across waves the first wave wins a tie
                sel = (np.arange(p.nb) % 256) // 64 == w
                if sel.any():
                    m = v[sel].max()
                    mi = i[sel][v[sel] == m].min()
                    if m > best or bi == INT_MAX:
                        best, bi = m, mi
            out[r] = bi
            continue
        cand = i[v == v.max()]
        out[r] = cand.max() if mut == "last_tie" else cand.min()
    return {"out": out}


# ---- qlm log-sum-exp -------------------------------------------------------------------------------------------------------------------
def _qlm_rows(p, b, mut=None):
    if p.row_off is not None and mut != "row_off_ignored":
        return range(int(p.row_off[b]), int(p.row_off[b + 1]))
    n_pos = p.n_pos if p.row_off is None else int(np.diff(p.row_off).max())
    return range(b * n_pos, min((b + 1) * n_pos, len(p.xlab)))


def qlm_expected(p, mut=None):
    out = np.zeros(p.rows, f64)
    st = p.stats.astype(f64)
    for b in range(p.rows):
        total = 0.0
        for row in _qlm_rows(p, b, mut):
            m, s = st[row, :, 0], st[row, :, 1]
            M = m.max()
            se = s.sum() if mut == "no_rescale" else (s * np.exp(m - M)).sum()
            total += (M + np.log(se)) - f64(p.xlab[row])
        dst = b if (p.out_idx is None or mut == "out_idx_ignored") else int(p.out_idx[b])
        out[dst] = total if mut == "sign" else -total
    return {"out": out}


def qlm_emulated(p, order="lanes", nudge=0):
    out = np.zeros(p.rows, f32)
    tid = np.arange(p.nb) % 256
    for b in range(p.rows):
        total = f32(0)
        for row in _qlm_rows(p, b):
            m, s = p.stats[row, :, 0].astype(f32), p.stats[row, :, 1].astype(f32)
            M = m.max()
            with np.errstate(invalid="ignore"):
                terms = (s * np.exp((m - M).astype(f32), dtype=f32)).astype(f32)
            if order == "lanes":                             # thread-strided chains, a butterfly per wave, the four waves in order
                waves = []
                for w in range(4):
                    lanes = np.zeros(64, f32)
                    for l in range(64):
                        lanes[l] = _chain32(terms[tid == w * 64 + l])
                    waves.append(_butterfly32(lanes))
                se = _chain32(waves)
            else:
                se = _sum32(terms, order, None)
            lse = f32(M + _nudge(np.log(f32(se), dtype=f32), nudge))
            total = f32(total + f32(lse - f32(p.xlab[row])))
        out[b if p.out_idx is None else int(p.out_idx[b])] = -total
    return {"out": out}


# ---- rope --------------------------------------------------------------------------------------------------------------------------
def rope_expected(p, mut=None):
    """qkv [T, ld] fp16 -> fp64 [T, ld]: rotated query / key heads, biased value heads, pad columns as they were."""
    hd, half, H, n_kv = p.hd, p.hd // 2, p.H, p.n_kv
    out = p.qkv.astype(f64).copy()
    n_rot = H + n_kv
    touched = np.zeros(out.shape, bool)
    for t in range(p.rows):
        tr = int(p.pos[t]) if mut != "row_t" else t
        if mut == "pos_plus1":
            tr = min(tr + 1, p.cos.shape[0] - 1)
        c, s = p.cos[tr].astype(f64), p.sin[tr].astype(f64)
        if mut == "sin_sign":
            s = -s
        for h in range(n_rot):
            if mut == "keys_not_rotated" and h >= H:
                continue
            x = out[t, h * hd:(h + 1) * hd].copy()
            bh = (h + 1) % n_rot if mut == "bias_next_head" else h
            b = None if p.bias is None else p.bias[bh * hd:(bh + 1) * hd].astype(f64)
            if b is not None and mut != "bias_after":
                x = x + b
            x1, x2 = x[:half], x[half:]
            if mut == "partner_quarter":                      # pairs i with i + hd / 4 inside each half
                q = hd // 4
                y = x.copy()
                for base in (0, half):
                    a1, a2 = x[base:base + q], x[base + q:base + 2 * q]
                    y[base:base + q] = a1 * c[:q] - a2 * s[:q]
                    y[base + q:base + 2 * q] = a2 * c[:q] + a1 * s[:q]
            else:
                y = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s])
            if b is not None and mut == "bias_after":
                y = y + b
            out[t, h * hd:(h + 1) * hd] = y
            touched[t, h * hd:(h + 1) * hd] = True
        if p.bias is not None and mut != "values_no_bias":
            lo, hi = n_rot * hd, (n_rot + n_kv) * hd
            out[t, lo:hi] += p.bias[lo:hi].astype(f64)
            touched[t, lo:hi] = True
    return {"out": out, "touched": touched}


def rope_emulated(p, order="lanes", nudge=0):
    """The kernels' arithmetic: fp32 bias add, fp32 products; order "lanes" = as documented (with bias: element 0 of a thread's eight
    fused, the rest unfused; without: unfused), "chain" = everything unfused, "pairwise" = everything fused."""
    hd, half, H, n_kv = p.hd, p.hd // 2, p.H, p.n_kv
    out = p.qkv.astype(f32).copy()
    n_rot = H + n_kv
    j0 = np.arange(half) % 8 == 0
    fused = np.ones(half, bool) if order == "pairwise" else (j0 if (order == "lanes" and p.bias is not None) else np.zeros(half, bool))
    for t in range(p.rows):
        c, s = p.cos[int(p.pos[t])].astype(f32), p.sin[int(p.pos[t])].astype(f32)
        for h in range(n_rot):
            x = out[t, h * hd:(h + 1) * hd]
            if p.bias is not None:
                x = (x + p.bias[h * hd:(h + 1) * hd].astype(f32)).astype(f32)
            x1, x2 = x[:half], x[half:]
            lo_u = ((c * x1).astype(f32) - (s * x2).astype(f32)).astype(f32)
            hi_u = ((c * x2).astype(f32) + (s * x1).astype(f32)).astype(f32)
            lo_f = (c.astype(f64) * x1 - (s * x2).astype(f32).astype(f64)).astype(f32)
            hi_f = (c.astype(f64) * x2 + (s * x1).astype(f32).astype(f64)).astype(f32)
            out[t, h * hd:(h + 1) * hd] = np.concatenate([np.where(fused, lo_f, lo_u), np.where(fused, hi_f, hi_u)])
        if p.bias is not None:
            lo, hi = n_rot * hd, (n_rot + n_kv) * hd
            out[t, lo:hi] = (out[t, lo:hi] + p.bias[lo:hi].astype(f32)).astype(f32)
    return {"out": out}


# ---- kv fill ---------------------------------------------------------------------------------------------------------------------
def kv_fill_expected(p, mut=None):
    """The cache (flat fp16, K [rows][n_kv][P][hd] then V) after the fill, from its pre-fill."""
    hd, H, n_kv, P = p.hd, p.H, p.n_kv, p.P
    n_rows = p.n_slots if p.slots is not None else p.rows
    cache = p.cache.copy().reshape(2, n_rows, n_kv, P, hd)
    kstride = H if mut == "stride_H" else n_kv
    for b in range(p.rows):
        slot = b if (p.slots is None or mut == "slots_ignored") else int(p.slots[b])
        if slot < 0 or slot >= n_rows:
            continue
        L = int(p.seq_off[b + 1] - p.seq_off[b])
        for t in range(min(L, P)):
            tok = int(p.seq_off[b]) + t + (1 if mut == "row_plus1" else 0)
            tok = min(tok, p.qkv.shape[0] - 1)
            row = p.qkv[tok]
            for h in range(n_kv):
                k = row[(H + h) * hd:(H + h + 1) * hd]
                vcol = (H + kstride + h) * hd
                v = row[vcol:vcol + hd] if vcol + hd <= row.size else np.zeros(hd, f16)
                if mut == "kv_swapped":
                    k, v = v, k
                cache[0, slot, h, t] = k
                cache[1, slot, h, t] = v
    return {"out": cache.reshape(-1)}


# ---- the three advance machines --------------------------------------------------------------------------------------------------------
class GreedyMachine:
    """rk_t5_generate's token feedback.  st = {t, finished step, eos, pad}: the decoder just ran input position t.  Prefix positions
    (t + 1 < dec_len) are forced; otherwise column n = t + 1 - dec_len gets the arg-max, or pad once the row has finished; EOS
    finishes a row; the token is the next input.  st[1] (0 until then) = n + 1 at the column where the last row finished, or max_new.
    The position advances, held at dec_len + max_new - 1: a step after the end writes nothing but pads over pads."""

    def __init__(self, st, prefix, done, out, next_ids, dec_len, max_new, mut=None):
        self.st, self.prefix, self.done, self.out, self.next = (np.array(a, np.int32) for a in (st, prefix, done, out, next_ids))
        self.out = self.out.reshape(len(self.done), max_new)
        self.dec_len, self.max_new, self.mut = dec_len, max_new, mut

    def step(self, argmax):
        t, eos, pad = int(self.st[0]), int(self.st[2]), int(self.st[3])
        n = t + 1 - self.dec_len
        for b in range(len(self.done)):
            nxt = pad
            if n < 0:
                nxt = int(self.prefix[t + 1])
            elif n < self.max_new:
                tok = int(argmax[b]) if (not self.done[b] or self.mut == "no_pad") else pad
                self.out[b, n] = tok
                if tok == eos:
                    self.done[b] = 1
                nxt = tok
            self.next[b] = nxt
        if 0 <= n < self.max_new and self.st[1] == 0 and (self.done.all() or n == self.max_new - 1):
            self.st[1] = n + 1 + (1 if self.mut == "finish_off_by_one" else 0)
        end = self.dec_len + self.max_new - 1
        self.st[0] = t + 1 if (t + 1 < end or self.mut == "pos_not_held") else end
        return self

    def state(self):
        return [self.st.copy(), self.done.copy(), self.out.reshape(-1).copy(), self.next.copy()]


class LlamaMachine:
    """rk_llama_generate's.  st = {n, finished step, pad, n_eos, max_new, max_total, P, 0, eos[8]}: column n gets the arg-max, or pad
    once the row has finished; a row finishes at one of the EOS ids or, with max_total > 0, once len + n + 1 >= max_total.  The
    token is the next input at position len[b] + n, held at P - 1.  st[1] as above.  Nothing happens at n == max_new."""

    def __init__(self, st, length, done, pos, out, next_ids, mut=None):
        self.st, self.len, self.done, self.pos, self.out, self.next = (np.array(a, np.int32) for a in (st, length, done, pos, out, next_ids))
        self.out = self.out.reshape(len(self.done), int(self.st[4]))
        self.mut = mut

    def step(self, argmax):
        st = self.st
        n, pad, n_eos, max_new, max_total, P = (int(st[i]) for i in (0, 2, 3, 4, 5, 6))
        if n >= max_new:
            return self
        eos = set(int(x) for x in st[8:8 + n_eos])
        for b in range(len(self.done)):
            tok = int(argmax[b]) if (not self.done[b] or self.mut == "no_pad") else pad
            self.out[b, n] = tok
            if not self.done[b] and ((max_total > 0 and int(self.len[b]) + n + 1 >= max_total) or tok in eos):
                self.done[b] = 1
            self.next[b] = tok
            q = int(self.len[b]) + n
            self.pos[b] = q if (q < P - 1 or self.mut == "pos_not_held") else P - 1
        if st[1] == 0 and (self.done.all() or n == max_new - 1):
            st[1] = n + 1 + (1 if self.mut == "finish_off_by_one" else 0)
        st[0] = n + 1
        return self

    def state(self):
        return [self.st.copy(), self.done.copy(), self.pos.copy(), self.out.reshape(-1).copy(), self.next.copy()]


class SessionMachine:
    """A decoding session's.  st = {finishes so far, pad, n_eos, max_len, cap, 0, 0, 0, eos[8]}; per slot len, col, max_new, done
    (1: idle or finished).  An active slot's column col gets its arg-max; it finishes at an EOS id or at its max_new-th (or cap-th)
    token; the token is its next input at position len + col, held at max_len - 1.  An idle or done slot emits nothing, keeps its
    position, feeds pad and is not counted again.  admit = (slots, lens, max_news): arg-max row r belongs to slot slots[r], which
    starts here; only those slots are touched; an entry outside [0, n_slots) is skipped."""

    def __init__(self, st, length, col, max_new, done, pos, out, next_ids, mut=None):
        arrs = [np.array(a, np.int32) for a in (st, length, col, max_new, done, pos, out, next_ids)]
        self.st, self.len, self.col, self.max_new, self.done, self.pos, self.out, self.next = arrs
        self.out = self.out.reshape(len(self.done), int(self.st[4]))
        self.mut = mut

    def step(self, argmax, admit=None):
        st = self.st
        pad, n_eos, max_len, cap = (int(st[i]) for i in (1, 2, 3, 4))
        eos = set(int(x) for x in st[8:8 + n_eos])
        n_slots = len(self.done)
        if admit is not None and self.mut == "admit_resets_all":
            self.col[:] = 0
            self.done[:] = 0
        rows = range(len(admit[0])) if admit is not None else range(n_slots)
        fin = 0
        for r in rows:
            b = r
            if admit is not None:
                b = int(admit[0][r])
                if b < 0 or b >= n_slots:
                    continue
                self.len[b], self.max_new[b], self.col[b], self.done[b] = admit[1][r], admit[2][r], 0, 0
            if self.done[b]:
                self.next[b] = pad
                if self.mut == "done_counted_twice":
                    fin += 1
                continue
            tok, c = int(argmax[r]), int(self.col[b])
            f = c + 1 >= self.max_new[b] or c + 1 >= cap or tok in eos
            if c < cap:
                self.out[b, c] = tok
            self.next[b] = tok
            q = int(self.len[b]) + c
            self.pos[b] = q if (q < max_len - 1 or self.mut == "pos_not_held") else max_len - 1
            self.col[b] = c + 1
            if f:
                self.done[b] = 1
                fin += 1
        st[0] += fin
        return self

    def state(self):
        return [self.st.copy(), self.len.copy(), self.col.copy(), self.max_new.copy(), self.done.copy(), self.pos.copy(),
                self.out.reshape(-1).copy(), self.next.copy()]


# ---- the yardstick and the verdicts ---------------------------------------------------------------------------------------------------
EXPECTED = {"embed": embed_expected, "rowscale": rowscale_expected, "rmsnorm": rmsnorm_expected, "head_rows": head_expected,
            "argmax_blocks": argmax_expected, "qlm_lse": qlm_expected, "rope": rope_expected, "kv_fill": kv_fill_expected}
EMULATED = {"embed": embed_emulated, "rowscale": rowscale_emulated, "rmsnorm": rmsnorm_emulated, "qlm_lse": qlm_emulated,
            "rope": rope_emulated}
TOLERANCED = {"embed": "rowscale", "rowscale": "out", "rmsnorm": "out", "qlm_lse": "out", "rope": "out"}   # op -> its toleranced output
HONEST = [(o, n) for o in ("lanes", "chain", "pairwise") for n in (0, 1, -1)]


def expected(p, mut=None):
    return EXPECTED[p.op](p, mut)


def emulated(p, order="lanes", nudge=0):
    return EMULATED[p.op](p, order, nudge)


def yardstick(p, want=None):
    """E of the problem's toleranced output (module docstring): per row and absolute for fp16 outputs, one relative figure, at
    least 2^-24, for fp32 outputs."""
    key = TOLERANCED[p.op]
    want = expected(p)[key] if want is None else want
    emu = emulated(p, "lanes")[key].astype(f64)
    if p.op == "rope":
        return np.abs(emu - want).max(axis=1, keepdims=True)
    if p.op == "rmsnorm":                                    # a row's elements share one factor: relative, per row
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(want != 0, np.abs(emu - want) / np.abs(want), 0.0)
        return np.maximum(rel.max(axis=1, keepdims=True), U24)
    nz = want != 0
    rel = (np.abs(emu - want)[nz] / np.abs(want[nz])).max() if nz.any() else 0.0
    return max(float(rel), U24)


def miss(p, got, want=None, E=None):
    """Largest (error - half ulp) / (C_ROWS-free) E of a toleranced output: <= C_ROWS passes.  got: the output as the device (or an
    emulation) left it, fp16 for rmsnorm / rope, fp32 otherwise."""
    key = TOLERANCED[p.op]
    want = expected(p)[key] if want is None else want
    E = yardstick(p, want) if E is None else E
    g = np.asarray(got).astype(f64)
    if p.op in ("rmsnorm", "rope"):
        w = np.clip(want, -F16_MAX, F16_MAX)
        over = np.maximum(np.abs(g - w) - half_ulp16(w), 0.0)
        scale = np.abs(w) if p.op == "rmsnorm" else 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(over > 0, over / (np.broadcast_to(E, over.shape) * scale), 0.0)
        return float(np.nan_to_num(r, nan=np.inf).max())
    err = np.abs(g - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / (E * np.abs(want)), 0.0)
    return float(np.nan_to_num(r, nan=np.inf).max())


def judge(p, got, what=""):
    """Asserts the random-tier bound of a toleranced output; returns the ratio (for the record)."""
    g = np.asarray(got)
    assert np.isfinite(g.astype(f64)).all(), f"{what}: non-finite output"
    r = miss(p, g)
    print(f"{what}: worst (error - half ulp) / E = {r:.3f} (C_ROWS {C_ROWS})")
    assert r <= C_ROWS, f"{what}: off by {r:.3f} E, C_ROWS = {C_ROWS}"
    return r


def judge_head(p, got, what=""):
    """Head logits: exact for integer operands, else tau = 4 E32 of tests/_gemm_ref.py on the call's operands - x and the WHOLE head
    table, as the GEMM tests take the whole W: E32 is a maximum over sampled chains, and the one chain of a 1 x 1 call (its error
    may happen to be a tenth of an ulp of the sum) is no yardstick for another honest order of the same 520 terms."""
    want = head_expected(p)["out"]
    if p.tier == "S":
        assert np.array_equal(np.asarray(got, dtype=f64), want), f"{what}: integer logits differ"
        return 0.0
    return G.check_f32(got, want, G.tau(p.x, p.head), what)


# ---- builders --------------------------------------------------------------------------------------------------------------------------
def banded(rs, interior, band_rows):
    """A table [rows, d] with band_rows finite trap rows in front and behind; returns (whole, interior offset in elements)."""
    d = interior.shape[1]
    band = lambda: (rs.standard_normal((band_rows, d)) * 8 + 100).astype(interior.dtype)
    return np.concatenate([band(), interior, band()]), band_rows * d


def build_embed(seed, rows, d, vocab=37, fold=1, eps=1e-6, ids=None):
    rs = np.random.RandomState(seed)
    table = (rs.standard_normal((vocab, d)) * rs.choice([0.01, 1.0, 30.0], size=(vocab, 1))).astype(f16)
    table[0, :] = 0                                          # an all-zero row: factor rsqrt(eps) / xs
    table[1, 0::3] = f16(2.0 ** -13)                         # subnormal in fp16 after the scaling by 2^-4
    table[1, 1::3] = f16(6e-8)                               # the smallest subnormal: scales to 0
    table[2, 0::2] = f16(65504)
    table[2, 1::2] = f16(-65504)
    if ids is None:
        ids = np.array(([0, vocab - 1, 1, 2, 1] + list(rs.randint(0, vocab, size=rows)))[:rows], np.int32)
    return problem("embed", rows=rows, d=d, vocab=vocab, fold=fold, eps=eps, xs=XS, table=table, ids=np.asarray(ids, np.int32))


def build_rowscale(seed, rows, nb, d=None, eps=1e-6):
    rs = np.random.RandomState(seed)
    ssq = (rs.chisquare(64, size=(rows, nb)) * rs.choice([1e-4, 1.0, 1e4], size=(rows, 1))).astype(f32)
    return problem("rowscale", rows=rows, nb=nb, d=d or 64 * nb, eps=eps, xs=XS, ssq=ssq)


def build_rmsnorm(seed, rows, d, tier="R", row_map=None, out_scale=1.0, eps=1e-6, src_rows=None):
    rs = np.random.RandomState(seed)
    src_rows = src_rows or (rows if row_map is None else int(max(row_map)) + 2)
    if tier == "S":
        assert d % 32 == 0
        x = np.zeros((src_rows, d), f32)
        for r in range(src_rows):
            k = r % 3
            vals = [(1.0, d // 2)] if k == 0 else ([(2.0, 7 * d // 8)] if k == 1 else [(4.0, 31 * d // 32)])
            row = np.zeros(d, f32)
            n = vals[0][1]
            row[rs.permutation(d)[:n]] = vals[0][0] * rs.choice([-1.0, 1.0], size=n)
            x[r] = row
        w = (2.0 ** ((np.arange(d) * 7 + 3) % 5 - 2)).astype(f32) * np.where(np.arange(d) % 3 == 0, -1, 1).astype(f32)
        return problem("rmsnorm", tier="S", rows=rows, d=d, src_rows=src_rows, x=x, w=w, row_map=row_map, out_scale=out_scale, eps=0.5)
    x = (rs.standard_normal((src_rows, d)) * rs.choice([0.05, 1.0, 40.0], size=(src_rows, 1))).astype(f32)
    if src_rows >= 3:
        x[1] = 0                                             # a zero row
        x[2] = (rs.standard_normal(d) * 2e-3).astype(f32)    # mean square of a few eps
    if src_rows >= 4:
        x[3, ::5] *= 4000                                    # products above 65504: saturate
    w = (1.0 + 0.5 * rs.standard_normal(d)).astype(f32)
    w[::7] *= 30
    if src_rows >= 4:
        w[35] = 3e5 / out_scale                              # with the row's largest element (at least its rms): far above 65504
        x[3, 35] = np.abs(x[3]).max()
    return problem("rmsnorm", rows=rows, d=d, src_rows=src_rows, x=x, w=w, row_map=row_map, out_scale=out_scale, eps=eps)


def build_head(seed, rows, n_out, d, vocab=67, tier="R", out_ids=None):
    rs = np.random.RandomState(seed)
    if tier == "S":
        x = rs.randint(-4, 5, size=(rows, d)).astype(f16)
        head = rs.randint(-4, 5, size=(vocab, d)).astype(f16)
    else:
        x = rs.standard_normal((rows, d)).astype(f16)
        head = rs.standard_normal((vocab, d)).astype(f16)
    if out_ids is None:
        out_ids = ([0, vocab - 1, 0] + list(rs.randint(0, vocab, size=n_out)))[:n_out]
    return problem("head_rows", tier=tier, rows=rows, n_out=n_out, d=d, vocab=vocab, x=x, head=head, out_ids=np.asarray(out_ids, np.int32))


def build_verdict(seed, n_seq, d, vocab=67, tier="R"):
    """Pairs whose logits are integers (tier S): pair 0 an exact tie (both orderings the same row), pair 1 a margin of more than
    104 (one exp underflows: P exactly 0 or 1), the rest small margins."""
    p = build_head(seed, n_seq, 2, d, vocab, tier, out_ids=[5, vocab - 1])
    p.op, p.false_id, p.true_id = "pair_verdict", 5, vocab - 1
    if tier == "S":
        p.x[1] = p.x[0]
        if n_seq >= 4:
            p.head[p.true_id, :] = 0
            p.head[p.false_id, :] = 0
            p.head[p.true_id, :8] = 4
            p.x[2, :8] = 4                                   # true - false = 128: P(true) = 1 exactly
            p.x[3, :8] = -4                                  # -128: P(true) = 0 exactly
    return p


def build_argmax(seed, rows, nb):
    rs = np.random.RandomState(seed)
    bval = rs.randint(-3, 4, size=(rows, nb)).astype(f32)    # few distinct values: ties everywhere
    bidx = (np.arange(nb)[None, :] * 32 + rs.randint(0, 32, size=(rows, nb))).astype(np.int32)
    for r in range(rows):                                    # the block order is not the column order: a tie is won by the smaller COLUMN
        perm = rs.permutation(nb)
        bval[r], bidx[r] = bval[r][perm], bidx[r][perm]
    if rows >= 2:
        bval[1] = -np.inf                                    # all -inf: the smallest index
    if rows >= 3 and nb >= 257:                              # a tie across waves and across a lane's stride: maximum at blocks 256 (lane 0,
        bval[2] = 0                                          # second pass), 70 (wave 1) and 3 (wave 0); the smallest column sits in wave 1
        bval[2, [3, 70, 256]] = 9
        bidx[2, [3, 70, 256]] = [5000, 17, 4000]
    return problem("argmax_blocks", rows=rows, nb=nb, bval=bval, bidx=bidx)


def build_qlm(seed, n_seq, nb, n_pos=0, row_lens=None, out_idx=None):
    rs = np.random.RandomState(seed)
    row_off = None if row_lens is None else np.concatenate([[0], np.cumsum(row_lens)]).astype(np.int32)
    R = n_seq * n_pos if row_off is None else int(row_off[-1])
    stats = np.zeros((R, nb, 2), f32)
    stats[:, :, 0] = rs.standard_normal((R, nb)) * 3
    stats[:, :, 1] = 1.0 + rs.rand(R, nb) * 31
    if nb >= 3:
        stats[:, nb // 2, 0] += 200                          # block maxima 200 apart
        stats[:, -1, 0] = -np.inf                            # a fully masked tail block
        stats[:, -1, 1] = 0
    xlab = (rs.standard_normal(R) * 3).astype(f32)
    return problem("qlm_lse", rows=n_seq, nb=nb, n_pos=n_pos, row_off=row_off, out_idx=None if out_idx is None else np.asarray(out_idx, np.int32),
                   stats=stats, xlab=xlab)


def ragged_positions(T, max_pos):
    """Positions of a ragged batch: restarting at 0, the last row at max_pos - 1."""
    pos = np.array([[0, 1, 2, 0, 1, 0, 3][i % 7] for i in range(T)], np.int32)
    pos[-1] = max_pos - 1
    return pos


def build_rope(seed, T, H, n_kv, hd, tier="R", bias=False, pad=8, max_pos=9):
    rs = np.random.RandomState(seed)
    half, n_all = hd // 2, (H + 2 * n_kv) * hd
    ld = n_all + pad
    if tier == "S":
        sel = rs.randint(0, 4, size=(max_pos, half))
        cos = np.array([1, 0, 0, -1], f32)[sel]
        sin = np.array([0, 1, -1, 0], f32)[sel]
        qkv = rs.randint(-64, 65, size=(T, ld)).astype(f16)
        b = rs.randint(-32, 33, size=n_all).astype(f32) if bias else None
    else:
        ang = np.arange(max_pos)[:, None] * (10000.0 ** (-np.arange(half) / half))[None, :]
        cos, sin = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
        qkv = (rs.standard_normal((T, ld)) * 4).astype(f16)
        b = (rs.standard_normal(n_all) * 8).astype(f32) if bias else None
    return problem("rope", tier=tier, rows=T, H=H, n_kv=n_kv, hd=hd, ld=ld, max_pos=max_pos, pos=ragged_positions(T, max_pos), cos=cos, sin=sin,
                   bias=b, qkv=qkv)


def build_kv_fill(seed, H, n_kv, hd, lens, P, slots=None, n_slots=0, pad=8, band_rows=2):
    rs = np.random.RandomState(seed)
    ld = (H + 2 * n_kv) * hd + pad
    T = int(sum(lens))
    qkv = rs.randint(-2000, 2000, size=(T, ld)).astype(f16)  # distinct enough: a wrong row, head or half shows
    whole, off = banded(rs, qkv, band_rows)
    n_rows = n_slots if slots is not None else len(lens)
    cache = rs.randint(3000, 4000, size=2 * n_rows * n_kv * P * hd).astype(f16)   # the pre-fill: values no qkv element has
    return problem("kv_fill", rows=len(lens), H=H, n_kv=n_kv, hd=hd, ld=ld, P=P, seq_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
                   slots=None if slots is None else np.asarray(slots, np.int32), n_slots=n_slots, qkv=qkv, qkv_whole=whole, qkv_off=off, cache=cache)


def build_cached_step(seed, H, n_seq, P, pos, tier, band=8):
    """The T5 cached step (rk_debug_attn kind 6) as a tree-form decoder problem of tests/_attn_ref.py, whose reference, selector
    fixtures and judge it reuses: one buffer of fused rows q | k | v - the n_seq step rows first, then the cache rows (sequence b,
    position j at row n_seq + b P + j) -; query row b at position pos sees the cache rows 0 .. pos - 1 of its sequence and, as key
    pos, its own row.  p.step_q / p.step_cache are the operands of the device call.  Tier S traps: the stale cache row AT pos, the
    cache row behind pos, the row in front of the sequence's cache (a neighbour's last row, another sequence's step row)."""
    rs = np.random.RandomState(seed)
    I, n_rows = 64 * H, n_seq + n_seq * P
    buf = A._rows_buffer(rs, n_rows, 3 * I, band, tier)
    tk = np.zeros((n_seq, P), np.int32)
    for b in range(n_seq):
        tk[b] = n_seq + b * P + np.arange(P)
        tk[b, pos] = b
    p = A.problem(A.DEC, H=H, n_seq=n_seq, Ld=P, band=band, ldq=3 * I, ldctx=I, out_rows=n_seq, tier=tier, k_col=I, v_col=2 * I,
                  tree_keys=tk, tree_pos=np.full(n_seq, pos, np.int32), pos=np.array([pos], np.int32), P=P)
    if tier == "S":
        p.lut = np.zeros((H, A.LUT_N), f32)
        buf[:, 2 * I:] = A._int_values(rs, (buf.shape[0], I))
        for h in range(H):
            queries, traps = [], []
            for b in range(n_seq):
                adm = tuple(int(band + x) for x in tk[b, :pos + 1])
                sp = [adm[-1], adm[0], adm[max(pos - 1, 0)]] + [adm[k] for k in A.edges_of(pos + 1, 16)]
                queries.append((adm, [sp[(b + h) % len(sp)]]))
                c0 = band + n_seq + b * P
                traps.append((b, [c0 + pos, c0 + pos + 1 if pos + 1 < P else c0 + pos, c0 - 1][(b + h) % 3]))
            K, win, placed = A.selector(rs, buf.shape[0], 64, 4, queries, traps, what=f"cached step head {h}")
            p.n_traps += len(placed)
            buf[:, I + h * 64:I + h * 64 + 64] = K
            buf[band:band + n_seq, h * 64:h * 64 + 64] = K[win]
    else:
        p.lut = (2.0 * rs.standard_normal((H, A.LUT_N))).astype(f32)
    p.q, p.out = buf, A.sentinel16((n_seq, I))
    p.step_q = np.ascontiguousarray(buf[:band + n_seq + band])
    p.step_cache = np.ascontiguousarray(buf[band + n_seq:band + n_rows, I:]).reshape(-1)
    return p


def cached_step_cache_expected(p):
    """The cache after the step: row pos of every sequence holds the step row's k | v, every other row its pre-fill."""
    I, pos = 64 * p.H, int(p.pos[0])
    c = p.step_cache.copy().reshape(p.n_seq, p.P, 2 * I)
    c[:, pos] = p.q[p.band:p.band + p.n_seq, I:]
    return c.reshape(-1)


# the CPU-side fixtures behind C_ROWS: the toleranced problems of tests/test_gpu_rows.py
def FIXTURES():
    fx = []
    for d, rows in ((64, 1), (576, 4), (1024, 5)):
        fx.append(build_embed(11 + d, rows, d))
    for nb, rows in ((4, 1), (8, 256), (5, 257), (1, 5)):
        fx.append(build_rowscale(20 + nb, rows, nb))
    for d in (64, 1024, 1088, 2048, 2112, 4096):
        fx.append(build_rmsnorm(30 + d, 5, d, row_map=[4, 0, 3, 3, 1, 2][:5], out_scale=d ** -0.5, src_rows=6))
        fx.append(build_rmsnorm(31 + d, 1, d))
    for nb, n_pos in ((1, 1), (255, 1), (257, 33), (1004, 1)):
        fx.append(build_qlm(40 + nb, 2, nb, n_pos=n_pos))
    fx.append(build_qlm(49, 4, 257, row_lens=[3, 0, 33, 1], out_idx=[2, 0, 3, 1]))
    for hd, H, n_kv in ((128, 1, 1), (128, 4, 2), (128, 32, 8), (64, 4, 2), (64, 64, 8)):
        for bias in (False, True):
            fx.append(build_rope(50 + hd + H, 7, H, n_kv, hd, bias=bias))
    return fx


def measure_c_rows(fixtures=None):
    """{op: the largest ratio an honest order reaches}, and C_ROWS = twice the largest, rounded up to a tenth."""
    worst = {}
    for p in (FIXTURES() if fixtures is None else fixtures):
        key = TOLERANCED[p.op]
        want = expected(p)[key]
        E = yardstick(p, want)
        for order, nudge in HONEST:
            if p.op == "rope" and nudge:
                continue
            got = emulated(p, order, nudge)[key]
            got = f16_sat(got) if p.op in ("rmsnorm", "rope") else got
            worst[p.op] = max(worst.get(p.op, 0.0), miss(p, got, want, E))
    return worst, float(np.ceil(2 * max(worst.values()) * 10 - 1e-9) / 10)
