"""The drafting step (rk_debug_attn kind 5 with g1 > 1: kv_cache_append_kernel + the attn_dec_keys_* entries) on top of the step
references: tests/_attn_ref.py (128-wide heads), tests/_attn_ref_hd64.py (64-wide), tests/_attn_ref_win.py's window rule and
tests/_qwen3_ref.py's q / k head norm.  Those modules cut a plain step into (row, head) pieces - the row's rotated query, the cache
keys below pos and the row's own rotated key and value at pos; here the rows come g1 per cache row and the rule, written from the
contract above attn_dec_cached_body (KEYS) and kv_cache_append_kernel, is:

  every LIVE row's rotated key and its value are appended to cache row b // g1 at pos[b]; then step row b attends cache row b // g1
  at the keys lo .. pos[b] (lo = max(0, pos[b] - W + 1) under a window W, else 0) - whichever row of the step wrote them.  A dead row
  writes nothing and its context is unspecified.

`items` takes the plain module's pieces of the same rows (so the rotation, the bias, the norm, the kv head of a query head and the
scale stay written down in ONE place) and replaces their keys by that rule; the pieces are then judged by the modules' own rule:
tier S bit for bit, tier R within half an fp16 ulp + A.C x E, E = the chain emulation's largest error against fp64 over the pieces
(every piece is one row: the sample is all of them).  No tolerance of its own.

Poison.  Every cache position above a slot's highest live position holds fp16 NaN: the kernels clamp their loads to pos, so a finite
context proves that nothing beyond pos was read, and a NaN that survives in the cache proves that nothing was written there (a dead
row's would-be position included).  Positions below a window's lo stay finite: the kernel loads and masks them.

Tier S (no window, no norm): _attn_ref.build_step's selector design in ONE key space per (slot, kv head) that all the slot's rows
share: a query copies its winner's key row; winners at the row's own key, the key before it (an earlier row of the SAME step wrote
it), key 0 and both sides of every 128-key edge; the key behind pos - the next row's new key, or the poison - is a copy of the
winner with another value row, so a row that admits it comes out as the mean of two value rows (or NaN); the cache holds the
NEGATED key at every live position, so a row whose append is lost or misplaced loses its winner.

The sequential plain equivalent (`sequential`): g1 plain steps over the slots, call j feeding row (s, j) at its position on the
cache the previous call left (a slot whose row j is dead feeds its last live row again: the same bytes to the same place).  The
drafting call's context of every live row and its final cache equal that sequence's byte for byte - no tolerance.

Mutants (tests/test_attn_ref_draft_host.py): "sees_pos_plus1" (row j admits key pos + 1), "append_ignores_live" (dead rows write
too), "append_row_b" (the append goes to cache row b instead of b // g1), "lo_minus1" / "lo_plus1" (the window's first key)."""
from types import SimpleNamespace

import numpy as np

import _attn_ref as A
import _attn_ref_hd64 as H64

f16, f32, f64 = np.float16, np.float32, np.float64
NAN16 = 0x7E00
MUTANTS = ("sees_pos_plus1", "append_ignores_live", "append_row_b", "lo_minus1", "lo_plus1")


def _mod(p):
    return A if p.hd == 128 else H64


def view(p):
    """The plain STEP problem of the same n_seq rows, row b on a copy of cache row b // g1: what the step modules cut into pieces."""
    v = SimpleNamespace(**{k: x for k, x in p.__dict__.items() if not k.startswith("_")})
    half = p.cache.size // 2
    kc, vc = (c.reshape(p.n_slots, -1) for c in (p.cache[:half], p.cache[half:]))
    rows = np.arange(p.n_seq) // p.g1
    v.cache = np.concatenate([kc[rows].reshape(-1), vc[rows].reshape(-1)])
    return v


def _plain_items(p, emul):
    if p.qk_w is not None:
        import _qwen3_ref as Q
        return Q.qkn_step_items(view(p), emul)
    return _mod(p).items(view(p), None, emul)


def _slot_cache(p, dtype):
    slots = SimpleNamespace(n_seq=p.n_slots, n_kv=p.n_kv, P=p.P)
    kc, vc = _mod(p).step_cache_views(slots, p.cache.astype(dtype))
    return kc.copy(), vc.copy()


def _appends(p, plain, mut):
    """(cache row, kv head, position) -> (key, value), in row order"""
    w = {}
    for it in plain:
        b, g, pos, knew, vnew = it["new"]
        if p.live[b] or mut == "append_ignores_live":
            w[(b % p.n_slots if mut == "append_row_b" else b // p.g1, g, pos)] = (knew, vnew)
    return w


def items(p, mut=None, emul=False):
    """The (live row, head) pieces of a drafting step: the plain pieces' q, scale and output place, the keys by the rule above."""
    plain = _plain_items(p, emul)
    w = _appends(p, plain, mut)
    kc, vc = _slot_cache(p, f16 if emul else f64)
    for (s, g, t), (k, v) in w.items():
        kc[s, g, t], vc[s, g, t] = k, v
    out = []
    for it in plain:
        b, g, pos = it["new"][:3]
        if not p.live[b]:
            continue
        hi = pos + (1 if mut == "sees_pos_plus1" and pos + 1 < p.P else 0)
        lo = max(0, pos - p.W + 1 + {"lo_minus1": -1, "lo_plus1": 1}.get(mut, 0)) if p.W else 0
        out.append(dict(it, k=kc[b // p.g1, g, lo:hi + 1], v=vc[b // p.g1, g, lo:hi + 1]))
    return out


def expected_cache(p, emul=False, mut=None):
    """The cache after the step (fp64, or with emul the kernels' fp16 rows) and the mask of the appended elements"""
    w = _appends(p, _plain_items(p, emul), mut)
    kc, vc = _slot_cache(p, f16 if emul else f64)
    new = np.zeros(kc.shape, dtype=bool)
    for (s, g, t), (k, v) in w.items():
        kc[s, g, t], vc[s, g, t], new[s, g, t] = k, v, True
    return np.concatenate([kc.reshape(-1), vc.reshape(-1)]), np.concatenate([new.reshape(-1), new.reshape(-1)])


def expected64(p, mut=None):
    """fp64 context rows [n_seq, ldctx]; NaN in a dead row (unspecified) - and wherever a mutant lets the poison in"""
    out = np.full((p.n_seq, p.ldctx), np.nan)
    for it in items(p, mut):
        with np.errstate(invalid="ignore"):
            out[it["out_rows"], it["out_col"]:it["out_col"] + it["v"].shape[1]] = A.attend64(it)
    return out


def yardstick(p):
    if getattr(p, "_E", None) is None:
        p._E = max(float(np.abs(A.emulate_item(em).astype(f64) - A.attend64(ref)).max()) for ref, em in zip(items(p), items(p, emul=True)))
    return p._E


def judge(p, got, what=""):
    """`got` [n_seq, ldctx] fp16, the interior of the call's output: the live rows by the step modules' rule (tier S bit for bit, tier R
    half an fp16 ulp + A.C x E); a dead row may hold anything.  Returns the largest (error - half ulp) / E (0.0 in tier S)."""
    if getattr(p, "_want", None) is None:
        p._want = expected64(p)
    want, got = p._want, np.asarray(got)
    assert got.shape == want.shape and got.dtype == f16
    rows = np.flatnonzero(p.live)
    assert not np.isnan(want[rows]).any(), "the reference itself read the poison"
    g, x = got[rows], want[rows]
    assert np.isfinite(g.astype(f64)).all(), f"{what}: non-finite output in live row {rows[np.argwhere(~np.isfinite(g.astype(f64)))[0][0]]} (the poison beyond pos?)"
    if p.tier == "S":
        bad = g.view(np.uint16) != A.f16_sat(x).view(np.uint16)
        if bad.any():
            i, j = np.argwhere(bad)[0]
            raise AssertionError(f"{what}: step row {rows[i]}, column {j} (head {j // p.hd}): got {g[i, j]}, the selected row has {x[i, j]}")
        return 0.0
    E = yardstick(p)
    err = np.abs(g.astype(f64) - x)
    over = err - A.half_ulp16(x)
    if (over > A.C * E).any():
        i, j = np.argwhere(over > A.C * E)[0]
        raise AssertionError(f"{what}: step row {rows[i]}, column {j} (head {j // p.hd}): got {g[i, j]}, fp64 {x[i, j]:.6g}, error {err[i, j]:.3g} > "
                             f"half ulp {A.half_ulp16(x[i, j]):.3g} + {A.C} x E ({E:.3g})")
    return float(over.max()) / E


def judge_cache(p, got, what=""):
    """The cache after the step (interior, flat fp16): the live rows' positions hold their key and value (the step modules' rule),
    every other element is the caller's bit for bit - the poison and a dead row's would-be position included."""
    (want, new), em = expected_cache(p), expected_cache(p, emul=True)[0].astype(f64)
    got = np.asarray(got).reshape(-1)
    assert got.size == want.size and got.dtype == f16
    stale = ~new & (got.view(np.uint16) != p.cache.reshape(-1).view(np.uint16))
    assert not stale.any(), f"{what}: cache element {np.argwhere(stale)[0][0]} changed and is not a live row's"
    if p.tier == "S":
        assert (got[new].view(np.uint16) == A.f16_sat(want[new]).view(np.uint16)).all(), f"{what}: the appended key / value rows are not the live rows'"
        return
    e = float(np.abs(em[new] - want[new]).max())           # includes the emulation's own fp16 rounding: at least what a kernel may add
    err = np.abs(got[new].astype(f64) - want[new])
    assert (err <= A.half_ulp16(want[new]) + e).all(), f"{what}: appended row off by {err.max():.3g}"


# ---- the problem ------------------------------------------------------------------------------------------------------------------------
def build_draft_step(seed, H, n_kv, slot_pos, g1, live, P, tier, *, hd=128, bias=False, W=0, qkn=False, band=8):
    """n_slots = len(slot_pos) cache rows, g1 step rows each: row (s, j) at slot_pos[s] + j, live[s][j] (row 0 always; a row that would
    pass P - 1 must be dead and gets position 0, as draft_lookup_kernel gives a dead row).  Tier R: N(0, 1) operands on the modules'
    rotary tables; tier S: the module docstring's selector design (no window, no norm)."""
    mod = A if hd == 128 else H64
    n_slots = len(slot_pos)
    live = np.asarray(live, dtype=np.int32).reshape(n_slots, g1)
    would = np.asarray(slot_pos)[:, None] + np.arange(g1)[None, :]
    assert live[:, 0].all() and (would[live == 1] < P).all() and (tier == "R" or not (W or qkn))
    pos = np.where(would < P, would, 0).astype(np.int32).reshape(-1)
    rs = np.random.RandomState(seed)
    n_seq, Q, KV, G = n_slots * g1, hd * H, hd * n_kv, H // n_kv
    ldq = Q + 2 * KV
    q = A._rows_buffer(rs, n_seq, ldq, band, tier, amp=8)
    p = A.problem(A.STEP, H=H, n_kv=n_kv, n_seq=n_seq, P=P, pos=pos, band=band, ldq=ldq, ldctx=Q, out_rows=n_seq, tier=tier, p16=False,
                  hd=hd, g1=g1, live=live.reshape(-1), n_slots=n_slots, W=W, qk_w=None, qk_eps=0.0)
    top = np.where(live == 1, would, -1).max(axis=1)         # a slot's highest live position
    if tier == "S":
        p.cos, p.sin = np.ones((P, hd // 2), dtype=f32), np.zeros((P, hd // 2), dtype=f32)
        kc = np.zeros((n_slots, n_kv, P, hd), dtype=f16)
        vc = A._int_values(rs, (n_slots, n_kv, P, hd))
        q[:, Q + KV:] = A._int_values(rs, (q.shape[0], KV))
        for s in range(n_slots):
            rows = [j for j in range(g1) if live[s, j]]
            for g in range(n_kv):
                queries, traps = [], []
                for j in rows:
                    t = int(would[s, j])
                    sp = [k for k in [t, t - 1, 0] + A.edges_of(t + 1, 128) if 0 <= k <= t]
                    for r in range(G):
                        queries.append((range(0, t + 1), [sp[(r + g + s + j) % len(sp)]]))
                        if t >= 16 or (t > 0 and j == rows[-1]):             # (a copy per row in front of position 16 would leave the next rows no free winner)
                            traps.append((len(queries) - 1, t + 1))
                K, win, placed = A.selector(rs, P, hd, 8, queries, traps, scale=hd ** -0.5, what=f"draft step slot {s} kv head {g}")
                p.n_traps += len(placed)
                kc[s, g] = K
                for n, j in enumerate(rows):
                    t, b = int(would[s, j]), band + s * g1 + j
                    q[b, Q + g * hd:Q + g * hd + hd] = K[t]                  # the key comes from the row ...
                    kc[s, g, t] = -K[t]                                      # ... the cache row it replaces would lose
                    for r in range(G):
                        q[b, (g * G + r) * hd:(g * G + r) * hd + hd] = K[win[n * G + r]]
        if bias:                                                             # integer bias, row entries shifted so that row + bias is the design
            p.qkv_bias = rs.randint(-3, 4, size=ldq).astype(f32)
            q[band:band + n_seq] = (q[band:band + n_seq].astype(f32) - p.qkv_bias).astype(f16)
    else:
        p.cos, p.sin = mod.rope_tables(P)
        kc, vc = (rs.standard_normal((n_slots, n_kv, P, hd)).astype(f16) for _ in range(2))
        if bias:
            p.qkv_bias = (rs.standard_normal(ldq) * np.where(rs.rand(ldq) < 0.02, 8.0, 0.5)).astype(f32)
        if qkn:
            import _qwen3_ref as Q3
            p.qk_w, p.qk_eps = Q3.head_weights(np.random.RandomState(seed + 1)), float(f32(1e-6))
    for s in range(n_slots):
        kc[s, :, top[s] + 1:].view(np.uint16)[...] = NAN16
        vc[s, :, top[s] + 1:].view(np.uint16)[...] = NAN16
    p.cache = np.concatenate([kc.reshape(-1), vc.reshape(-1)])
    p.q, p.out = q, A.sentinel16((n_seq, Q))
    return p


def sequential(p):
    """The g1 plain steps that stand for the drafting step: per call j (step rows fed [n_slots], the plain STEP problem without its
    cache - the caller puts in what the previous call left)."""
    live = p.live.reshape(p.n_slots, p.g1)
    calls = []
    for j in range(p.g1):
        src = np.array([s * p.g1 + max(i for i in range(j + 1) if live[s, i]) for s in range(p.n_slots)])
        c = A.problem(A.STEP, H=p.H, n_kv=p.n_kv, n_seq=p.n_slots, P=p.P, pos=p.pos[src].copy(), band=p.band, ldq=p.ldq, ldctx=p.ldctx,
                      out_rows=p.n_slots, tier=p.tier, p16=False, cos=p.cos, sin=p.sin, qkv_bias=p.qkv_bias, hd=p.hd, qk_w=p.qk_w, qk_eps=p.qk_eps)
        c.q = np.concatenate([p.q[:p.band], p.q[p.band + src], p.q[-p.band:]])
        c.out = A.sentinel16((p.n_slots, p.ldctx))
        calls.append((src, c))
    return calls


# ---- the problems of tests/test_gpu_draft_attention.py (and of the host test that shows they tell the mutants apart) ---------------------
P_DRAFT = 304
HEADS = [(8, 1), (8, 2), (4, 2), (4, 4), (28, 4)]            # G = 8, 4, 2, 1, 7
G1S = (2, 4, 8)
_PROBLEMS = {}


def slot_sets(g1, P=P_DRAFT):
    """Three calls of 2 - 3 slots: (slot base positions, live rows per slot).  A slot's rows straddle an edge when its base lies
    max(1, g1 // 2) in front of it: positions 31 / 32 (a wave's keys), 127 / 128 and 255 / 256 (LDC_CHUNK: two and three chunks), 63 / 64
    (the toys' window starts to bite), 190 .. 193 (the window's lo crosses 127 / 128), P - 1 (the rows that would pass it dead);
    one slot at position 0; one slot with only row 0 live."""
    half = max(1, g1 // 2)
    return [([32 - half, 128 - half, 0], [g1, g1, g1]),
            ([256 - half, P - half, 200], [g1, half, 1]),
            ([190, 64 - half], [g1, g1])]


def problem(hd, heads, g1, call, tier, bias=False, W=0, qkn=False):
    """built once, shared by every option and engine that runs it, and left unchanged"""
    key = (hd, heads, g1, call, tier, bias, W, qkn)
    if key not in _PROBLEMS:
        base, n_live = slot_sets(g1)[call]
        live = [[int(j < n) for j in range(g1)] for n in n_live]
        seed = 900 + 97 * HEADS.index(heads) + 11 * g1 + call + (5 if bias else 0)
        _PROBLEMS[key] = build_draft_step(seed, heads[0], heads[1], base, g1, live, P_DRAFT, tier, hd=hd, bias=bias, W=W, qkn=qkn)
    return _PROBLEMS[key]


# ---- the documented arithmetic as the "kernel" (host tests) --------------------------------------------------------------------------------
def emulated(p, mut=None):
    """What kernels of the documented arithmetic return for the live rows (a dead row keeps the pre-fill), under one broken rule if mut"""
    out = p.out.copy()
    for it in items(p, mut, emul=True):
        with np.errstate(invalid="ignore"):
            out[it["out_rows"], it["out_col"]:it["out_col"] + it["v"].shape[1]] = A.emulate_item(it).astype(f16)
    return out


def emulated_cache(p, mut=None):
    return expected_cache(p, emul=True, mut=mut)[0].astype(f16)
