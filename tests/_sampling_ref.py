"""Reference for the sampling head (csrc/sampling_kernels.h), numpy only.

* philox4x32_10: Philox4x32-10 (Salmon et al., SC'11), vectorised; uniform(): the engine's u = (first word >> 8) * 2^-24 with
  key = the 64-bit seed (low word, high word), counter = (token index, 0, 0, 0).
* filter_row: HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper in fp64, top-p stated on values as
  include/rk_engine.h states it (an id stays iff the mass of the kept ids with z_j <= z_i exceeds 1 - p), with the two clearances
  the GPU tests put on their inputs.
* Row: the filtered row with its fp64 CDF in vocabulary order; interval(t) is token t's CDF interval, draw(u) the reference's
  own token for a uniform u.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (anything that converts to uint32) -> [..., 4] uint32"""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] & MASK for i in range(4)]
    k0 = np.asarray(key, dtype=np.uint64)[..., 0] & MASK
    k1 = np.asarray(key, dtype=np.uint64)[..., 1] & MASK
    for r in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform(seeds, index):
    """u of every (seed, token index) pair, fp64 in [0, 1) on the 2^-24 grid"""
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    ctr = np.zeros((seeds.size, 4), np.uint64)
    ctr[:, 0] = index.astype(np.uint64)
    key = np.stack([seeds & MASK, seeds >> np.uint64(32)], axis=-1)
    x0 = philox4x32_10(ctr, key)[:, 0].astype(np.uint64)
    return (x0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


class Row:
    """One filtered row: kept_k / kept (bool [V]: after top-k, after top-p), w (fp64 [V], exp((x - max x) / T) for kept ids, else
    0), Z, cdf (inclusive running sum of w in vocabulary order), and the clearances of the inputs: k_gap (the k-th largest logit
    minus the (k+1)-th; inf when top-k is off), p_clear (how far the cumulative mass on either side of the top-p boundary is from
    1 - p; inf when top-p is off), spread = sum w |x - max| / T / Z (the weights' error grows with it)."""

    def interval(self, t):
        t = np.asarray(t)
        return self.cdf[t] - self.w[t], self.cdf[t]

    def draw(self, u):
        """first kept id in vocabulary order whose running sum exceeds u Z"""
        t = np.searchsorted(self.cdf, np.asarray(u) * self.Z, side="right")
        return np.minimum(t, np.flatnonzero(self.kept)[-1])


def filter_row(x, T, k, p) -> Row:
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    V = x.size
    z = x / float(T)
    r = Row()
    r.k_gap = r.p_clear = np.inf
    if 0 < k < V:
        srt = np.sort(x)
        r.kept_k = z >= np.sort(z)[V - k]
        r.k_gap = srt[V - k] - srt[V - k - 1]
    else:
        r.kept_k = np.ones(V, bool)
    m = x.max()
    with np.errstate(invalid="ignore"):
        w = np.where(r.kept_k, np.exp((x - m) / float(T)), 0.0)
    w = np.nan_to_num(w, nan=0.0)
    r.kept = r.kept_k.copy()
    if p < 1:
        ids = np.flatnonzero(r.kept_k)
        order = ids[np.argsort(z[ids], kind="stable")]                 # ascending
        zs, q = z[order], w[order] / w[order].sum()
        cum = np.cumsum(q)
        last = np.searchsorted(zs, zs, side="right") - 1               # the last member of every group of equal values
        first = np.searchsorted(zs, zs, side="left")
        tail = cum[last]                                               # mass of the kept ids with z_j <= z_i
        keep = tail > 1.0 - p
        keep[-1] = True                                                # (the largest: its tail is 1)
        r.kept = np.zeros(V, bool)
        r.kept[order[keep]] = True
        b = int(np.argmax(keep))                                       # the first kept position: its group is the boundary
        below = cum[first[b] - 1] if first[b] > 0 else 0.0
        r.p_clear = min(tail[b] - (1.0 - p), (1.0 - p) - below)
    r.w = np.where(r.kept, w, 0.0)
    r.Z = r.w.sum()
    r.cdf = np.cumsum(r.w)
    with np.errstate(invalid="ignore"):
        a = np.where(r.w > 0, np.abs(x - m) / float(T), 0.0)
    r.spread = float((r.w * a).sum() / r.Z)
    return r


def make_rows(V, n_rows, seed):
    """n_rows logit rows of V ids, kinds in turn: 0 mixed sign (a wide bulk, and V // 4 <= 32 ids on a ladder of 0.37 above it that
    carries most of the mass), 1 the same all negative, 2 all equal, 3 one dominant id, 4 mixed sign with a tenth of the bulk at -inf."""
    rng = np.random.default_rng(seed)
    rows = np.empty((n_rows, V), np.float32)
    for r in range(n_rows):
        kind = r % 5
        x = rng.normal(0.0, 2.0, V)
        n_top = min(32, max(1, V // 4))
        top = rng.choice(V, n_top, replace=False)
        ladder = 6.0 + 0.37 * np.arange(n_top) + rng.uniform(-0.05, 0.05, n_top)
        if kind in (0, 1, 4):
            x[top] = ladder
        if kind == 1:
            x -= 40.0
        if kind == 2:
            x[:] = 1.5
        if kind == 3:
            x = rng.normal(0.0, 1.0, V)
            x[top[0]] = 60.0
        if kind == 4:
            bulk = np.setdiff1d(np.arange(V), top)
            x[rng.choice(bulk, max(1, bulk.size // 10), replace=False)] = -np.inf
        rows[r] = x.astype(np.float32)
    return rows
