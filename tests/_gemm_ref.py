"""fp64 reference of every epilogue of the engine's GEMM (csrc/gemm.h) and the tolerance model its tests use.

Plain numpy, fp64 throughout.  Everything is derived from acc = A @ W.T in fp64 - never from a kernel.

Tier A (exact): integer-valued fp16 operands, |a|, |w| <= 4, K <= 1024: every partial sum is an integer below 2^24, exact in
fp32 under ANY summation order, so fp32 outputs, fp16 roundings (RNE, saturation), block maxima / first indices, the fp16 copy
of the stream and its sums of squares are compared bit for bit.

Tier B (random): N(0, 1) operands (and an outlier form).  The yardstick E32 is the largest error against fp64 of a k-ordered fp32
chain of the exact products (np.cumsum(..., dtype=float32)) over a fixed sample of at most 16 rows x 256 columns of the very
problem; tau = 4 E32 is what an accumulator may be off by.  Why 4: the kernels sum in other orders (MFMA k-groups, 64-wide K
tiles, split K, lane-strided K + tree); blocked orders measured 3-5 x SMALLER than the chain on the CPU, so 4 x the chain is
generous for any legitimate order - and still below one fp16 half-ulp at the typical output magnitude, two orders of magnitude
below the 2e-3 sqrt(K) the kernel tests used before.
"""
import numpy as np

EPI_STORE_F16, EPI_RESID_F32, EPI_GEGLU_F16, EPI_RELU_F16, EPI_STORE_F32, EPI_SWIGLU_F16, EPI_ARGMAX_F32, EPI_LSE_F32 = range(8)
EPI_NAMES = ["store_f16", "resid_f32", "geglu_f16", "relu_f16", "store_f32", "swiglu_f16", "argmax_f32", "lse_f32"]
TILED, STREAM, GEMV = 0, 1, 2
GATED = (EPI_GEGLU_F16, EPI_SWIGLU_F16)
F16_EPIS = (EPI_STORE_F16, EPI_GEGLU_F16, EPI_RELU_F16, EPI_SWIGLU_F16)
FAMILY_HAS = {            # gemv_has / stream_has / tiled_has of csrc/rk_engine.hip
    TILED: [e for e in range(8) if e != EPI_ARGMAX_F32],
    STREAM: [e for e in range(8) if e != EPI_LSE_F32],
    GEMV: [EPI_STORE_F16, EPI_RESID_F32, EPI_GEGLU_F16, EPI_RELU_F16, EPI_STORE_F32],
}
F16_MAX = 65504.0
XS = 1.0 / 16.0           # RK_XRAW_SCALE: the fp16 copy of the stream is stored x 2^-4
U16, U24 = 2.0 ** -11, 2.0 ** -24     # half-ulp of fp16 / fp32 relative to the value
SENTINEL = 0xCD


# ---- the operation -----------------------------------------------------------------------------------------------------------
def acc64(a16, w16):
    return a16.astype(np.float64) @ w16.astype(np.float64).T


def gelu_new(x):
    """tanh form (hf: activations.py NewGELUActivation), as oracle/t5_numpy.py."""
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def gelu_new_grad(x):
    x = np.asarray(x, dtype=np.float64)
    c = np.sqrt(2.0 / np.pi)
    t = np.tanh(c * (x + 0.044715 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3 * 0.044715 * x * x)


def silu(x):
    """x * sigmoid(x), as oracle/llama_numpy.py."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def silu_grad(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def interleave_gate_up(gate, up):
    """Rows of the gate and the up matrix in groups of 32, gate then up (the weight packer's layout): [2 F, K]."""
    f = gate.shape[0]
    assert f % 32 == 0 and up.shape == gate.shape
    return np.stack([gate.reshape(f // 32, 32, -1), up.reshape(f // 32, 32, -1)], axis=1).reshape(2 * f, -1)


def deinterleave_gate_up(x, axis=0):
    """Inverse of interleave_gate_up along `axis`: (gate, up)."""
    x = np.moveaxis(np.asarray(x), axis, 0)
    n = x.shape[0]
    assert n % 64 == 0
    y = x.reshape(n // 64, 2, 32, *x.shape[1:])
    g, u = y[:, 0].reshape(n // 2, *x.shape[1:]), y[:, 1].reshape(n // 2, *x.shape[1:])
    return np.moveaxis(g, 0, axis), np.moveaxis(u, 0, axis)


def f16_sat(x):
    """fp64 -> fp16, round to nearest even, saturating at +-65504 (common.h: f2h_sat).  Goes through fp32 like the kernels; the
    double rounding is harmless for the exact tier (integers below 2^24 are fp32 values)."""
    x32 = np.clip(np.asarray(x, dtype=np.float64), -F16_MAX, F16_MAX).astype(np.float32)
    return x32.astype(np.float16)


def consumer_factor(K, eps, rowscale=None, ssq_in=None):
    """Row factor of the folded-RMSNorm consumer: given, or rsqrt(sum(ssq_in) / K + eps) / xs.  [M] fp64 (1 without a fold)."""
    if rowscale is not None:
        return np.asarray(rowscale, dtype=np.float64)
    if ssq_in is not None:
        return 1.0 / np.sqrt(np.asarray(ssq_in, dtype=np.float64).sum(axis=1) / K + eps) / XS
    return None


def expected(epi, a16, w16, *, c_in=None, factor=None, labels=None, acc=None):
    """fp64 expected output of one epilogue on the logical [M, N] problem (addressing is the caller's business).
    acc: acc64(a16, w16) where the caller already holds it (one fp64 product shared by several tests).
    Returns a dict: "out" (fp64, before any rounding to the output type), and for the block epilogues "max", "idx" / "sumexp",
    "xlab"; for the gated ones also "lip" (the Lipschitz factor of the output in the accumulators)."""
    acc = acc64(a16, w16) if acc is None else np.asarray(acc, dtype=np.float64)
    if factor is not None:
        acc = acc * np.asarray(factor, dtype=np.float64)[:, None]
    if epi == EPI_STORE_F16 or epi == EPI_STORE_F32:
        return {"out": acc, "lip": 1.0}
    if epi == EPI_RESID_F32:
        return {"out": np.asarray(c_in, dtype=np.float64) + acc, "lip": 1.0}
    if epi == EPI_RELU_F16:
        return {"out": np.maximum(acc, 0.0), "lip": 1.0}
    if epi in GATED:
        g, u = deinterleave_gate_up(acc, axis=1)
        act, grad = (gelu_new, gelu_new_grad) if epi == EPI_GEGLU_F16 else (silu, silu_grad)
        return {"out": act(g) * u, "lip": np.abs(grad(g)) * np.abs(u) + np.abs(act(g))}
    m, n = acc.shape
    nblk = -(-n // 32)
    pad = np.full((m, nblk * 32), -np.inf)
    pad[:, :n] = acc
    blk = pad.reshape(m, nblk, 32)
    mx = blk.max(axis=2)
    if epi == EPI_ARGMAX_F32:
        return {"max": mx, "idx": blk.argmax(axis=2) + 32 * np.arange(nblk)[None, :]}      # argmax: the FIRST maximum
    se = np.exp(blk - mx[:, :, None]).sum(axis=2)
    lab = np.asarray(labels)
    return {"max": mx, "sumexp": se, "xlab": acc[np.arange(m), lab]}


def producer_expected(c_out, nblock_cols):
    """Producer side of the folded norm from the NEW fp32 rows c_out [M, N]: xraw = fp16_sat(c_out * xs), and the sums of squares
    of each row's blocks of nblock_cols valid columns (the last block may be partial)."""
    c = np.asarray(c_out, dtype=np.float64)
    m, n = c.shape
    nb = -(-n // nblock_cols)
    pad = np.zeros((m, nb * nblock_cols))
    pad[:, :n] = c
    return f16_sat(c * XS), (pad ** 2).reshape(m, nb, nblock_cols).sum(axis=2)


def gemv_block_bounds(n_out, n_cu):
    """Column ranges of the few-row GEMV kernel's workgroups (gemv_rows.h): its producer writes one partial per workgroup."""
    g = min(n_cu, -(-n_out // 4))
    cb = -(-n_out // g)
    return [(min(n_out, i * cb), min(n_out, (i + 1) * cb)) for i in range(g)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def int_operands(rs, m, n, k, amax=4):
    """Tier A operands: integers in [-amax, amax] as fp16."""
    assert amax <= 4 and k <= 1024
    return rs.randint(-amax, amax + 1, size=(m, k)).astype(np.float16), rs.randint(-amax, amax + 1, size=(n, k)).astype(np.float16)


def int_operands_big(rs, m, n, k, amax=4):
    """Tier A operands whose first row reaches sums above 2048 (K > 128), where fp16 has steps of 2 .. 8: column 0 = 16 K, column
    1 = 12 x (an odd count) + 16 x (the rest), never a multiple of 8 - fp16 roundings of it are visible."""
    a, w = int_operands(rs, m, n, k, amax)
    a[0] = 4
    w[0] = 4
    if n > 1:
        v = rs.choice([3, 4], size=k)
        if (v == 3).sum() % 2 == 0:
            v[0] = 7 - v[0]
        w[1] = v
    return a, w


def normal_operands(rs, m, n, k, outliers=False):
    """Tier B operands: N(0, 1) as fp16; outliers: a few A columns x 100 (as _synth.with_outlier_channels shapes a stream)."""
    a = rs.standard_normal((m, k)).astype(np.float32)
    w = rs.standard_normal((n, k)).astype(np.float16)
    if outliers:
        for c in (17, 300, 777):
            a[:, c % k] *= 100.0
    return a.astype(np.float16), w


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def chain_error(a16, w16, max_rows=16, max_cols=256):
    """E32: max |k-ordered fp32 chain of the exact products - fp64| over a fixed sample (evenly spaced rows / columns, first and
    last included) of the problem."""
    m, n = a16.shape[0], w16.shape[0]
    rows = np.unique(np.linspace(0, m - 1, min(m, max_rows)).round().astype(int))
    cols = np.unique(np.linspace(0, n - 1, min(n, max_cols)).round().astype(int))
    a = a16[rows].astype(np.float64)
    w = w16[cols].astype(np.float64)
    worst = 0.0
    for i in range(len(rows)):
        prod = w * a[i][None, :]                                  # exact: 11-bit x 11-bit significands
        chain = np.cumsum(prod.astype(np.float32), axis=1, dtype=np.float32)[:, -1]
        worst = max(worst, float(np.abs(chain.astype(np.float64) - prod.sum(axis=1)).max()))
    return worst


def tau(a16, w16):
    """Allowed accumulator error of a legitimate fp32 summation of the problem: 4 E32 (module docstring)."""
    return 4.0 * chain_error(a16, w16)


def factor_rel_error(nb_in):
    """Relative error of a row factor the kernel forms ITSELF from nb_in fp32 block sums, from the formats: a sum of nb_in positive
    fp32 terms (nb_in half-ulps), the division by K, the addition of eps, the 1-ulp hardware rsqrt (two half-ulps), and the two
    multiplications that bring it onto the accumulator: (nb_in + 8) 2^-24.  0 for a given rowscale (fp32 values, applied exactly
    up to the product's own rounding, which the output terms cover)."""
    return (nb_in + 8) * U24


def tol_f32(want, t, factor=None, frel=0.0, mag=None):
    """fp32 outputs: tau (scaled by the row factor, which multiplies the accumulator) + the fp32 rounding of the result
    (+ frel x the scaled accumulator's magnitude `mag` when the kernel formed the factor itself: factor_rel_error)."""
    f = 1.0 if factor is None else np.abs(np.asarray(factor, dtype=np.float64))[:, None]
    return t * f + U24 * np.abs(want) + frel * (np.abs(want) if mag is None else mag)


def tol_f16(want, t, lip=1.0, factor=None, frel=0.0, mag=None):
    """fp16 outputs: half an fp16 ulp (+ 2^-17 for the 1-ulp hardware exp2 / rcp of the gated ones), the smallest subnormal step,
    and the accumulator error through the epilogue function (Lipschitz factor lip, from the fp64 reference)."""
    f = 1.0 if factor is None else np.abs(np.asarray(factor, dtype=np.float64))[:, None]
    return (U16 + 2.0 ** -17) * np.abs(want) + 2.0 ** -25 + lip * t * f + frel * (np.abs(want) if mag is None else mag)


def check_f32(got, want, t, what="", factor=None, frel=0.0, mag=None):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err, tol = np.abs(got - want), tol_f32(want, t, factor, frel, mag)
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} fp32 outputs off; worst err {err.max():.3e} (tau {t:.3e}) at {np.unravel_index((err - tol).argmax(), err.shape)}"
    return float(err.max())


def check_f16(got16, want, t, what="", lip=1.0, factor=None, frel=0.0, mag=None):
    """fp16 outputs within tol_f16; exactly +-65504 wherever |want| exceeds 65504 by more than the tolerance; finite everywhere."""
    got = np.asarray(got16).astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite fp16 output (inf instead of saturation?)"
    tol = tol_f16(want, t, lip, factor, frel, mag)
    clipped = np.clip(want, -F16_MAX, F16_MAX)
    err = np.abs(got - clipped)
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} fp16 outputs off; worst err {err.max():.3e} vs tol {tol[np.unravel_index(err.argmax(), err.shape)]:.3e} at {np.unravel_index((err - tol).argmax(), err.shape)}"
    over = np.abs(want) > F16_MAX + tol
    assert (np.abs(got[over]) == F16_MAX).all() and (np.sign(got[over]) == np.sign(want[over])).all(), f"{what}: not saturated at +-65504"
    return float(err.max())


def check_sumexp(got, want, t, what=""):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    rel = np.abs(got - want) / want
    assert (rel <= 2.0 ** -17 + t).all(), f"{what}: block sum-of-exp off by {rel.max():.3e} relative (allowed {2.0 ** -17 + t:.3e})"
    return float(rel.max())


def check_ssq(got, c_out_device, bounds_or_cols, what=""):
    """ssq against fp64 squares of the DEVICE's own new rows: relative 64 x 2^-24 (a sum of at most 64 fp32 squares, any order;
    the few-row kernel's longer blocks are chains of fmas: the bound scales with the block length / 64)."""
    c = np.asarray(c_out_device, dtype=np.float64)
    if isinstance(bounds_or_cols, int):
        bounds = [(b, min(c.shape[1], b + bounds_or_cols)) for b in range(0, c.shape[1], bounds_or_cols)]
    else:
        bounds = bounds_or_cols
    want = np.stack([(c[:, lo:hi] ** 2).sum(axis=1) for lo, hi in bounds], axis=1)
    length = max(1, max(hi - lo for lo, hi in bounds))
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    tol = max(1.0, length / 64.0) * 64 * U24 * want
    assert (np.abs(got - want) <= tol).all(), f"{what}: ssq off by {(np.abs(got - want) / np.maximum(want, 1e-300)).max():.3e} relative"


# ---- mutants (numpy emulations of subtly wrong kernels; tests/test_gemm_ref_host.py proves the checks reject them) -------------
def blocked_sum_f32(a16, w16, block=64, round_acc_f16=False):
    """An honest kernel's accumulator: fp32 sums of the exact products inside blocks of `block` k, fp32 across blocks.
    round_acc_f16: the MUTANT that rounds its accumulator to fp16 after every block."""
    m, k = a16.shape
    a, w = a16.astype(np.float32), w16.astype(np.float32)
    acc = np.zeros((m, w16.shape[0]), dtype=np.float32)
    for k0 in range(0, k, block):
        part = np.zeros_like(acc)
        for kk in range(k0, min(k, k0 + block), 16):             # MFMA k16 groups
            part = part + (a[:, kk:kk + 16].astype(np.float64) @ w[:, kk:kk + 16].astype(np.float64).T).astype(np.float32)
        acc = acc + part
        if round_acc_f16:
            acc = acc.astype(np.float16).astype(np.float32)
    return acc


# ---- the contract (mirror of gemm_contract / plan_gemm in csrc/rk_engine.hip; DESIGN.md "GEMM contract") -----------------------
def contract_violation(family, epi, M, N, K, *, lda=None, ldw=None, ldc=None, c_off=0, n_split=0, split_stride=0, batch=1,
                       bsA=0, bsW=0, bsC=0, consumer=None, producer=False, pp2=False):
    """None when the kernel family runs the call as described, else the reason.  consumer: None / "rowscale" / "ssq_in";
    pp2: the plan puts rows on the ping-pong kernel (a property of the plan, reported by rk_debug_gemm_ex)."""
    gated, blocks = epi in GATED, epi in (EPI_ARGMAX_F32, EPI_LSE_F32)
    f16 = epi in F16_EPIS
    if family == STREAM and batch == 1 and (epi == EPI_LSE_F32 or n_split):
        family = TILED                                       # plan_gemm: what the weight-streaming kernel does not take goes to the tiles
    if epi not in FAMILY_HAS[family]:
        return "the family has no such epilogue"
    lda, ldw = lda or K, ldw or K
    width = -(-N // 32) if blocks else (n_split if n_split else (N // 2 if gated else N))
    ldc = ldc or width
    if lda < K or ldw < K or lda % 8 or ldw % 8 or bsA % 8 or bsW % 8:
        return "operand rows: 16-byte aligned, at least K long"
    if gated and N % 64:
        return "gated: N % 64"
    if ldc < width:
        return "ldc below the output width"
    if producer and (epi != EPI_RESID_F32 or n_split or batch > 1):
        return "producer: fp32 residual, one batch, no n_split"
    if consumer and batch > 1:
        return "consumer: one batch"
    if family == GEMV:
        if M > 16 or K % 8 or K > 3072 or batch != 1 or n_split:
            return "few-row GEMV: M <= 16, K % 8, K <= 3072, one batch, no n_split"
        return None
    piece = 8 if family == TILED and f16 else 4
    if not blocks:
        if N % piece or ldc % piece or n_split % piece or split_stride % piece or bsC % piece or c_off % piece:
            return f"{piece}-column output pieces"
        if n_split and N % n_split:
            return "n_split divides N"
    if family == STREAM:
        if K % 16:
            return "weight-streaming: K % 16"
        if batch > 1 and epi == EPI_ARGMAX_F32:
            return "argmax: one batch"
        return None
    if batch > 1:
        return contract_violation(STREAM, epi, M, N, K, lda=lda, ldw=ldw, ldc=ldc, c_off=c_off, n_split=0, batch=batch, bsA=bsA,
                                  bsW=bsW, bsC=bsC, consumer=consumer, producer=producer) if not n_split else "batch with n_split"
    if K % 64:
        return "tiled: K % 64"
    if consumer and not f16:
        return "tiled: consumer fold for fp16 epilogues only"
    if n_split and (epi == EPI_RESID_F32 or gated or blocks):
        return "tiled: n_split for plain stores only"
    if pp2 and consumer == "ssq_in":
        return "ping-pong kernel: ready-made row factors only"
    return None


# Calls OUTSIDE the contract: refused by the plan, asserted on the GPU without a launch (reading the kernels says what they would do).
REFUSED = [
    # (family, epi, M, N, K, keyword arguments, what the kernel would do)
    (TILED, EPI_STORE_F16, 33, 260, 64, {}, "half8 store of the last piece: 4 halfs past column N (next row / past C)"),
    (TILED, EPI_RELU_F16, 300, 516, 128, {}, "the same"),
    (TILED, EPI_STORE_F16, 64, 256, 64, {"ldc": 260}, "rows only 8-byte aligned: misaligned 16-byte stores"),
    (TILED, EPI_STORE_F16, 64, 256, 64, {"ldc": 512, "c_off": 4}, "column offset of 4 halfs: misaligned 16-byte stores"),
    (TILED, EPI_GEGLU_F16, 64, 96, 64, {}, "gate / up pairing needs whole groups of 64 weight rows"),
    (TILED, EPI_SWIGLU_F16, 64, 32, 64, {}, "the same"),
    (STREAM, EPI_GEGLU_F16, 8, 96, 64, {}, "the same"),
    (GEMV, EPI_GEGLU_F16, 2, 96, 64, {}, "the same"),
    (TILED, EPI_STORE_F32, 64, 66, 64, {}, "f32x4 store of the last piece: 2 floats past column N"),
    (STREAM, EPI_STORE_F16, 8, 66, 64, {}, "half4 store of the last piece: 2 halfs past column N"),
    (STREAM, EPI_RESID_F32, 8, 64, 64, {"ldc": 66}, "misaligned f32x4 rows"),
    (TILED, EPI_STORE_F32, 64, 64, 96, {}, "K tiles of 64: the last half tile would be dropped"),
    (TILED, EPI_STORE_F32, 64, 64, 32, {}, "no whole K tile: nothing summed"),
    (STREAM, EPI_STORE_F32, 8, 64, 72, {}, "k16 steps: the last 8 k would be dropped"),
    (GEMV, EPI_STORE_F32, 17, 64, 64, {}, "more rows than the kernel stages"),
    (GEMV, EPI_STORE_F32, 4, 64, 3136, {}, "more than six 16-byte pieces per lane"),
    (GEMV, EPI_STORE_F32, 4, 64, 68, {}, "K in 16-byte pieces"),
    (GEMV, EPI_ARGMAX_F32, 4, 64, 64, {}, "no such instantiation"),
    (GEMV, EPI_SWIGLU_F16, 4, 64, 64, {}, "no such instantiation"),
    (TILED, EPI_ARGMAX_F32, 64, 64, 64, {}, "no such instantiation"),
    (STREAM, EPI_LSE_F32, 8, 64, 64, {"batch": 2, "bsA": 64, "bsW": 64 * 64, "bsC": 2, "lda": 128, "ldc": 4}, "no such instantiation (one batch runs on the tiles)"),
    (TILED, EPI_STORE_F32, 64, 64, 64, {"lda": 68}, "operand rows not 16-byte aligned"),
    (TILED, EPI_STORE_F32, 64, 64, 64, {"ldc": 60}, "rows overlap"),
    (TILED, EPI_RESID_F32, 64, 64, 64, {"consumer": "rowscale"}, "the prefetching residual epilogues never read the row factors: silently unscaled"),
    (TILED, EPI_STORE_F32, 64, 64, 128, {"consumer": "rowscale"}, "the ping-pong kernel's fp32 instantiations never read the row factors"),
    (TILED, EPI_LSE_F32, 64, 64, 128, {"consumer": "ssq_in"}, "the same"),
    (TILED, EPI_RESID_F32, 64, 128, 64, {"n_split": 64, "split_stride": 64 * 64, "ldc": 64}, "the old-row prefetch ignores n_split"),
    (TILED, EPI_GEGLU_F16, 64, 128, 64, {"n_split": 32, "split_stride": 64 * 32, "ldc": 32}, "n_split would apply to halved columns"),
    (TILED, EPI_STORE_F16, 64, 128, 64, {"n_split": 48, "split_stride": 64 * 48, "ldc": 48}, "n_split must divide N"),
    (TILED, EPI_STORE_F16, 64, 128, 64, {"producer": True}, "producer statistics exist in the fp32 residual epilogue only"),
    (TILED, EPI_RESID_F32, 64, 128, 64, {"producer": True, "n_split": 64, "split_stride": 64 * 64, "ldc": 64}, "xraw / ssq ignore n_split"),
    (STREAM, EPI_RESID_F32, 8, 64, 64, {"producer": True, "batch": 2, "bsA": 64, "bsW": 64 * 64, "bsC": 64, "lda": 128, "ldc": 128},
     "xraw / ssq are not offset per batch: every batch would write the same rows"),
    (STREAM, EPI_ARGMAX_F32, 8, 64, 64, {"batch": 2, "bsA": 64, "bsW": 64 * 64, "bsC": 2, "lda": 128, "ldc": 4}, "the index buffer is not offset per batch"),
    (STREAM, EPI_STORE_F16, 8, 64, 64, {"consumer": "rowscale", "batch": 2, "bsA": 64, "bsW": 64 * 64, "bsC": 64, "lda": 128, "ldc": 128}, "row factors per batch do not exist"),
]
