"""numpy restatement of the engine's FP8 step-weight format (include/rk_engine.h at rk_llama_set_weight_fp8; DESIGN.md section 3
"FP8 step weights"), for the tests that hold the engine's quantiser and its FP8 kernel against it.

A matrix W [N][K] fp16:
  groups  128 consecutive k of one row; the last may be shorter
  e       the smallest integer with absmax <= 448 * 2^e, clamped to [-15, 7]; an all-zero group takes -15
  q       OCP e4m3fn byte of w * 2^-e, round to nearest even, saturating at +-448
  d       q * 2^e - an fp16 number by construction
Nothing here imports the engine."""
import numpy as np

GROUP = 128
E_MIN, E_MAX = -15, 7
FP8_MAX = 448.0


def encode_e4m3fn(x) -> np.ndarray:
    """float64 array -> e4m3fn bytes: round to nearest even, saturating at +-448 (never the NaN encoding).  Integer / exact float64
    arithmetic only: |x| is clipped to 448, values below 2^-6 are multiples of the subnormal step 2^-9, the others keep three
    mantissa bits."""
    x = np.asarray(x, dtype=np.float64)
    sign = np.where(np.signbit(x), 0x80, 0).astype(np.uint8)
    a = np.minimum(np.abs(x), FP8_MAX)
    out = np.zeros(a.shape, dtype=np.int64)
    sub = a < 2.0 ** -6
    out[sub] = np.rint(a[sub] * 512.0).astype(np.int64)               # np.rint: ties to even; 8 = the encoding of 2^-6
    m, ex = np.frexp(a[~sub])                                          # a = m 2^ex, 0.5 <= m < 1  ->  1.f x 2^(ex - 1)
    steps = np.rint(m * 16.0).astype(np.int64)                         # 8 .. 16 eighths of 2^(ex - 1)
    carry = steps == 16
    steps = np.where(carry, 8, steps)
    ex = ex - 1 + carry
    out[~sub] = ((ex + 7) << 3) | (steps - 8)
    assert out.max(initial=0) <= 0x7E
    return (out.astype(np.uint8) | sign).astype(np.uint8)


def decode_e4m3fn(b) -> np.ndarray:
    """e4m3fn bytes -> float64 (0x7F / 0xFF, the NaN encodings, never occur in what encode_e4m3fn returns)."""
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    ex, mant = (b >> 3) & 15, b & 7
    a = np.where(ex == 0, mant * 2.0 ** -9, (1.0 + mant / 8.0) * 2.0 ** (ex - 7.0))
    return np.where(b & 0x80, -a, a)


def group_exponents(w16) -> np.ndarray:
    """[N, K] fp16 -> int8 [N, ceil(K / 128)]: per group the smallest e with absmax <= 448 * 2^e, clamped; all-zero: -15."""
    w = np.asarray(w16, dtype=np.float16).astype(np.float64)
    n, k = w.shape
    g = -(-k // GROUP)
    pad = np.zeros((n, g * GROUP))
    pad[:, :k] = np.abs(w)
    amax = pad.reshape(n, g, GROUP).max(axis=2)
    e = np.full((n, g), E_MIN, dtype=np.int64)
    nz = amax > 0
    m, ex = np.frexp(amax[nz])                                         # amax = m 2^ex, 0.5 <= m < 1;  448 = 0.875 * 2^9
    e[nz] = np.where(m <= 0.875, ex - 9, ex - 8)                       # the smallest e with m 2^ex <= 0.875 * 2^(9 + e)
    return np.clip(e, E_MIN, E_MAX).astype(np.int8)


def quantize(w16):
    """[N, K] fp16 -> (bytes uint8 [N, K], exponents int8 [N, groups], dequantised fp16 [N, K])."""
    w16 = np.asarray(w16, dtype=np.float16)
    n, k = w16.shape
    e = group_exponents(w16)
    e_k = np.repeat(e.astype(np.int64), GROUP, axis=1)[:, :k]
    q = encode_e4m3fn(np.ldexp(w16.astype(np.float64), -e_k))
    d = np.ldexp(decode_e4m3fn(q), e_k)
    d16 = d.astype(np.float16)
    assert (d16.astype(np.float64) == d).all(), "a dequantised weight is not an fp16 number"
    return q, e, d16


def dequantize(q, e, k=None) -> np.ndarray:
    q = np.asarray(q, dtype=np.uint8)
    e_k = np.repeat(np.asarray(e).astype(np.int64), GROUP, axis=1)[:, :q.shape[1]]
    return np.ldexp(decode_e4m3fn(q), e_k).astype(np.float16)


def torch_bytes(x) -> np.ndarray:
    """The same values through torch.float8_e4m3fn on the CPU (cross-check of encode_e4m3fn; |x| <= 448: torch does not saturate)."""
    import torch
    t = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.float8_e4m3fn)
    return t.view(torch.uint8).numpy().copy()


def adversarial_matrix(n=70, k=400, seed=3) -> np.ndarray:
    """fp16 [n, k] (k = 400: three full groups and a tail group of 16) holding by construction an all-zero group, a group with
    absmax 60 000 (exponent clamp at 7, saturation), a group with absmax 1e-7 (clamp at -15, results below the fp16 subnormal
    step), exact rounding ties and +-448 * 2^e boundary values."""
    rs = np.random.RandomState(seed)
    w = (rs.standard_normal((n, k)) * 0.05).astype(np.float16)
    w[1, 0:128] = 0                                                    # all-zero group
    w[2, 128:256] = (rs.standard_normal(128) * 9000).astype(np.float16)
    w[2, 130] = np.float16(60000.0)                                    # clamp at 7: 60000 / 128 = 468.75 -> saturates at 448
    w[2, 131] = np.float16(-65504.0)
    w[3, 256:384] = (rs.standard_normal(128) * 3e-8).astype(np.float16)
    w[3, 260] = np.float16(1e-7)                                       # clamp at -15: multiples of 2^-24 only
    w[3, 261] = np.float16(-2.0 ** -24)
    # exact ties at e = 0 (absmax 448): 17 -> 16, 19 -> 20, 2^-10 -> 0, 3 * 2^-10 -> 2^-8 (subnormal ties), 447 -> 448
    w[4, 0:8] = np.array([448.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 447.0, -17.0, -2.0 ** -10], dtype=np.float16)
    # +-448 * 2^e boundaries: absmax exactly 448 * 2^e keeps e; the next fp16 number above it takes e + 1
    for j, e in enumerate((-15, -9, -3, 0, 4, 7)):
        w[5 + j, 128:256] = 0
        w[5 + j, 128] = np.float16(448.0 * 2.0 ** e)
        w[5 + j, 129] = np.float16(-448.0 * 2.0 ** e)
        w[12 + j, 128:256] = 0
        w[12 + j, 128] = np.nextafter(np.float16(448.0 * 2.0 ** e), np.float16(np.inf)) if e < 7 else np.float16(65504.0)
        w[12 + j, 130] = np.float16(17.0 * 2.0 ** max(e, -14))
    w[20, 384:400] = 0                                                 # the tail group, all zero
    w[21, 384:400] = np.float16(448.0)
    return w
