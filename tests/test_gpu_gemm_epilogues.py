"""Every epilogue of the engine's GEMM on every kernel family against an fp64 reference (tests/_gemm_ref.py), through
rk_debug_gemm_ex: the call goes through plan_gemm and the launchers as the engine's own calls do, every output sits between
sentinel bands.

Tier A: integer operands - bit for bit.  Tier B: N(0, 1) operands (every second case with outlier channels) - within tau = 4 E32,
E32 = the error of a k-ordered fp32 chain on a sample of the very problem (never a figure read off a kernel).
Every case: sentinels intact in both bands, every pad column and every row >= M; a second run gives the same bytes; the
producer's block count is the plan's; the plan agrees with the Python mirror of the contract.

RATIOS (max error / E32 per family, tier B) are collected for the record (printed by the last test, quoted in DESIGN.md); they are
not bounds."""
import numpy as np
import pytest

import _gemm_ref as R
from conftest import load_state

pytestmark = pytest.mark.gpu

BAND_ROWS = 256
RATIOS = {}                # family name -> largest observed accumulator error / E32
# tiled "variants": (option gemm_variant, option gemm_glds)
TILED_VARIANTS = [(1, 1), (1, 0), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1)]
M_TILED = [1, 31, 33, 64, 65, 255, 257, 300, 777]
N_F16 = [64, 72, 128, 136, 192, 200, 256, 264, 520]              # around 64 / 128 / 192 / 256 multiples, 8-column pieces
N_F32 = [64, 68, 128, 132, 192, 196, 256, 260, 516]              # ... 4-column pieces, N = 8 j + 4 among them
N_GATED = [64, 128, 192, 256, 320, 384, 448, 512, 576]
N_BLOCKS = [33, 64, 100, 128, 191, 192, 257, 260, 515]           # the block epilogues take any N
K_ALL = [64, 128, 192, 1024, 2816]


@pytest.fixture(scope="module")
def eng(ckpt_dirs):
    from llmrankers._engine import RkEngine
    dims, state = load_state(ckpt_dirs["ckpt_gated_untied"])
    e = RkEngine(dims, device=0, max_tokens=2048, max_seqs=16, max_dec_len=8).load_state(state.items())
    e.gemm_info = e.debug_gemm_ex(R.EPI_STORE_F32, R.TILED, np.zeros(64, np.float16), np.zeros(64 * 64, np.float16), 1, 64, 64, plan_only=True)
    yield e
    e.close()


class Options:
    """Engine options for the length of a block, restored to the defaults after it."""
    DEFAULTS = {"gemm_variant": 0, "gemm_glds": 1, "gemm_sk": 1, "gemm_s64_stages": 0, "gemm_split": 1, "gemm_persistent": 1}

    def __init__(self, eng, **kw):
        self.eng, self.kw = eng, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.eng.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.eng.set_option(k, self.DEFAULTS[k])


def _sentinel_array(n, dtype):
    return np.frombuffer(bytes([R.SENTINEL]) * (n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def _pad_rows(x, ld, fill):
    """[rows, k] -> flat [rows * ld] with the pad columns = fill (NaN: a kernel that reads them poisons its result)."""
    out = np.full((x.shape[0], ld), fill, dtype=np.float16)
    out[:, :x.shape[1]] = x
    return out.reshape(-1)


def run_case(eng, fam, epi, M, N, K, tier, seed, *, layout=0, consumer=None, producer=False, outliers=False, n_split=0,
             split_stride=0, heads=None, big=True, what=""):
    """One call, both runs, every assertion.  Returns the plan.  layout: 0 tight, 1 padded lda / ldw / ldc, 2 ldc = 3 x width with
    a column offset (the fused-QKV / `dq + r0 * I` form).  heads: (batch, bsA, bsW, bsC, lda, ldw, ldc) of a .heads() call."""
    rs = np.random.RandomState(seed)
    gated, blocks = epi in R.GATED, epi in (R.EPI_ARGMAX_F32, R.EPI_LSE_F32)
    f16 = epi in R.F16_EPIS
    batch = heads[0] if heads else 1
    what = what or f"family {fam} {R.EPI_NAMES[epi]} M={M} N={N} K={K} tier {tier} layout {layout} consumer {consumer} producer {producer}"
    # ---- operands ----
    probs = []
    for b in range(batch):
        if tier == "A":
            a, w = (R.int_operands_big if big and not producer else R.int_operands)(rs, M, N, K, amax=1 if producer else 4)
            if epi == R.EPI_ARGMAX_F32 and N >= 41:           # exact ties: inside a block, across blocks, in the last (partial) block
                w[40 % N] = w[35]
                w[N - 1] = w[N - 2]
                if N > 70:
                    w[70] = w[35]
        else:
            a, w = R.normal_operands(rs, M, N, K, outliers)
        probs.append((a, w))
    width = -(-N // 32) if blocks else (n_split if n_split else (N // 2 if gated else N))
    piece = 1 if (blocks or fam == R.GEMV) else (8 if fam == R.TILED and f16 else 4)
    if heads:
        _, bsA, bsW, bsC, lda, ldw, ldc = heads
        c_off = 0
        a_flat = np.full(M * lda, np.nan, dtype=np.float16).reshape(M, lda)
        w_flat = np.full((batch - 1) * bsW + N * ldw, np.nan, dtype=np.float16)
        for b, (a, w) in enumerate(probs):
            a_flat[:, b * bsA:b * bsA + K] = a
            w_flat[b * bsW:b * bsW + N * ldw].reshape(N, ldw)[:, :K] = w
        a_flat = a_flat.reshape(-1)
    else:
        bsA = bsW = bsC = 0
        lda, ldw = (K, K) if layout == 0 else (K + 8, K + 16)
        ldc, c_off = {0: (width, 0), 1: (width + 3 * piece, 0), 2: (3 * width, width)}[layout]
        if layout == 2 and width % piece:
            ldc, c_off = 3 * width + (piece - 3 * width % piece) % piece, -(-width // piece) * piece
        a_flat, w_flat = _pad_rows(probs[0][0], lda, np.nan), _pad_rows(probs[0][1], ldw, np.nan)
    nsb = N // n_split if n_split else 1
    split_stride = split_stride or (M * ldc + 5 * 8 if n_split else 0)
    # ---- where the call's outputs live inside the interior ----
    bb, mm, nn = np.meshgrid(np.arange(batch), np.arange(M), np.arange(nsb * width if n_split else width), indexing="ij")
    pos = c_off + bb * bsC + mm * ldc + ((nn // n_split) * split_stride + nn % n_split if n_split else nn)
    c_elems = int(pos.max()) + 1 if not heads else M * ldc
    dt = np.float16 if f16 else np.float32
    per = 2 if epi == R.EPI_LSE_F32 else 1
    c_in = _sentinel_array(c_elems * per, dt)
    c_old = None
    if epi == R.EPI_RESID_F32:
        c_old = [(rs.randint(-64, 65, size=(M, N)) if tier == "A" else rs.standard_normal((M, N))).astype(np.float32) for _ in range(batch)]
        for b in range(batch):
            c_in[pos[b]] = c_old[b]
    # ---- the fold ----
    kw = {}
    factor, frel = None, 0.0
    eps = eng.gemm_info["eps"]
    if consumer == "rowscale":
        rsc = (2.0 ** rs.randint(-3, 4, size=M)).astype(np.float32) if tier == "A" else rs.uniform(0.5, 2.0, size=M).astype(np.float32)
        if tier == "A" and f16:
            rsc[0] = 64.0                                     # the big row saturates: 16 K x 64 > 65504
        kw["rowscale"] = rsc
        factor = R.consumer_factor(K, eps, rowscale=rsc)
    elif consumer == "ssq_in":
        nb_in = [4, 7, 16, 33, 80][seed % 5]                 # DMA path (nb_in % 4 == 0, <= 64), scalar path, beyond 64
        ssq_in = (rs.uniform(0.5, 2.0, size=(M, nb_in)) * K * 256.0 / nb_in).astype(np.float32)    # mean square ~ 1 / xs^2: factors near 1
        kw["ssq_in"] = ssq_in
        factor, frel = R.consumer_factor(K, eps, ssq_in=ssq_in), R.factor_rel_error(nb_in)
    labels = rs.randint(0, N, size=M).astype(np.int32) if epi == R.EPI_LSE_F32 else None
    call = dict(lda=lda, ldw=ldw, ldc=ldc, c_in=c_in, c_off=c_off, producer=producer, n_split=n_split, split_stride=split_stride,
                batch=batch, bsA=bsA, bsW=bsW, bsC=bsC, labels=labels, **kw)
    # ---- the plan agrees with the mirror of the contract ----
    plan = eng.debug_gemm_ex(epi, fam, a_flat, w_flat, M, N, K, plan_only=True, **call)
    pp2 = plan["family"] == R.TILED and (plan["m_pp2"] > 0 or plan["variant"] == 5)
    assert R.contract_violation(fam, epi, M, N, K, lda=lda, ldw=ldw, ldc=ldc, c_off=c_off, n_split=n_split, split_stride=split_stride,
                                batch=batch, bsA=bsA, bsW=bsW, bsC=bsC, consumer=consumer, producer=producer, pp2=pp2) is None, what
    # ---- two runs: the same bytes ----
    r = eng.debug_gemm_ex(epi, fam, a_flat, w_flat, M, N, K, **call)
    r2 = eng.debug_gemm_ex(epi, fam, a_flat, w_flat, M, N, K, **call)
    for key in ("C", "idx", "xraw", "ssq", "xlab"):
        if r.get(key) is not None:
            assert r[key].tobytes() == r2[key].tobytes(), f"{what}: {key} differs between two runs"
    assert (r["family"], r["variant"], r["m_pp2"], r["nb"]) == (plan["family"], plan["variant"], plan["m_pp2"], plan["nb"]), what
    # ---- sentinels: bands, pad columns, rows >= M ----
    band = r["band"]
    full = r["C"].reshape(-1, per) if per == 2 else r["C"]
    owned = np.zeros(2 * band + c_elems, dtype=bool)
    owned[band + pos.reshape(-1)] = True
    raw = full.view(np.uint8).reshape(2 * band + c_elems, -1)
    stray = np.where((raw[~owned] != R.SENTINEL).any(axis=1))[0]
    assert stray.size == 0, f"{what}: {stray.size} elements outside the call's [M, N] were written, first at flat offset {np.where(~owned)[0][stray[0]] - band} of the interior (ldc {ldc})"
    if r["idx"] is not None:
        assert (r["idx"].view(np.uint8).reshape(-1, 4)[~owned] == R.SENTINEL).all(), f"{what}: index buffer written outside [M, blocks]"
    # ---- results ----
    nb_cols = {R.TILED: 64, R.STREAM: 32}.get(r["family"])
    for b, (a, w) in enumerate(probs):
        got = full[band + pos[b]]
        t = 0.0 if tier == "A" else R.tau(a, w)
        e = R.expected(epi, a, w, c_in=None if c_old is None else c_old[b], factor=factor, labels=labels)
        e32 = t / 4.0
        tag = f"{what} batch {b}"
        mag = None if factor is None else np.abs(R.acc64(a, w) * factor[:, None])    # what the factor's own error multiplies
        if epi in (R.EPI_STORE_F32, R.EPI_RESID_F32):
            if tier == "A":
                np.testing.assert_array_equal(got.astype(np.float64), e["out"], err_msg=tag)
            else:
                err = R.check_f32(got, e["out"], t, tag, factor=factor, frel=frel, mag=mag)
                if factor is None:
                    _record(r["family"], err, e32)
        elif f16:
            if tier == "A" and not gated:
                np.testing.assert_array_equal(got.astype(np.float32), R.f16_sat(e["out"]).astype(np.float32), err_msg=tag)
                if consumer == "rowscale" and big and K > 16:
                    assert (np.abs(got[0].astype(np.float64)) == R.F16_MAX).any(), f"{tag}: the saturating row never saturated"
            else:
                gmag = None if mag is None or not gated else 2.0 * e["lip"] * np.maximum(*[np.abs(x) for x in R.deinterleave_gate_up(mag, axis=1)])
                R.check_f16(got, e["out"], t, tag, lip=e["lip"], factor=factor, frel=frel, mag=gmag if gated else mag)
        elif epi == R.EPI_ARGMAX_F32:
            idx = r["idx"][band + pos[b]]
            if tier == "A":
                np.testing.assert_array_equal(got.astype(np.float64), e["max"], err_msg=tag)
                np.testing.assert_array_equal(idx, e["idx"], err_msg=f"{tag}: first index of the block maximum")
            else:
                R.check_f32(got, e["max"], t, tag, factor=factor, frel=frel)
                acc = R.acc64(a, w) * (1.0 if factor is None else factor[:, None])
                lo = 32 * np.arange(idx.shape[1])[None, :]
                assert ((idx >= lo) & (idx < np.minimum(lo + 32, N))).all(), f"{tag}: index outside its block"
                picked = np.take_along_axis(acc, idx, axis=1)
                assert (picked >= e["max"] - 2 * R.tol_f32(e["max"], t, factor, frel)).all(), f"{tag}: index of a column that is not the maximum"
        else:
            mx, se = got[..., 0], got[..., 1]
            if tier == "A":
                np.testing.assert_array_equal(mx.astype(np.float64), e["max"], err_msg=tag)
                np.testing.assert_array_equal(r["xlab"].astype(np.float64), e["xlab"], err_msg=f"{tag}: label logit")
            else:
                err = R.check_f32(mx, e["max"], t, tag)
                R.check_f32(r["xlab"][:, None], e["xlab"][:, None], t, f"{tag}: label logit")
                _record(r["family"], err, e32)
            R.check_sumexp(se, e["sumexp"], t, tag)
        if producer:
            rows = slice(BAND_ROWS, BAND_ROWS + M)
            for key in ("xraw", "ssq"):
                outside = np.ones(r[key].shape[0], dtype=bool)
                outside[rows] = False
                assert (r[key][outside].view(np.uint8) == R.SENTINEL).all(), f"{tag}: {key} written outside its [M, ...] rows"
            bounds = R.gemv_block_bounds(N, r["n_cu"]) if r["family"] == R.GEMV else nb_cols
            want_nb = len(bounds) if r["family"] == R.GEMV else -(-N // nb_cols)
            assert r["nb"] == want_nb == r["ssq"].shape[1], f"{tag}: producer blocks {r['nb']} (plan) vs {want_nb}"
            assert np.isfinite(r["ssq"][rows]).all() and np.isfinite(r["xraw"][rows].astype(np.float32)).all(), tag
            if tier == "A":
                xr, _ = R.producer_expected(e["out"], 64)
                np.testing.assert_array_equal(r["xraw"][rows].view(np.uint16), xr.view(np.uint16), err_msg=f"{tag}: xraw")
                c64 = e["out"]
                bl = bounds if r["family"] == R.GEMV else [(lo, min(N, lo + nb_cols)) for lo in range(0, N, nb_cols)]
                want_ssq = np.stack([(c64[:, lo:hi] ** 2).sum(axis=1) for lo, hi in bl], axis=1)
                assert want_ssq.max() < 2 ** 24, "the case's sums of squares leave the exact range: change its inputs"
                np.testing.assert_array_equal(r["ssq"][rows].astype(np.float64), want_ssq, err_msg=f"{tag}: ssq")
            else:
                R.check_ssq(r["ssq"][rows], got, bounds, f"{tag}: ssq")
                xr, _ = R.producer_expected(got, 64)                           # from the device's own new rows: one rounding
                np.testing.assert_array_equal(r["xraw"][rows].view(np.uint16), xr.view(np.uint16), err_msg=f"{tag}: xraw")
    return r


def _record(family, err, e32):
    if e32 > 0:
        name = {R.TILED: "tiled", R.STREAM: "stream", R.GEMV: "gemv"}[family]
        RATIOS[name] = max(RATIOS.get(name, 0.0), err / e32)


def _n_list(fam, epi):
    if epi in R.GATED:
        return N_GATED
    if epi in (R.EPI_ARGMAX_F32, R.EPI_LSE_F32):
        return N_BLOCKS
    if fam == R.GEMV:
        return [5, 36, 64, 100, 261, 516, 1024, 2052, 8]
    return N_F16 if fam == R.TILED and epi in R.F16_EPIS else N_F32


def _consumers(fam, epi):
    """Consumer-fold forms the (family, epilogue) admits, cycled through the cases (None first)."""
    if fam == R.TILED:
        return [None, "rowscale", "ssq_in"] if epi in R.F16_EPIS else [None]
    return [None, "rowscale", "ssq_in"]


def _sweep(eng, fam, epi, tier, ms, ks, seed0):
    ns = _n_list(fam, epi)
    cons = _consumers(fam, epi)
    ks = [k for k in ks if tier == "B" or k <= 1024]
    for i, m in enumerate(ms):
        n, k = ns[(i + seed0) % len(ns)], ks[(i + seed0 // 3) % len(ks)]
        consumer = cons[(i + seed0) % len(cons)]
        if tier == "A" and consumer == "ssq_in":
            consumer = "rowscale"                               # exact tier: power-of-two factors only
        if consumer == "ssq_in" and fam == R.TILED:
            plan = eng.debug_gemm_ex(epi, fam, np.zeros(k, np.float16), np.zeros(k, np.float16), m, n, k, plan_only=True)
            if plan["m_pp2"] > 0 or plan["variant"] == 5:
                consumer = "rowscale"                           # the ping-pong kernel takes ready-made factors (contract)
        producer = epi == R.EPI_RESID_F32 and (i % 2 == 1 or n % 64 != 0)      # every partial last block of the statistics
        if tier == "A" and producer:
            consumer = None                                     # (scaled rows would carry fraction bits into the exact sums of squares)
        run_case(eng, fam, epi, m, n, k, tier, 1000 * seed0 + i, layout=i % 3, consumer=consumer, producer=producer, outliers=i % 2 == 0)


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("epi", R.FAMILY_HAS[R.TILED], ids=lambda e: R.EPI_NAMES[e])
@pytest.mark.parametrize("variant,glds", TILED_VARIANTS)
def test_tiled_family(eng, variant, glds, epi, tier):
    """Tile variants 1 (both stagings) .. 6: every epilogue the tiles have, M with partial tiles in every tile height, N around the
    tile widths (N = 8 j + 4 for the fp32 epilogues), every K, tight and padded leading dimensions, every consumer form the
    variant admits, the producer on every second residual case and on every N with a partial last statistics block."""
    with Options(eng, gemm_variant=variant, gemm_glds=glds):
        _sweep(eng, R.TILED, epi, tier, M_TILED, K_ALL, seed0=variant * 8 + epi)


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("epi", R.FAMILY_HAS[R.STREAM], ids=lambda e: R.EPI_NAMES[e])
def test_weight_streaming_family(eng, epi, tier):
    _sweep(eng, R.STREAM, epi, tier, [1, 32, 33, 74, 1, 32, 33, 74], [16, 64, 80, 192, 1024, 2816], seed0=epi)


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("epi", R.FAMILY_HAS[R.GEMV], ids=lambda e: R.EPI_NAMES[e])
def test_few_row_family(eng, epi, tier):
    _sweep(eng, R.GEMV, epi, tier, [1, 2, 3, 4, 5, 8, 9, 16], [8, 64, 72, 520, 1024, 2816, 3072], seed0=epi)


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("epi", [R.EPI_STORE_F32, R.EPI_RESID_F32], ids=lambda e: R.EPI_NAMES[e])
def test_k_split_pingpong(eng, epi, tier):
    """gemm_sk = 2: two workgroups per output tile wherever every half keeps two K tiles - the fp32 epilogues only."""
    with Options(eng, gemm_variant=5, gemm_sk=2):
        for i, (m, n, k) in enumerate([(300, 260, 1024), (777, 516, 2816 if tier == "B" else 512), (257, 256, 256), (64, 64, 384)]):
            r = run_case(eng, R.TILED, epi, m, n, k, tier, 7000 + i, layout=i % 3, producer=epi == R.EPI_RESID_F32 and i % 2 == 0)
            assert r["ksplit"] == 2, (m, n, k, r["ksplit"])


@pytest.mark.parametrize("case", [(R.EPI_STORE_F16, 300, 520, 192, "rowscale", False), (R.EPI_RESID_F32, 777, 516, 1024, None, True),
                                  (R.EPI_GEGLU_F16, 2100, 2048, 128, "rowscale", False)],       # 9 x 8 = 72 tiles: more than 64 workgroups
                         ids=lambda c: R.EPI_NAMES[c[0]])
def test_pingpong_grid_option_gives_the_same_bytes(eng, case):
    """Option gemm_persistent on the ping-pong variant: one workgroup per tile (0), 8 or 64 workgroups walking the tiles - the same
    bytes as the default (1: one workgroup per CU), which is held to the fp64 reference here; a value other than 1 plans no K split."""
    epi, m, n, k, consumer, outliers = case
    rs = np.random.RandomState(9300 + epi)
    a, w = R.normal_operands(rs, m, n, k, outliers)
    c_old = rs.standard_normal((m, n)).astype(np.float32) if epi == R.EPI_RESID_F32 else None
    rsc = rs.uniform(0.5, 2.0, size=m).astype(np.float32) if consumer else None
    width = n // 2 if epi in R.GATED else n

    def run():
        r = eng.debug_gemm_ex(epi, R.TILED, a, w, m, n, k, c_in=c_old, rowscale=rsc)
        assert r["variant"] == 5 and r["m_pp2"] == 0 and r["ksplit"] == 1, r
        assert (r["C"][:r["band"]].view(np.uint8) == R.SENTINEL).all() and (r["C"][r["band"] + m * width:].view(np.uint8) == R.SENTINEL).all()
        return r["C"]

    with Options(eng, gemm_variant=5):
        base = run()
        got = base[BAND_ROWS * width:BAND_ROWS * width + m * width].reshape(m, width)
        e = R.expected(epi, a, w, c_in=c_old, factor=None if rsc is None else rsc.astype(np.float64))
        if epi == R.EPI_RESID_F32:
            R.check_f32(got, e["out"], R.tau(a, w), R.EPI_NAMES[epi])
        else:
            R.check_f16(got, e["out"], R.tau(a, w), R.EPI_NAMES[epi], lip=e["lip"], factor=rsc)
        for value in (0, 8, 64):
            with Options(eng, gemm_persistent=value):
                assert run().tobytes() == base.tobytes(), f"{R.EPI_NAMES[epi]} {(m, n, k)}: gemm_persistent = {value} differs from 1"
    z = np.zeros(8, np.float16)
    with Options(eng, gemm_variant=5, gemm_sk=2):
        assert eng.debug_gemm_ex(R.EPI_STORE_F32, R.TILED, z, z, 300, 260, 1024, plan_only=True)["ksplit"] == 2
        for value in (0, 8, 64):
            with Options(eng, gemm_persistent=value):
                assert eng.debug_gemm_ex(R.EPI_STORE_F32, R.TILED, z, z, 300, 260, 1024, plan_only=True)["ksplit"] == 1, value


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("epi", [R.EPI_STORE_F16, R.EPI_RESID_F32, R.EPI_GEGLU_F16, R.EPI_RELU_F16], ids=lambda e: R.EPI_NAMES[e])
def test_pingpong_with_fill_in_split(eng, epi, tier):
    """plan_gemm puts whole rounds on the persistent ping-pong kernel and the rows behind them on a fill-in variant as a second
    launch with row-offset arguments (C, xraw, ssq, rowscale): M from the CU count so that m_pp2 > 0."""
    n, k = (1024, 128)
    n_cu = eng.debug_gemm_ex(epi, R.TILED, np.zeros(k, np.float16), np.zeros(n * k, np.float16), 1, n, k, plan_only=True)["n_cu"]
    wgs = n_cu & ~7
    tiles_n = -(-n // 256)
    m = (wgs // tiles_n) * 256 + 300
    consumer = "rowscale" if epi != R.EPI_RESID_F32 else None
    r = run_case(eng, R.TILED, epi, m, n, k, tier, 8000 + epi, layout=1, consumer=consumer, producer=epi == R.EPI_RESID_F32, big=False)
    assert r["m_pp2"] == (wgs // tiles_n) * 256 and r["variant"] != 5, (m, r)
    if epi != R.EPI_RESID_F32:                                   # such a plan takes no ssq_in (the ping-pong kernel has no form for it)
        from llmrankers._engine import RkError
        with pytest.raises(RkError) as ei:
            eng.debug_gemm_ex(epi, R.TILED, np.zeros(m * k, np.float16), np.zeros(n * k, np.float16), m, n, k,
                              ssq_in=np.ones((m, 4), np.float32), plan_only=True)
        assert ei.value.code == -4


@pytest.mark.parametrize("tier", ["A", "B"])
def test_heads_batches_with_the_decoder_strides(eng, tier):
    """.heads(): the two per-head projections around the query-side cross-attention (run_decoder), H = 3, d_model = 128."""
    h, dm, nr = 3, 128, 37
    inner = h * 64
    #         batch, bsA, bsW,     bsC, lda,    ldw, ldc
    run_case(eng, R.STREAM, R.EPI_STORE_F16, nr, dm, 64, tier, 9001, heads=(h, 64, dm * 64, dm, inner, 64, h * dm), big=False)
    run_case(eng, R.STREAM, R.EPI_STORE_F16, nr, 64, dm, tier, 9002, heads=(h, dm, 64 * dm, 64, h * dm, dm, inner), big=False)
    run_case(eng, R.TILED, R.EPI_STORE_F16, nr, 64, dm, tier, 9003, heads=(h, dm, 64 * dm, 64, h * dm, dm, inner), big=False)   # batch > 1: streamed whatever the caller marked


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("variant", [0, 1, 2, 5, 6])
def test_n_split_as_the_cross_kv_projection(eng, variant, tier):
    """.split(): N = layers x 2 I columns, block n / (2 I) goes to its own [max_tokens, 2 I] matrix."""
    inner2, layers, m = 2 * 192, 3, 300
    with Options(eng, gemm_variant=variant):
        run_case(eng, R.TILED, R.EPI_STORE_F16, m, layers * inner2, 128, tier, 9100 + variant, n_split=inner2, split_stride=(m + 12) * inner2)
        run_case(eng, R.TILED, R.EPI_STORE_F32, 65, 3 * 68, 192, tier, 9200 + variant, n_split=68, split_stride=70 * 68)


@pytest.mark.parametrize("prod,cons", [((R.TILED, 2), (R.TILED, 6)), ((R.TILED, 6), (R.STREAM, 0)), ((R.STREAM, 0), (R.TILED, 1)),
                                       ((R.GEMV, 0), (R.STREAM, 0)), ((R.STREAM, 0), (R.GEMV, 0)), ((R.TILED, 1), (R.TILED, 4))],
                         ids=lambda p: f"{['tiled', 'stream', 'gemv'][p[0]]}{p[1]}")
def test_producer_feeds_consumer_of_another_family(eng, prod, cons):
    """A residual GEMM leaves the fp16 copy of its new rows and their block sums of squares; a GEMM of ANOTHER family or variant
    reads both (A = xraw, ssq_in = ssq) and forms the RMSNorm row factor itself.  Against the fp64 reference of the whole chain,
    and bit-equal to the same consumer fed with the factors rowscale_kernel makes of the same sums (tiled and weight-streaming
    consumers: they add the block sums in rowscale_kernel's order - rk_row_factor; the few-row kernel adds them lane-strided and
    through a tree, its passes never mix with the others', so it is held to the reference only)."""
    rs = np.random.RandomState(prod[0] * 10 + cons[0])
    m, d, k1, n2 = 13, 256, 192, 136
    a1, w1 = R.normal_operands(rs, m, d, k1)
    c0 = rs.standard_normal((m, d)).astype(np.float32)
    with Options(eng, gemm_variant=prod[1]):
        p = eng.debug_gemm_ex(R.EPI_RESID_F32, prod[0], a1, w1, m, d, k1, c_in=c0, producer=True)
    rows = slice(BAND_ROWS, BAND_ROWS + m)
    xraw, ssq = p["xraw"][rows], p["ssq"][rows]
    w2 = rs.standard_normal((n2, d)).astype(np.float16)
    with Options(eng, gemm_variant=cons[1]):
        own = eng.debug_gemm_ex(R.EPI_STORE_F16, cons[0], xraw, w2, m, n2, d, ssq_in=ssq)
        ker = eng.debug_gemm_ex(R.EPI_STORE_F16, cons[0], xraw, w2, m, n2, d, ssq_in=ssq, factors_kernel=True)
    if cons[0] != R.GEMV:
        assert own["C"].tobytes() == ker["C"].tobytes(), "epilogue-formed row factors differ from rowscale_kernel's"
    got = own["C"][own["band"]:own["band"] + m * n2].reshape(m, n2)
    assert (own["C"][:own["band"]].view(np.uint8) == R.SENTINEL).all() and (own["C"][own["band"] + m * n2:].view(np.uint8) == R.SENTINEL).all()
    # fp64 reference of the chain: new rows, their RMS, the normalised rows times W2
    c1 = c0.astype(np.float64) + R.acc64(a1, w1)
    want = (c1 / np.sqrt((c1 ** 2).mean(axis=1, keepdims=True) + own["eps"])) @ w2.astype(np.float64).T
    # Error budget, from the formats (nothing read off a kernel):
    #  (1) the result's own fp16 rounding;
    #  (2) the fp16 copy of the stream: one rounding per element, independent, each at most 2^-11 |x_k w_k| / rms: 6 standard
    #      deviations of their sum (uniform errors: 2^-11 / sqrt(3) per term, in quadrature) - one element in 1e9 exceeds it;
    #  (3) the statistics: 64 x 2^-24 relative per block sum (check_ssq's bound) plus the factor's formation, through |x||w| / rms;
    #  (4) the accumulators: tau of the first GEMM through sum |w2| / rms, tau of the second x the factor 16 / rms.
    t1, t2 = R.tau(a1, w1), R.tau(xraw, w2)
    w2d = w2.astype(np.float64)
    rms = np.sqrt((c1 ** 2).mean(axis=1, keepdims=True) + own["eps"])
    lin = (np.abs(c1) / rms) @ np.abs(w2d).T
    quad = np.sqrt(((c1 / rms) ** 2) @ (w2d ** 2).T)
    tol = (R.U16 + 2.0 ** -17) * np.abs(want) + 2.0 ** -25 + 6.0 / np.sqrt(3.0) * R.U16 * quad + lin * (64 * R.U24 + R.factor_rel_error(ssq.shape[1])) \
        + (t1 * np.abs(w2d).sum(axis=1)[None, :] + t2 * 16.0) / rms
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got.astype(np.float32)).all() and (err <= tol).all(), f"chain off by {err.max():.3e} (allowed there {tol.reshape(-1)[err.argmax()]:.3e})"


def test_calls_outside_the_contract_are_refused_without_a_launch(eng):
    """Every call of _gemm_ref.REFUSED fails with RK_ERR_STATE and the contract's reason - decided by plan_gemm before anything is
    allocated or launched (reading the kernels says what they would have done: the list's last column)."""
    from llmrankers._engine import RkError
    for fam, epi, m, n, k, kw, why in R.REFUSED:
        kw = dict(kw)
        lda, ldw = kw.pop("lda", k), kw.pop("ldw", k)
        batch = kw.get("batch", 1)
        a = np.zeros((batch - 1) * kw.get("bsA", 0) + m * lda, np.float16)
        w = np.zeros((batch - 1) * kw.get("bsW", 0) + n * ldw, np.float16)
        consumer, producer = kw.pop("consumer", None), kw.pop("producer", False)
        if consumer == "rowscale":
            kw["rowscale"] = np.ones(m, np.float32)
        elif consumer == "ssq_in":
            kw["ssq_in"] = np.ones((m, 4), np.float32)
        labels = np.zeros(m, np.int32) if epi == R.EPI_LSE_F32 else None
        for plan_only in (True, False):
            with pytest.raises(RkError) as ei:
                eng.debug_gemm_ex(epi, fam, a, w, m, n, k, lda=lda, ldw=ldw, producer=producer, labels=labels, plan_only=plan_only, **kw)
            assert ei.value.code == -4, (fam, epi, m, n, k, kw, str(ei.value))
            assert "no kernel of family" in str(ei.value)


def test_debug_entry_checks_extents_before_it_launches(eng):
    from llmrankers._engine import RkError
    a, w = np.zeros(64 * 64, np.float16), np.zeros(64 * 64, np.float16)
    with pytest.raises(RkError) as ei:                           # A one row short
        eng.debug_gemm_ex(R.EPI_STORE_F32, R.TILED, a[:63 * 64], w, 64, 64, 64)
    assert ei.value.code == -1
    with pytest.raises(RkError) as ei:                           # C interior one row short
        eng.debug_gemm_ex(R.EPI_STORE_F32, R.TILED, a, w, 64, 64, 64, c_in=np.zeros(63 * 64, np.float32))
    assert ei.value.code == -1


def test_zz_report_error_ratios():
    """For the record (DESIGN.md quotes them): the largest accumulator error / E32 each family showed in tier B."""
    print("\n[gemm] max error / E32 per family:", {k: round(v, 3) for k, v in sorted(RATIOS.items())})
    if RATIOS:                                                    # (empty when this test is selected alone)
        assert sorted(RATIOS) == ["gemv", "stream", "tiled"], RATIOS
