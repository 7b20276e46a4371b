"""The ping-pong GEMM's timing-dependent parts - the K-split hand-off between two workgroups and the row-factor wait - run NOT
alone and NOT on the same operands twice: rk_debug_gemm_chain launches one described call several times back to back on slot 0's
encoder stream, new data per launch (every split launch uses the stream's one K-split workspace: slab and ticket addresses repeat,
the data does not), optionally beside a background GEMM on the decoder stream that covers part of the chip.

Reference and tolerances: tests/_gemm_ref.py, nothing new.  Tier A (integer operands) is compared bit for bit against fp64 (the
gated epilogue within tol_f16 at tau = 0, as in tests/test_gpu_gemm_epilogues.py: its activation is not exact); tier B (N(0, 1)
operands, every second case with outlier channels) byte for byte against the same call run alone through rk_debug_gemm_ex, which
is held to tau = 4 E32 against fp64.  DESIGN.md "How the K-split hand-off is tested" says what these tests can and cannot see."""
import numpy as np
import pytest

import _gemm_ref as R
from conftest import load_state

pytestmark = pytest.mark.gpu

BAND_ROWS = 256
NL = 8                                     # launches per chain (T1, T2)
NL_ROWS = 2                                # ... of the 272-tile row-factor cases (T3: 17.8 M outputs per launch, checked word by word)
# backgrounds (rk_debug_gemm_chain: bg): a weight-streaming call of 64 workgroups - a quarter of the CUs - and a 64x64-tile call of
# 128 tiles - half of them; both beside the ping-pong kernel, which owns whole CUs
BG_STREAM = dict(epi=R.EPI_STORE_F32, family=R.STREAM, M=32, N=2048, K=1024, variant=0)
BG_S64 = dict(epi=R.EPI_STORE_F32, family=R.TILED, M=512, N=1024, K=1024, variant=6)
LOADS = [(None, True), (BG_STREAM, True), (BG_S64, False)]           # (background, enqueued in front of the foreground launch)
ACC_CACHE = {}                             # (M, N, K, seed) -> (A [nl, M, K], W, fp64 products as exact fp32): one product per test module


class Options:
    """Engine options for the length of a block, restored to the defaults after it."""
    DEFAULTS = {"gemm_variant": 0, "gemm_sk": 1}

    def __init__(self, eng, **kw):
        self.eng, self.kw = eng, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.eng.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.eng.set_option(k, self.DEFAULTS[k])


@pytest.fixture(scope="module")
def eng(ckpt_dirs):
    from llmrankers._engine import RkEngine
    dims, state = load_state(ckpt_dirs["ckpt_gated_untied"])
    e = RkEngine(dims, device=0, max_tokens=2048, max_seqs=16, max_dec_len=8).load_state(state.items())
    yield e
    e.close()


@pytest.fixture(scope="module")
def llama(ckpt_dirs):
    from llmrankers._engine import RkLlamaEngine
    dims, state = load_state(ckpt_dirs["ckpt_llama"])
    e = RkLlamaEngine(dims, device=0, max_tokens=2048, max_seqs=16).load_state(state.items())
    yield e
    e.close()


def _interior(r, i, m):
    return r["C"][i, r["band"]:r["band"] + m * r["ldc"]].reshape(m, r["ldc"])


def _bands_intact(r, what):
    band = r["band"]
    for i in range(r["C"].shape[0]):
        raw = r["C"][i].view(np.uint8)
        nb = band * r["C"].itemsize
        assert (raw[:nb] == R.SENTINEL).all() and (raw[-nb:] == R.SENTINEL).all(), f"{what}: launch {i} wrote outside its [M, N]"


def _int_problem(m, n, k, nl, seed, big=False):
    """Tier A: nl different integer A_i, one W, and the fp64 products A_i W^T (exact integers below 2^24: kept as fp32)."""
    key = (m, n, k, nl, seed, big)
    if key not in ACC_CACHE:
        rs = np.random.RandomState(seed)
        a = np.stack([(R.int_operands_big if big else R.int_operands)(rs, m, 1, k)[0] for _ in range(nl)])
        w = (R.int_operands_big if big else R.int_operands)(rs, 1, n, k)[1]
        acc = np.stack([R.acc64(a[i], w) for i in range(nl)])
        assert np.abs(acc).max() < 2 ** 24 and (acc == np.rint(acc)).all()
        ACC_CACHE[key] = (a, w, acc.astype(np.float32))
    return ACC_CACHE[key]


# ---- T1: new data on old slabs, idle chip ---------------------------------------------------------------------------------------
T1_SHAPES = [(256, 256, 256),      # the smallest split: one tile, two workgroups
             (1024, 512, 512),
             (2048, 4096, 256),    # 128 tiles: exactly 256 workgroups
             (257, 260, 512)]      # partial tiles


@pytest.mark.parametrize("epi", [R.EPI_RESID_F32, R.EPI_STORE_F32], ids=lambda e: R.EPI_NAMES[e])
@pytest.mark.parametrize("shape", T1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k_split_chain_new_data_on_old_slabs(eng, shape, epi):
    """gemm_sk = 2: eight split launches back to back, every A_i different - a last arriver that read the previous launch's slab
    (or its own) gives other integers.  Bit for bit against fp64."""
    m, n, k = shape
    a, w, acc = _int_problem(m, n, k, NL, 4100 + m)
    rs = np.random.RandomState(4200 + m + epi)
    c_old = rs.randint(-64, 65, size=(NL, m, n), dtype=np.int8).astype(np.float32) if epi == R.EPI_RESID_F32 else None
    with Options(eng, gemm_variant=5, gemm_sk=2):
        r = eng.debug_gemm_chain(epi, a, w, m, n, k, c_in=c_old)
    assert (r["family"], r["variant"], r["ksplit"]) == (R.TILED, 5, 2), r
    _bands_intact(r, f"{shape} {R.EPI_NAMES[epi]}")
    for i in range(NL):
        want = acc[i].astype(np.float64) + (c_old[i] if c_old is not None else 0.0)
        np.testing.assert_array_equal(_interior(r, i, m).astype(np.float64), want, err_msg=f"{shape} {R.EPI_NAMES[epi]} launch {i}")


@pytest.mark.parametrize("shape", T1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k_split_chain_accumulates_into_one_residual_stream(eng, shape):
    """accumulate: all eight launches add into ONE C, as successive layers do: C = C0 + sum_i A_i W^T exactly (every partial an
    integer below 2^24 - asserted in fp64 first)."""
    m, n, k = shape
    a, w, acc = _int_problem(m, n, k, NL, 4100 + m)
    c0 = np.random.RandomState(4300 + m).randint(-64, 65, size=(m, n)).astype(np.float32)
    partial = c0.astype(np.float64) + np.cumsum(acc.astype(np.float64), axis=0)
    assert np.abs(partial).max() < 2 ** 24
    with Options(eng, gemm_variant=5, gemm_sk=2):
        r = eng.debug_gemm_chain(R.EPI_RESID_F32, a, w, m, n, k, c_in=c0, accumulate=True)
    assert r["ksplit"] == 2 and r["C"].shape[0] == 1
    _bands_intact(r, f"{shape} accumulate")
    np.testing.assert_array_equal(_interior(r, 0, m).astype(np.float64), partial[-1], err_msg=f"{shape} accumulate")


@pytest.mark.parametrize("shape", [(2304, 4096, 256),     # 9 x 16 = 144 tiles: twice that is beyond the 256 slabs
                                   (256, 256, 192)],      # three K tiles: one half would keep a single one
                         ids=lambda s: "x".join(map(str, s)))
def test_chain_over_the_split_line_gives_the_unsplit_bits(eng, shape):
    m, n, k = shape
    nl = 2
    rs = np.random.RandomState(4400 + m)
    a = rs.standard_normal((nl, m, k)).astype(np.float16)
    w = rs.standard_normal((n, k)).astype(np.float16)
    with Options(eng, gemm_variant=5, gemm_sk=2):
        r = eng.debug_gemm_chain(R.EPI_STORE_F32, a, w, m, n, k)
    with Options(eng, gemm_variant=5, gemm_sk=0):
        u = eng.debug_gemm_chain(R.EPI_STORE_F32, a, w, m, n, k)
    assert r["ksplit"] == 1 and u["ksplit"] == 1 and r["variant"] == 5
    assert r["C"].tobytes() == u["C"].tobytes()
    _bands_intact(r, f"{shape} unsplit")
    rows = np.unique(np.linspace(0, m - 1, 16).round().astype(int))
    for i in range(nl):
        R.check_f32(_interior(r, i, m)[rows], R.acc64(a[i][rows], w), R.tau(a[i], w), f"{shape} launch {i}")


# ---- T2: the same under load ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((256, 256, 256), R.EPI_RESID_F32, True), ((1024, 512, 512), R.EPI_STORE_F32, False),
                                  ((257, 260, 512), R.EPI_RESID_F32, True)], ids=lambda c: "x".join(map(str, c[0])))
def test_k_split_chain_under_uneven_load_equals_the_call_alone(eng, case):
    """N(0, 1) operands, eight launches, a background grid on part of the chip enqueued in front of or behind each foreground launch
    (both arrival orders of the two splits, both skip_publish outcomes): every launch's output byte-identical to the same call run
    alone, which is held to tau = 4 E32 against fp64; the chain twice: the same bytes."""
    (m, n, k), epi, outliers = case
    rs = np.random.RandomState(4500 + m)
    probs = [R.normal_operands(rs, m, n, k, outliers) for _ in range(NL)]
    w = probs[0][1]
    a = np.stack([p[0] for p in probs])
    c_old = rs.standard_normal((NL, m, n)).astype(np.float32) if epi == R.EPI_RESID_F32 else None
    with Options(eng, gemm_variant=5, gemm_sk=2):
        alone = []
        for i in range(NL):
            o = eng.debug_gemm_ex(epi, R.TILED, a[i], w, m, n, k, c_in=None if c_old is None else c_old[i])
            assert (o["variant"], o["ksplit"]) == (5, 2)
            got = o["C"][o["band"]:o["band"] + m * n].reshape(m, n)
            want = R.acc64(a[i], w) + (c_old[i] if c_old is not None else 0.0)
            R.check_f32(got, want, R.tau(a[i], w), f"{case[0]} alone {i}")
            alone.append(got)
        for bg in (BG_STREAM, BG_S64):
            for bg_first in (True, False):
                what = f"{case[0]} {R.EPI_NAMES[epi]} background {bg['family']}/{bg['variant']} first={bg_first}"
                r = eng.debug_gemm_chain(epi, a, w, m, n, k, c_in=c_old, bg=bg, bg_per_fg=2, bg_first=bg_first)
                r2 = eng.debug_gemm_chain(epi, a, w, m, n, k, c_in=c_old, bg=bg, bg_per_fg=2, bg_first=bg_first)
                assert r["ksplit"] == 2 and not (r["bg_family"] == R.TILED and (r["bg_variant"] == 5 or r["bg_m_pp2"] > 0)), r
                assert r["bg_family"] == bg["family"], r
                _bands_intact(r, what)
                assert r["C"].tobytes() == r2["C"].tobytes(), f"{what}: two runs of the chain differ"
                for i in range(NL):
                    assert _interior(r, i, m).tobytes() == alone[i].tobytes(), f"{what}: launch {i} differs from the call alone"


# ---- T3: row factors under load (the round-4 mechanism at unit size) --------------------------------------------------------------
M3, N3 = 4352, 4096                        # 17 x 16 = 272 tiles on 256 persistent workgroups: 16 of them walk two tiles


@pytest.mark.parametrize("k", [128, 1024])
@pytest.mark.parametrize("epi", [R.EPI_STORE_F16, R.EPI_GEGLU_F16, R.EPI_RELU_F16], ids=lambda e: R.EPI_NAMES[e])
def test_row_factors_with_new_data_per_launch_tier_a(eng, epi, k):
    """gemm_pp2_kernel<.., RS>: the row factors of the folded RMSNorm arrive by four asm loads under the last MFMAs and are waited
    for in front of the next tile's DMA.  A new rowscale_i (powers of two, row 0 saturating) and A_i per launch, idle and beside both
    backgrounds: stale factors or stale rows give other bits.  The idle chain against fp64, the loaded chains against the idle one's bytes."""
    a, w, acc = _int_problem(M3, N3, k, NL_ROWS, 4600 + k, big=True)
    rs = np.random.RandomState(4700 + k)
    rsc = (2.0 ** rs.randint(-3, 4, size=(NL_ROWS, M3))).astype(np.float32)
    rsc[:, 0] = 64.0                                          # 16 K x 64 > 65504
    exp = [R.expected(epi, a[i], w, factor=rsc[i].astype(np.float64), acc=acc[i]) for i in range(NL_ROWS)]
    with Options(eng, gemm_variant=5):
        idle = None
        for bg, bg_first in LOADS:
            what = f"{R.EPI_NAMES[epi]} K={k} background {bg and (bg['family'], bg['variant'])}"
            r = eng.debug_gemm_chain(epi, a, w, M3, N3, k, rowscale=rsc, bg=bg, bg_per_fg=2 if bg else 0, bg_first=bg_first)
            assert (r["family"], r["variant"], r["m_pp2"]) == (R.TILED, 5, 0), r
            _bands_intact(r, what)
            if idle is not None:                                  # beside a background: the idle chain's bytes, which the reference holds
                assert r["C"].tobytes() == idle.tobytes(), f"{what}: differs from the idle chain"
                continue
            idle = r["C"]
            for i in range(NL_ROWS):
                got = _interior(r, i, M3)
                if epi in R.GATED:
                    R.check_f16(got, exp[i]["out"], 0.0, f"{what} launch {i}", lip=exp[i]["lip"], factor=rsc[i])
                else:
                    np.testing.assert_array_equal(got.astype(np.float32), R.f16_sat(exp[i]["out"]).astype(np.float32), err_msg=f"{what} launch {i}")
                    assert (np.abs(got[0].astype(np.float64)) == R.F16_MAX).any(), f"{what}: the saturating row never saturated"


@pytest.mark.parametrize("k", [128, 1024])
@pytest.mark.parametrize("epi", [R.EPI_STORE_F16, R.EPI_GEGLU_F16, R.EPI_RELU_F16], ids=lambda e: R.EPI_NAMES[e])
def test_row_factors_with_new_data_per_launch_tier_b(eng, epi, k):
    """The same with N(0, 1) operands (K = 1024 with outlier channels) and factors in [0.5, 2): every launch byte-identical to the
    same call alone (tests/test_gpu_gemm_epilogues.py holds that call to the fp64 reference at every tile shape; here a sample of
    rows of the alone call is checked again at THIS shape)."""
    rs = np.random.RandomState(4800 + k + epi)
    w = rs.standard_normal((N3, k)).astype(np.float16)
    a = rs.standard_normal((NL_ROWS, M3, k)).astype(np.float32)
    if k == 1024:
        for c in (17, 300, 777):
            a[:, :, c] *= 100.0
    a = a.astype(np.float16)
    rsc = rs.uniform(0.5, 2.0, size=(NL_ROWS, M3)).astype(np.float32)
    rows = np.unique(np.linspace(0, M3 - 1, 16).round().astype(int))
    width = N3 // 2 if epi in R.GATED else N3
    with Options(eng, gemm_variant=5):
        alone = []
        for i in range(NL_ROWS):
            o = eng.debug_gemm_ex(epi, R.TILED, a[i], w, M3, N3, k, rowscale=rsc[i])
            assert o["variant"] == 5
            got = o["C"][o["band"]:o["band"] + M3 * width].reshape(M3, width)
            e = R.expected(epi, a[i][rows], w, factor=rsc[i][rows].astype(np.float64))
            R.check_f16(got[rows], e["out"], R.tau(a[i], w), f"alone {i}", lip=e["lip"], factor=rsc[i][rows])
            alone.append(got)
        for bg, bg_first in LOADS:
            what = f"{R.EPI_NAMES[epi]} K={k} background {bg and (bg['family'], bg['variant'])}"
            r = eng.debug_gemm_chain(epi, a, w, M3, N3, k, rowscale=rsc, bg=bg, bg_per_fg=2 if bg else 0, bg_first=bg_first)
            _bands_intact(r, what)
            for i in range(NL_ROWS):
                assert _interior(r, i, M3).tobytes() == alone[i].tobytes(), f"{what}: launch {i} differs from the call alone"


# ---- T4: the `down` shape, split by option; the default rule never splits -----------------------------------------------------------
def test_down_shape_split_chain_equals_the_calls_alone_and_the_default_rule_never_splits(llama):
    """The defaults (gemm_sk = 1, gemm_variant = 0) on a decoder-only engine plan NO K split: not for a `down`-shaped fp32 residual
    call on the slot stream, not for (700, 516, 14336) - the split would be decided from the launch's tile count, i.e. from the
    batch, and a sequence's bits are promised not to depend on it (choose_ksplit; tests/test_gpu_llama_plan_lines.py).  The
    hand-off at that shape stays covered under gemm_variant = 5, gemm_sk = 2: the ping-pong kernel with ksplit = 2, three launches
    with new data match the alone calls byte for byte."""
    m, n, k, nl = 1536, 4096, 14336, 3
    epi = R.EPI_RESID_F32
    z = np.zeros((1, 8), np.float16)
    small = llama.debug_gemm_chain(epi, z, z, 700, 516, 14336, plan_only=True)
    assert small["ksplit"] == 1 and small["variant"] == 6, small
    plan = llama.debug_gemm_chain(epi, z, z, m, n, k, plan_only=True)
    assert (plan["family"], plan["m_pp2"], plan["ksplit"]) == (R.TILED, 0, 1), plan
    rs = np.random.RandomState(4900)
    w = (rs.randint(-2048, 2049, size=(n, k), dtype=np.int16).astype(np.float32) / 1024.0).astype(np.float16)   # uniform in [-2, 2]
    a = (rs.randint(-2048, 2049, size=(nl, m, k), dtype=np.int16).astype(np.float32) / 1024.0).astype(np.float16)
    c_old = rs.standard_normal((nl, m, n)).astype(np.float32)
    rows = np.unique(np.linspace(0, m - 1, 16).round().astype(int))            # the fp64 check: a sample of rows and columns
    cols = np.unique(np.linspace(0, n - 1, 256).round().astype(int))
    with Options(llama, gemm_variant=5, gemm_sk=2):
        alone = []
        for i in range(nl):
            o = llama.debug_gemm_ex(epi, R.TILED, a[i], w, m, n, k, c_in=c_old[i])
            assert (o["variant"], o["ksplit"]) == (5, 2)
            got = o["C"][o["band"]:o["band"] + m * n].reshape(m, n)
            R.check_f32(got[np.ix_(rows, cols)], R.acc64(a[i][rows], w[cols]) + c_old[i][np.ix_(rows, cols)], R.tau(a[i], w), f"down alone {i}")
            alone.append(got)
        r = llama.debug_gemm_chain(epi, a, w, m, n, k, c_in=c_old)
        assert r["ksplit"] == 2
        _bands_intact(r, "down chain")
        for i in range(nl):
            assert _interior(r, i, m).tobytes() == alone[i].tobytes(), f"down projection: launch {i} differs from the call alone"


# ---- T5: refusals ------------------------------------------------------------------------------------------------------------
def test_chain_refusals_launch_nothing(eng):
    from llmrankers._engine import RkError
    m = n = k = 256
    a = np.ones((2, m, k), np.float16)
    w = np.ones((n, k), np.float16)

    def refused(code, epi=R.EPI_STORE_F32, **kw):
        n_out = 1 if kw.get("accumulate") else 2
        dt = np.float16 if epi in R.F16_EPIS else np.float32
        c_out = np.frombuffer(bytes([R.SENTINEL]) * (n_out * (2 * BAND_ROWS + m) * n * np.dtype(dt).itemsize), dtype=dt).copy()
        with pytest.raises(RkError) as ei:
            eng.debug_gemm_chain(epi, a, w, m, n, k, c_out=c_out, **kw)
        assert ei.value.code == code, (kw, str(ei.value))
        assert (c_out.view(np.uint8) == R.SENTINEL).all(), kw

    with Options(eng, gemm_variant=5, gemm_sk=2):
        refused(-1, n_launch=0)
        refused(-1, n_launch=65)
        refused(-1, bg=dict(epi=R.EPI_STORE_F32, family=R.TILED, M=512, N=512, K=256, variant=5), bg_per_fg=1)
        refused(-1, accumulate=True)                                             # store epilogue
        refused(-1, epi=R.EPI_STORE_F16, accumulate=True)
        refused(-4, epi=R.EPI_STORE_F32, rowscale=np.ones((2, m), np.float32))   # outside the kernels' contract: RK_ERR_STATE, as rk_debug_gemm_ex
        ok = eng.debug_gemm_chain(R.EPI_STORE_F32, a, w, m, n, k)                # (the same call without the fault runs)
    np.testing.assert_array_equal(_interior(ok, 1, m), np.full((m, n), float(k), np.float32))
