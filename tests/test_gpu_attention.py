"""Every attention launch plan of the engine against the fp64 reference of tests/_attn_ref.py, through rk_debug_attn: the call goes
through plan_*attn and that plan's launcher as the engine's own calls do, every output sits between sentinel bands.

Tier S: selector operands - bit for bit (which key, which head, which mask).  Tier R: N(0, 1) operands - within half an fp16 ulp +
C E, E = the error of the documented fp32 arithmetic on a sample of the very problem (never a figure read off a kernel).
Every case: the bands and every row / column the call does not own untouched; a second run gives the same bytes; the plan reported
is the plan the shape should take (Python mirrors of plan_*attn below, constants read from the headers); variants documented as
"same bits" give the same bytes on the random tier.

RATIOS (largest (error - half ulp) / E per plan, tier R) are collected for the record (printed by the last test, quoted in
DESIGN.md); they are not bounds."""
import os
import re

import numpy as np
import pytest

import _attn_ref as A
from conftest import REPO, load_state
from llmrankers._engine import RkError

pytestmark = pytest.mark.gpu

BAND = 8
RATIOS = {}
ERR_INVALID, ERR_HIP, ERR_STATE = -1, -3, -4
_PROBLEMS = {}


def _const(header, name):
    src = open(os.path.join(REPO, "llm-rankers_amd", "csrc", header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


ROW_MAXL, ATTX_MAXK, ATTX_MAXQ = _const("attention.h", "ATT_ROW_MAXL"), _const("attention.h", "ATTX_MAXK"), _const("attention.h", "ATTX_MAXQ")
ATTS_KSTR, XA_MAX_LD, LDC_CHUNK = _const("attention.h", "ATTS_KSTR"), _const("rk_engine.hip", "XA_MAX_LD"), _const("llama_kernels.h", "LDC_CHUNK")
XCDS = 8


@pytest.fixture(scope="module")
def t5(ckpt_dirs):
    from llmrankers._engine import RkEngine
    dims, state = load_state(ckpt_dirs["ckpt_gated_untied"])
    e = RkEngine(dims, device=0, max_tokens=2048, max_seqs=16, max_dec_len=8).load_state(state.items())
    e.n_cu = e.debug_attn(A.ENC, n_seq=1, H=1, seq_off=[0, 1], plan_only=True)["n_cu"]
    yield e
    e.close()


@pytest.fixture(scope="module")
def llama(ckpt_dirs):
    from llmrankers._engine import RkLlamaEngine
    dims, state = load_state(ckpt_dirs["ckpt_llama"])
    e = RkLlamaEngine(dims, device=0, max_tokens=2048, max_seqs=16).load_state(state.items())
    yield e
    e.close()


class Options:
    """Engine options for the length of a block, restored to the defaults after it."""
    DEFAULTS = {"attn_short": 5, "attn_heads_per_wg": 0, "attn_long": 1, "attn_long_nw": 0, "attn_long_xcd": 1, "dec_cross_mfma": 1, "dec_attn_seq": 1,
                "xattn_mfma": 1, "llama_attn_dma": 1, "llama_attn_nw": 0, "llama_dec_r": 0}

    def __init__(self, eng, **kw):
        self.eng, self.kw = eng, kw
        self.now = dict(self.DEFAULTS, **kw)

    def __enter__(self):
        for k, v in self.kw.items():
            self.eng.set_option(k, v)
        return self.now

    def __exit__(self, *exc):
        for k in self.kw:
            self.eng.set_option(k, self.DEFAULTS[k])


def cached(key, build):
    """A problem and its reference are built once, shared by every option variant, and left unchanged."""
    if key not in _PROBLEMS:
        _PROBLEMS[key] = build()
    return _PROBLEMS[key]


# ---- Python mirrors of the few lines of plan_*attn (csrc/rk_engine.hip) ------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _xcd_grid(groups, w):
    return _cdiv(groups, XCDS) * XCDS * w


def mirror_enc(o, n_cu, p):
    lens = np.diff(p.seq_off)
    n_seq, H, maxL, minL = p.n_seq, p.H, int(lens.max()), int(lens.min())
    if maxL <= ROW_MAXL and o["attn_short"]:
        ng = 1 if o["attn_short"] == 6 else 2
        hpw = o["attn_heads_per_wg"] or _cdiv(n_seq * H, n_cu * ng)
        return dict(kind=0, tparam=ng, heads_per_wg=hpw, grid=(_cdiv(n_seq * H, ng * hpw), 1, 1), skip_long=0)
    if o["attn_long"]:
        nw = o["attn_long_nw"] if o["attn_long_nw"] in (3, 6, 12) else 4
        return dict(kind=1, tparam=nw, skip_long=int(minL <= ROW_MAXL), grid=(_xcd_grid(n_seq * H, _cdiv(maxL, 32 * nw)), 1, 1),
                    grid2=(_cdiv(ROW_MAXL, 128), H, n_seq))
    return dict(kind=2, skip_long=0, grid2=(_cdiv(maxL, 128), H, n_seq))


def seq_lds(keys):
    kp = (keys + 3) & ~3
    return kp * ATTS_KSTR * 2 + kp * 64 * 2 + A.LUT_N * 4 + 12 + 4 * (64 * 4 + kp * 4) * 4


def row_lds(keys):
    return (64 + 256 + 8 + keys) * 4


def mirror_dec(o, p):
    H, Ld = p.H, p.Ld
    if p.tree_pos is not None:
        return dict(mfma=0, staged=2, grid2=(1, H, len(p.tree_pos)), lds=row_lds(Ld))
    keys = int(np.diff(p.seq_off).max()) if p.cross else Ld
    mf = bool(o["dec_cross_mfma"]) and Ld <= ATTX_MAXQ
    mfma = (mf and Ld >= 2) if p.cross else (mf and Ld > XA_MAX_LD)
    if mfma and keys <= ATTX_MAXK:
        return dict(mfma=1, staged=0, grid=(H, p.n_seq, 1))
    if o["dec_attn_seq"] and Ld >= 2 and seq_lds(keys) <= 160 * 1024:
        return dict(mfma=int(mfma), staged=1, grid2=(H, p.n_seq, 1), lds=seq_lds(keys))
    return dict(mfma=int(mfma), staged=2, grid2=(Ld, H, p.n_seq), lds=row_lds(keys))


def mirror_xattn(o, n_cu, p):
    nch = _cdiv(int(np.diff(p.seq_off).max()), 64)
    wgs16 = nch * p.M * _cdiv(p.H, 16)
    if o["xattn_mfma"] and p.d % 256 == 0:
        part = 0 if wgs16 <= 2 * n_cu else 1
    else:
        part = 2 if wgs16 >= 2 * n_cu else 3
    return dict(part=part, nch=nch, grid=(nch, p.M, _cdiv(p.H, 4 if part == 3 else 16)), grid2=(p.H, p.M, 1), tparam=4 if part == 3 else 16)


def mirror_llama(o, p):
    maxL = int(np.diff(p.seq_off).max())
    if not o["llama_attn_dma"]:
        return dict(kind=0, grid=(_cdiv(maxL, 128), p.H, p.n_seq))
    nw = 8 if o["llama_attn_nw"] == 8 else 4
    return dict(kind=1, tparam=nw, grid=(_xcd_grid(p.n_seq * p.n_kv, (p.H // p.n_kv) * _cdiv(maxL, 32 * nw)), 1, 1))


def mirror_step(o, p):
    G = p.H // p.n_kv
    R = 8 if G % 8 == 0 else 4 if G % 4 == 0 else 2 if G % 2 == 0 else 1
    if o["llama_dec_r"] == 1:
        R = 1
    if o["llama_dec_r"] == 2 and G == 7:
        R = 7
    nch = _cdiv(p.P, LDC_CHUNK)
    return dict(R=R, nch=nch, tparam=R, grid=(nch, p.H // R, p.n_seq), grid2=(p.H, p.n_seq, 1))


# ---- one call, both runs, every assertion ------------------------------------------------------------------------------------
def call_args(p):
    kw = dict(n_seq=p.n_seq, H=p.H, q=p.q, out=p.out, kv=p.kv, band_rows=p.band, n_kv=p.n_kv, Ld=p.Ld, cross=p.cross, M=p.M, row0=p.row0, d=p.d, P=p.P,
              ldq=p.ldq, ldkv=p.ldkv, ldctx=p.ldctx, k_col=p.k_col, v_col=p.v_col, seq_off=p.seq_off, row_off=p.row_off, tree_keys=p.tree_keys,
              tree_pos=p.tree_pos, row_seq=p.row_seq, pos=p.pos, bias_lut=p.lut, cos=p.cos, sin=p.sin, qkv_bias=p.qkv_bias, cache=p.cache)
    return kw


def _all_sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == A.SENTINEL).all())


def run_case(eng, p, mirror, name, what):
    """Runs the problem under the options in force: plan == mirror, bands intact, second run the same bytes, the interior judged
    against fp64 (rows and columns outside the call included).  Returns the interior (and the cache's) bytes."""
    kw = call_args(p)
    plan = eng.debug_attn(p.kind, plan_only=True, **kw)
    for k, v in mirror.items():
        assert plan[k] == v, f"{what}: plan field {k} = {plan[k]}, the shape should take {v} (plan {plan})"
    try:
        r1 = eng.debug_attn(p.kind, **kw)
        r2 = eng.debug_attn(p.kind, **kw)
    except RkError as err:
        if err.code == ERR_HIP:                  # a fault on the device: nothing more is started on it from this module
            pytest.exit(f"{what}: {err}", returncode=3)
        raise
    out = r1["out"]
    assert out.tobytes() == r2["out"].tobytes(), f"{what}: a second run gives other bytes"
    assert _all_sentinel(out[:p.band]) and _all_sentinel(out[-p.band:]), f"{what}: a guard band of the output was written"
    inner = out[p.band:-p.band]
    if p.kind == A.DEC:                       # which pieces round their probabilities to fp16: the matrix-core kernel's
        p.p16 = (lambda nk: nk <= ATTX_MAXK) if (plan["mfma"] and p.cross) else bool(plan["mfma"])
    for fmt, r in A.judge(p, inner, what=what).items():
        RATIOS[name + (" fp16 P" if fmt else " fp32 P")] = max(RATIOS.get(name + (" fp16 P" if fmt else " fp32 P"), 0.0), r)
        print(f"{what}: ratio {r:.2f}")
    extra = b""
    if p.kind == A.STEP:
        c1, cb = r1["cache"], p.band * 128
        assert c1.tobytes() == r2["cache"].tobytes(), f"{what}: a second run leaves another cache"
        assert _all_sentinel(c1[:cb]) and _all_sentinel(c1[-cb:]), f"{what}: a guard band of the cache was written"
        A.judge_cache(p, c1[cb:-cb], what)
        extra = c1.tobytes()
    return inner.tobytes() + extra


def same_bits(results, what):
    first = next(iter(results))
    for k, v in results.items():
        assert v == results[first], f"{what}: {k} and {first} are documented as the same bits and differ"


# ---- T5 encoder --------------------------------------------------------------------------------------------------------------
SHORT = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192]
ENC_BATCHES = {"all13": SHORT, "one": [192], "three": [33, 1, 128], "five": [65, 2, 191, 64, 31]}
ENC_LONG = [193, 255, 256, 257, 384, 385, 513, 641, 900]
ENC_TIERS = {"S": dict(tier="S"), "spike": dict(tier="S", spike=[5, -7, 128, -128, 1, -1]), "R": dict(tier="R"), "Rflat": dict(tier="R", flat=True)}
ENC_KERNEL = ["attn_enc_dma", "attn_enc_long", "attn_enc tiled"]


def _enc(seed, H, lens, tname, pad):
    return cached(("enc", seed, H, tuple(lens), tname, pad), lambda: A.build_enc(seed, H, lens, band=BAND, pad=pad, **ENC_TIERS[tname]))


@pytest.mark.parametrize("H", [3, 6])
@pytest.mark.parametrize("batch", sorted(ENC_BATCHES))
def test_encoder_short(t5, H, batch):
    lens = ENC_BATCHES[batch]
    for n, tname in enumerate(ENC_TIERS):
        p = _enc(100 + n, H, lens, tname, (64, 8) if n % 2 else (0, 0))
        bits = {}
        for short, hpw in ((5, 0), (6, 0), (5, 1), (6, 3), (0, 0)):
            with Options(t5, attn_short=short, attn_heads_per_wg=hpw) as o:
                m = mirror_enc(o, t5.n_cu, p)
                bits[(short, hpw)] = run_case(t5, p, m, ENC_KERNEL[m["kind"]], f"encoder H={H} {batch} {tname} attn_short={short} hpw={hpw}")
        same_bits(bits, f"encoder H={H} {batch} {tname}")


@pytest.mark.parametrize("long", ENC_LONG)
def test_encoder_long(t5, long):
    i = ENC_LONG.index(long)
    H = 3 if i % 2 else 6
    lens = [long] if i % 4 == 3 else [33, long, 1, 192][:2 + i % 3]        # with and without short companions (skip_long)
    for n, tname in enumerate(("S", "R", "spike") if i % 2 == 0 else ("S", "Rflat")):
        p = _enc(200 + 10 * i + n, H, lens, tname, (8, 64) if n == 1 else (0, 0))
        bits = {}
        for nw in (0, 3, 6, 12):
            for xcd in (1, 0):
                with Options(t5, attn_long_nw=nw, attn_long_xcd=xcd) as o:
                    m = mirror_enc(o, t5.n_cu, p)
                    assert m["kind"] == 1 and m["skip_long"] == int(min(lens) <= ROW_MAXL)
                    bits[(nw, xcd)] = run_case(t5, p, m, ENC_KERNEL[1], f"encoder long {lens} H={H} {tname} nw={nw} xcd={xcd}")
        same_bits(bits, f"encoder long {lens} H={H} {tname}")
        with Options(t5, attn_long=0) as o:                                # the tiled kernel for every length
            m = mirror_enc(o, t5.n_cu, p)
            assert m["kind"] == 2
            run_case(t5, p, m, ENC_KERNEL[2], f"encoder long {lens} H={H} {tname} attn_long=0")


# ---- T5 decoder --------------------------------------------------------------------------------------------------------------
DEC_LD = [1, 2, 4, 5, 16, 17, 33, 64, 65]
DEC_KERNEL = {(1, 0): "attn_dec_cross_mfma", (0, 1): "attn_dec_seq", (0, 2): "attn_dec (row)", (1, 1): "attn_dec_cross_mfma + seq", (1, 2): "attn_dec_cross_mfma + row"}
TREE_SMALL = ([[0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 2, 0], [0, 1, 3, 0], [0, 4, 0, 0], [0, 1, 2, 5]], [0, 1, 2, 2, 1, 3])


def _dec_variants(eng, p, what):
    bits = {}
    for mf in (1, 0):
        for seq in (1, 0):
            with Options(eng, dec_cross_mfma=mf, dec_attn_seq=seq) as o:
                m = mirror_dec(o, p)
                bits[(mf, seq)] = (m["mfma"], run_case(eng, p, m, DEC_KERNEL[(m["mfma"], m["staged"])], f"{what} mfma={mf} seq={seq}"))
    # SEQ and ROW are the same bits wherever the same kernel class (matrix-core or staged) takes the sequences
    for mf in (1, 0):
        assert bits[(mf, 1)][1] == bits[(mf, 0)][1], f"{what}: dec_attn_seq 1 and 0 are documented as the same bits and differ (dec_cross_mfma={mf})"


def seq_row_edge(eng):
    """Largest key count the staged (head, sequence) kernel takes, from the plan (its LDS formula against 160 KiB), not a number."""
    lo, hi = ATTX_MAXK + 1, 2048
    q = lambda keys: eng.debug_attn(A.DEC, n_seq=1, H=1, Ld=2, cross=True, seq_off=[0, keys], plan_only=True)["staged"]
    assert q(lo) == 1 and q(hi) == 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if q(mid) == 1 else (lo, mid)
    assert seq_lds(lo) <= 160 * 1024 < seq_lds(hi)
    return lo


@pytest.mark.parametrize("Ld", DEC_LD)
def test_decoder_self(t5, Ld):
    H = 6 if Ld in (4, 33) else 3
    tiers = [("S", dict(tier="S")), ("spike", dict(tier="S", spike=[0, -1, -(Ld - 1), -(Ld // 2), -2, -3])), ("R", dict(tier="R")), ("Rflat", dict(tier="R", flat=True)),
             ("Snolut", dict(tier="S", with_lut=False))]
    for n, (tname, kw) in enumerate(tiers):
        p = cached(("dec", Ld, tname), lambda: A.build_dec(300 + n, H, Ld=Ld, n_seq=3, band=BAND, pad=(8, 64) if n % 2 else (0, 0), **kw))
        _dec_variants(t5, p, f"decoder self Ld={Ld} H={H} {tname}")


def test_decoder_self_clamp(t5):
    """More than 128 positions: the clamp entry of the table, with exactly one key that far away."""
    p = cached(("dec", "clamp"), lambda: A.build_dec(390, 3, "S", Ld=130, n_seq=2, band=BAND, spike=[-128, -1, -127]))
    _dec_variants(t5, p, "decoder self Ld=130 spike at the clamp")


@pytest.mark.parametrize("Ld", DEC_LD)
def test_decoder_cross(t5, Ld):
    edge = seq_row_edge(t5)
    mixes = {"seq": [1, 63, 64, 65, 191, 192, 193, 300], "seq_edge": [192, 1, edge - 1, 193, edge, 64], "row_edge": [65, edge + 1, 191, 193, edge]}
    H = 6 if Ld in (2, 64) else 3
    for n, (mname, keys) in enumerate(mixes.items()):
        for tname in ("S", "R") if n == 0 else (("S",) if n == 1 else ("R",)):
            p = cached(("decx", Ld, mname, tname), lambda: A.build_dec(400 + n, H, tname, Ld=Ld, n_seq=len(keys), key_lens=keys, band=BAND,
                                                                      pad=(64, 8) if n else (0, 0), ldkv_pad=8 * n))
            _dec_variants(t5, p, f"decoder cross Ld={Ld} H={H} keys {mname} {tname}")


@pytest.mark.parametrize("rows", [(2, 4, 3, 2), (5, 16, 9), (17, 64, 33, 18), (65, 70)])
def test_decoder_ragged(t5, rows):
    """Row counts that share a class key (dec_len_class): one pass, every sequence its own count."""
    for n, tname in enumerate(("S", "R")):
        p = cached(("decrag", rows, tname), lambda: A.build_dec(500 + n, 3, tname, rows=list(rows), band=max(BAND, max(rows)), spare=4))
        _dec_variants(t5, p, f"decoder ragged self {rows} {tname}")
        keys = [64, 193, 1, 300][:len(rows)]
        p = cached(("decragx", rows, tname), lambda: A.build_dec(510 + n, 3, tname, rows=list(rows), key_lens=keys, band=BAND, spare=4))
        _dec_variants(t5, p, f"decoder ragged cross {rows} {tname}")


def _big_tree():
    """A 5-row shared prefix, then 6 branches of depth 1 to 3 (rk_t5_greedy2's shape): rows 0-4 the prefix, each branch its own rows."""
    Ld, keys, pos = 8, [], []
    for r in range(5):
        keys.append(list(range(r + 1)) + [0] * (Ld - r - 1))
        pos.append(r)
    row = 5
    for br in range(6):
        chain = [0, 1, 2, 3, 4]
        for dpt in range(1 + br % 3):
            chain = chain + [row]
            keys.append(chain + [0] * (Ld - len(chain)))
            pos.append(len(chain) - 1)
            row += 1
    return keys, pos


@pytest.mark.parametrize("tree", ["small", "big"])
def test_decoder_tree(t5, tree):
    tk = TREE_SMALL if tree == "small" else _big_tree()
    for n, tname in enumerate(("S", "R")):
        p = cached(("dectree", tree, tname), lambda: A.build_dec(520 + n, 3, tname, tree=tk, band=BAND))
        m = mirror_dec(Options.DEFAULTS, p)
        run_case(t5, p, m, "attn_dec (tree)", f"decoder tree {tree} {tname}")


# ---- query-side cross-attention ----------------------------------------------------------------------------------------------
XA_LENS = [1, 63, 64, 65, 128, 129, 200]
XA_KERNEL = ["xattn_part_mfma<few>", "xattn_part_mfma", "xattn_part<16>", "xattn_part<4>"]


@pytest.mark.parametrize("M,Ld,H,d", [(1, 1, 6, 256), (13, 1, 6, 256), (13, 1, 16, 256), (33, 1, 6, 256), (33, 4, 6, 256), (320, 1, 6, 256), (320, 4, 16, 256),
                                      (13, 4, 6, 160), (320, 1, 6, 160)])
def test_query_side(t5, M, Ld, H, d):
    n_seq = _cdiv(M + 3, Ld)
    lens = [XA_LENS[(3 * b + M) % len(XA_LENS)] for b in range(n_seq)]
    seen = set()
    for n, (tname, row0, rs) in enumerate((("S", 0, False), ("R", 3, False), ("S", 2, True), ("Rflat", 0, True))):
        if M == 320 and H == 16 and n >= 2:
            continue
        row_seq = [(7 * r) % n_seq for r in range(M + row0)] if rs else None
        p = cached(("xa", M, Ld, H, d, n), lambda: A.build_xattn(600 + n, H, d, M, Ld, lens, tname[:1], row0=row0, row_seq=row_seq, band=BAND,
                                                                flat=tname == "Rflat"))
        for mf in (1, 0):
            with Options(t5, xattn_mfma=mf) as o:
                m = mirror_xattn(o, t5.n_cu, p)
                seen.add(m["part"])
                run_case(t5, p, m, XA_KERNEL[m["part"]], f"query-side M={M} Ld={Ld} H={H} d={d} {tname} row0={row0} row_seq={rs} xattn_mfma={mf}")
    if d % 256:
        assert seen <= {2, 3}, "a width the matrix-core form does not take went to it"


def test_query_side_both_sides_of_the_few_line(t5):
    """MFMA_FEW / MFMA and VALU4 / VALU16 are chosen by the workgroup count against the CU count: both sides, from the plan."""
    seen = set()
    for M in (1, 13, 33, 320):
        for mf in (1, 0):
            with Options(t5, xattn_mfma=mf):
                seen.add(t5.debug_attn(A.XATTN, n_seq=M, H=6, M=M, Ld=1, d=256, ldq=6 * 256, ldkv=256, ldctx=6 * 256,
                                       seq_off=np.arange(M + 1) * 200, plan_only=True)["part"])
    assert seen == {0, 1, 2, 3}


# ---- Llama -------------------------------------------------------------------------------------------------------------------
LLAMA_CASES = {(4, 4): [1, 63, 64, 65, 700], (8, 2): [127, 128, 129, 257], (28, 4): [1, 64, 129, 257]}


@pytest.mark.parametrize("heads", sorted(LLAMA_CASES))
def test_llama_prefill(llama, heads):
    H, n_kv = heads
    for n, tname in enumerate(("S", "R", "Rpeaked")):                      # Rpeaked: queries x 4, scores as peaked as a trained model's
        p = cached(("llama", heads, tname), lambda: A.build_llama(700 + n, H, n_kv, LLAMA_CASES[heads], tname[:1], band=BAND, pad=(8, 64) if n else (0, 0),
                                                                 qscale=4.0 if n == 2 else 1.0))
        bits = {}
        for dma in (1, 0):
            for nw in (0, 8):
                with Options(llama, llama_attn_dma=dma, llama_attn_nw=nw) as o:
                    m = mirror_llama(o, p)
                    bits[(dma, nw)] = run_case(llama, p, m, "attn_causal128_dma" if dma else "attn_causal128", f"llama prefill {heads} {tname} dma={dma} nw={nw}")
        assert bits[(1, 0)] == bits[(1, 8)], f"llama prefill {heads} {tname}: llama_attn_nw 4 and 8 are documented as the same bits and differ"
        assert bits[(0, 0)] == bits[(0, 8)]


STEP_POS = [0, 1, 127, 128, 129, 255, 256, 300]


@pytest.mark.parametrize("heads", [(8, 1), (8, 2), (4, 2), (4, 4), (28, 4)])      # G = 8, 4, 2, 1, 7
@pytest.mark.parametrize("bias", [False, True])
def test_llama_step(llama, heads, bias):
    H, n_kv = heads
    pos = {(8, 1): [300], (8, 2): [0, 1, 127], (4, 2): [128, 129, 255, 256, 300], (4, 4): [1, 128], (28, 4): STEP_POS}[heads]
    pos = pos[::-1] if bias else pos
    P = max(STEP_POS) + 4
    for n, tname in enumerate(("S", "R")):
        p = cached(("step", heads, bias, tname), lambda: A.build_step(800 + n, H, n_kv, pos, P, tname, bias=bias, band=BAND))
        bits = {}
        for r in (0, 1, 2):
            with Options(llama, llama_dec_r=r) as o:
                m = mirror_step(o, p)
                bits[r] = run_case(llama, p, m, f"attn_dec_cached<128, {m['R']}>" + ("+bias" if bias else ""), f"llama step {heads} bias={bias} {tname} rows={len(pos)} llama_dec_r={r}")
        same_bits(bits, f"llama step {heads} bias={bias} {tname}")


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(t5, llama):
    """A call outside what a plan's kernels take, or beyond the buffers given, stops with an error status before anything is launched."""
    enc = cached(("enc", 100, 3, tuple(ENC_BATCHES["three"]), "S", (0, 0)), lambda: A.build_enc(100, 3, ENC_BATCHES["three"], "S", band=BAND))
    ll = cached(("llama", (8, 2), "S"), lambda: A.build_llama(700, 8, 2, LLAMA_CASES[(8, 2)], "S", band=BAND))

    def refused(eng, kind, code, **change):
        p = enc if kind == A.ENC else ll
        kw = dict(call_args(p), **change)
        with pytest.raises(RkError) as ei:
            eng.debug_attn(kind, **kw)
        assert ei.value.code == code, f"{change}: status {ei.value.code}, expected {code}"

    refused(llama, A.ENC, ERR_STATE)                                        # the wrong family, both ways
    refused(t5, A.LLAMA, ERR_STATE)
    refused(t5, A.ENC, ERR_INVALID, ldq=enc.ldq - 8, q=enc.q[:, :-8])       # rows narrower than q | k | v
    refused(t5, A.ENC, ERR_INVALID, q=enc.q[:-1])                           # one row short
    refused(t5, A.ENC, ERR_INVALID, out=enc.out[:-1])
    refused(t5, A.ENC, ERR_INVALID, seq_off=[0, 33, 33, 162])               # an empty sequence
    refused(llama, A.LLAMA, ERR_INVALID, n_kv=3)                            # kv heads that do not divide the heads
    # the per-row kernel's LDS is opted in for the engine's capacity: more keys than that is not a call the engine could make
    with pytest.raises(RkError) as ei:
        t5.debug_attn(A.DEC, n_seq=1, H=1, Ld=1, cross=True, seq_off=[0, 4096], plan_only=True)
    assert ei.value.code == ERR_STATE
    with pytest.raises(RkError) as ei:                                      # a width the score loop's 32-column steps do not divide
        t5.debug_attn(A.XATTN, n_seq=1, H=6, M=1, Ld=1, d=100, ldq=600, ldkv=100, ldctx=600, seq_off=[0, 5], plan_only=True)
    assert ei.value.code == ERR_INVALID


def test_zz_report_ratios():
    """For the record: the largest (error - half ulp) / E per plan on the random tier.  Not a bound."""
    for k in sorted(RATIOS):
        print(f"ATTN_RATIO {k}: {RATIOS[k]:.2f}")
