"""The attention reference can fail (no GPU): numpy mutants of the documented arithmetic, each breaking ONE rule of tests/_attn_ref.py
- an addressing rule of items() or a step of the emulation - run on fixtures from the builders the GPU test uses, and each must be rejected by tier
S (bit for bit) or tier R (half an fp16 ulp + C E); the honest emulation in every order a kernel uses must be accepted.  A mutant
that passes means the fixtures or the tolerance are too weak: fix those, never the list."""
import numpy as np
import pytest

import _attn_ref as A

TREE = ([[0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 2, 0], [0, 1, 3, 0], [0, 4, 0, 0], [0, 1, 2, 5]], [0, 1, 2, 2, 1, 3])
_FIX = {}


def fixtures():
    """name -> problem, built once and left unchanged."""
    if not _FIX:
        _FIX.update({
            "enc_S": A.build_enc(1, 3, [1, 2, 33, 65, 129, 192], "S", pad=(64, 64)),
            "enc_spike": A.build_enc(2, 3, [129, 64, 5], "S", spike=[5, -7, 128]),
            "enc_R": A.build_enc(3, 3, [1, 33, 65, 150], "R"),
            "enc_Rflat": A.build_enc(4, 3, [2, 64, 129], "R", flat=True),
            "dec_S": A.build_dec(5, 3, "S", Ld=17, n_seq=3),
            "dec_spike": A.build_dec(6, 3, "S", Ld=33, n_seq=2, spike=[0, -3, -20]),
            "dec_clamp": A.build_dec(7, 3, "S", Ld=130, n_seq=1, spike=[-128, -1, -127]),
            "dec_ragged_S": A.build_dec(8, 3, "S", rows=[2, 4, 3], spare=4),
            "dec_tree_S": A.build_dec(9, 3, "S", tree=TREE),
            "dec_cross_S": A.build_dec(10, 3, "S", Ld=5, n_seq=3, key_lens=[1, 64, 193]),
            "dec_R": A.build_dec(11, 3, "R", Ld=65, n_seq=2),
            "dec_ragged_R": A.build_dec(12, 3, "R", rows=[2, 4, 3], spare=4),
            "dec_tree_R": A.build_dec(13, 3, "R", tree=TREE),
            "dec_cross_R": A.build_dec(14, 3, "R", Ld=5, n_seq=3, key_lens=[1, 64, 193]),
            "xattn_S": A.build_xattn(15, 6, 256, 13, 1, [1, 63, 64, 65, 128, 129, 200] * 2, "S"),
            "xattn_R": A.build_xattn(16, 6, 256, 13, 1, [1, 63, 64, 65, 128, 129, 200] * 2, "R"),
            "llama_S": A.build_llama(17, 8, 2, [1, 63, 129], "S"),
            "llama_R": A.build_llama(18, 8, 2, [1, 63, 129], "R"),
            "llama_Rpeaked": A.build_llama(21, 8, 2, [1, 63, 129], "R", qscale=4.0),
            "step_S": A.build_step(19, 8, 2, [0, 1, 127, 128, 300], 304, "S", bias=True),
            "step_R": A.build_step(20, 8, 2, [0, 1, 127, 128, 300], 304, "R", bias=True),
        })
    return _FIX


ORDERS = [("chain", 64), ("online", 64), ("online", 128), ("flash", 64), ("flash", 128), ("tree4", 64)]
# mutant -> the fixtures of every kind it applies to; at least one of each group must reject it
MUTANTS = {
    "drop_last": [["enc_S", "enc_R"], ["dec_S", "dec_R"], ["dec_cross_S", "dec_cross_R"], ["xattn_S", "xattn_R"], ["llama_S", "llama_R"], ["step_S", "step_R"]],
    "next_seq": [["enc_S"], ["dec_S"], ["dec_cross_S"], ["xattn_S"], ["llama_S"], ["step_S"]],
    "causal_plus1": [["dec_S"], ["llama_S"], ["step_S"]],
    "bias_head": [["enc_spike", "enc_R"], ["dec_spike", "dec_R"]],
    "bias_sign": [["enc_spike", "enc_R"], ["dec_spike", "dec_R"]],
    "clamp127": [["enc_spike"], ["dec_clamp"]],
    "kv_mod": [["llama_S", "llama_R"], ["step_S", "step_R"]],
    "scale_nohd": [["llama_R"], ["step_R"]],
    # exp(s) rounded to fp16 as it is: visible where scores leave fp16's exponent range, as unscaled T5's and a trained Llama's do
    # (N(0, 1) rows under the 128**-0.5 scale give scores of N(0, 1): there the mutant IS the honest arithmetic)
    "p16_before_max": [["enc_R"], ["dec_R"], ["dec_cross_R"], ["xattn_R"], ["llama_Rpeaked"]],
    "merge_no_rescale": [["enc_R"], ["dec_cross_R"], ["xattn_R"], ["llama_R"], ["step_R"]],
    "ragged_longest": [["dec_ragged_S", "dec_ragged_R"]],
    "tree_neighbour": [["dec_tree_S", "dec_tree_R"]],
}


def _rejects(p, got, what):
    try:
        A.judge(p, got, what=what)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_is_rejected(mut):
    fx = fixtures()
    for group in MUTANTS[mut]:
        order = "flash" if mut == "merge_no_rescale" else "chain"
        hit = [name for name in group if _rejects(fx[name], A.emulated(fx[name], order, 64, mut=mut), f"{mut} on {name}")]
        assert hit, f"mutant {mut} passes on {group}: the fixtures or the tolerance are too weak"


def test_selector_mutants_fail_bit_for_bit():
    """The addressing mutants are caught by tier S alone, whatever the tolerance: one admitted trap row, one dropped winner."""
    fx = fixtures()
    for mut, names in (("drop_last", ["enc_S", "dec_S", "dec_cross_S", "xattn_S", "llama_S", "step_S"]), ("next_seq", ["enc_S", "dec_S", "dec_cross_S", "xattn_S", "llama_S", "step_S"]),
                       ("causal_plus1", ["dec_S", "llama_S", "step_S"]), ("kv_mod", ["llama_S", "step_S"]), ("ragged_longest", ["dec_ragged_S"]),
                       ("tree_neighbour", ["dec_tree_S"]), ("bias_head", ["enc_spike", "dec_spike"]), ("bias_sign", ["enc_spike", "dec_spike"]),
                       ("clamp127", ["enc_spike", "dec_clamp"])):
        for name in names:
            assert _rejects(fx[name], A.emulated(fx[name], mut=mut), f"{mut} on {name}"), f"tier S misses {mut} on {name}"


def test_honest_orders_pass():
    """Every fixture, every order, both probability formats: accepted, and the largest (error - half ulp) / E stays below C.  Prints
    the table quoted in the docstring of _attn_ref.py."""
    fx = fixtures()
    table = {}
    for name, p in fx.items():
        formats = [p.p16] if p.tier == "S" else [True, False]
        keep = p.p16
        try:
            for fmt in formats:
                p.p16 = fmt
                for order, tile in ORDERS:
                    r = A.judge(p, A.emulated(p, order, tile), what=f"{name} {order} {tile} p16={fmt}")
                    for k, v in r.items():
                        table[(order, tile, k)] = max(table.get((order, tile, k), 0.0), v)
        finally:
            p.p16 = keep
    for key in sorted(table):
        print("order %-6s tile %3d  p16 %-5s  ratio %.2f" % (*key, table[key]))
        assert table[key] <= A.C
    assert max(v for (o, _, _), v in table.items() if o != "chain") > 0.5, "the re-orderings do not differ from the chain: nothing was measured"


def test_selector_fixtures_carry_their_traps():
    """Every selector fixture has forbidden rows that hold a winner's copy (a builder that placed none would test no mask)."""
    for name, p in fixtures().items():
        if p.tier == "S" and p.exact is None:
            assert p.n_traps >= p.H if p.kind != A.LLAMA and p.kind != A.STEP else p.n_traps >= p.n_kv, f"{name}: {p.n_traps} traps"


def test_step_cache_rule():
    """The cache after a step: the honest rows pass; a value written one position late, or a neighbour row touched, does not."""
    fx = fixtures()
    for name in ("step_S", "step_R"):
        p = fx[name]
        good = A.expected_cache(p, emul=True).astype(np.float16)
        A.judge_cache(p, good, name)
        kc, _ = A.step_cache_views(p, good.copy())
        late = good.copy()
        kl, _ = A.step_cache_views(p, late)
        t = int(p.pos[1])
        kl[1, 0, t + 1], kl[1, 0, t] = kc[1, 0, t], A.step_cache_views(p, p.cache)[0][1, 0, t]
        with pytest.raises(AssertionError):
            A.judge_cache(p, late, name)


def test_builder_refuses_a_thin_margin():
    """The margin is asserted, never redrawn: +-4 rows at d = 128 under the Llama scale do not reach 128 and the builder says so."""
    rs = np.random.RandomState(0)
    queries = [(range(0, i + 1), []) for i in range(700)]
    with pytest.raises(AssertionError, match="margin"):
        A.selector(rs, 700, 128, 4, queries, [], scale=128.0 ** -0.5, what="thin")


# ---- the decoder's query-side chain (rk_debug_xattn_chain; _attn_ref.py: build_chain / judge_chain) -----------------------------
CHAIN_LENS = [1, 63, 64, 65, 129, 200, 7, 64, 128, 130, 1, 33, 70]
TREE_SEQ = [0, 0, 0, 2, 1, 1, 0, 2, 2, 1, 0, 1, 2, 0, 1, 2]        # row_seq of the tree form: row -> sequence, not row // Ld
_CHAIN = {}


def chain_fixtures():
    """name -> chain problem: 13 rows at one position (every norm form, both paths of the block sum), and 9 rows of a 4-position call
    starting at row 3, with and without row_seq."""
    if not _CHAIN:
        for tier in "SR":
            for norm, nb in (("none", 0), ("rowscale", 0), ("ssq", 5), ("ssq", 8)):
                _CHAIN[f"{tier}_{norm}{nb or ''}"] = A.build_chain(30, 13, 1, 2, 128, CHAIN_LENS, tier, norm=norm, nb=nb, ldo_pad=8)
            _CHAIN[f"{tier}_row0"] = A.build_chain(31, 9, 4, 2, 128, [130, 64, 5], tier, norm="rowscale", row0=3)
            _CHAIN[f"{tier}_tree"] = A.build_chain(32, 9, 4, 2, 128, [130, 64, 5], tier, norm="ssq", nb=4, row0=3, row_seq=TREE_SEQ)
        _CHAIN["R_chunks"] = A.build_chain(34, 6, 1, 2, 128, [1450, 1, 4100, 700, 64], "R", norm="rowscale", row_seq=[0, 1, 2, 3, 4, 2])   # 23 and 65 chunks
        _CHAIN["R_wide"] = A.build_chain(33, 5, 1, 6, 512, [300, 64, 1, 129, 65], "R", norm="ssq", nb=16)    # K = 512: the orders differ more
    return _CHAIN


CHAIN_ORDERS = [("chain", "fma", True), ("eighths", "fma", True), ("eighths", 4, True), ("eighths", 16, True), ("inter16", "fma", False), ("inter16", 4, False)]
# mutant -> fixtures that must reject it (at least one of each group); "R:" groups must do so on the random tier alone
CHAIN_MUTANTS = {
    "wq_head": [["S_rowscale"], ["R_rowscale"]],
    "wk_untransposed": [["S_rowscale"], ["R_rowscale"]],
    "no_factor": [["S_rowscale"], ["S_ssq5"], ["R_rowscale"], ["R_ssq8"]],
    "factor_next_row": [["S_rowscale"], ["S_ssq5"], ["R_rowscale"]],
    "factor_after_round": [["R_rowscale"], ["R_ssq5"]],
    "ssq_nb_minus1": [["S_ssq5"], ["R_ssq5"], ["R_ssq8"]],
    "no_eps": [["R_ssq5"], ["R_ssq8"]],
    "seq_ignores_row0": [["S_row0"], ["S_tree"], ["R_row0"]],
    "row_seq_ignored": [["S_tree"], ["R_tree"]],
    "merge_call_nch": [["S_rowscale"], ["R_rowscale"]],
    "merge_no_rescale": [["R_rowscale"], ["R_wide"]],
    "wv_head": [["S_rowscale"], ["R_rowscale"]],
    "ctx_slab_later": [["S_rowscale"], ["R_rowscale"]],
    "no_inner_round": [["R_rowscale"], ["R_wide"]],
}


def _chain_rejects(p, res, what):
    try:
        A.judge_chain(p, res, what=what)
    except AssertionError as err:
        return str(err)
    return ""


@pytest.mark.parametrize("mut", sorted(CHAIN_MUTANTS))
def test_chain_mutant_is_rejected(mut):
    fx = chain_fixtures()
    for group in CHAIN_MUTANTS[mut]:
        why = [_chain_rejects(fx[n], A.emulated_chain(fx[n], mut=mut), f"{mut} on {n}") for n in group]
        print(mut, group, [w[:200] for w in why])
        assert any(why), f"chain mutant {mut} passes on {group}: the fixtures or the tolerance are too weak"


def test_chain_honest_orders_pass():
    """Every chain fixture in every honest order (fused and five-launch form): accepted; the largest ratios per stage - and of the
    inner values q and merged sums against their own E, which is what the flip window is made of - stay within C_CHAIN.  Prints the
    figures quoted in _attn_ref.py; C_CHAIN must be at least twice the largest."""
    table = {}
    for name, p in chain_fixtures().items():
        cache = {}
        for order, merge, fused in CHAIN_ORDERS:
            r = A.judge_chain(p, A.emulated_chain(p, order, merge, fused=fused), what=f"{name} {order} merge {merge}", cache=cache)
            for k, v in r.items():
                table[k] = max(table.get(k, 0.0), v)
    # the GPU test's own shapes (but the two widest, whose emulation takes the CPU a minute), the fused and the five-launch form
    for shape in sorted(set(A.CHAIN_SHAPES) - {"large", "wide"}):
        p, cache = A.build_chain_shape(shape, "ssq", 5, "R"), {}
        for order, merge, fused in (("eighths", "fma", True), ("inter16", 4, False)):
            for k, v in A.judge_chain(p, A.emulated_chain(p, order, merge, fused=fused), what=f"{shape} {order} merge {merge}", cache=cache).items():
                table[k] = max(table.get(k, 0.0), v)
    for k in sorted(table):
        print("chain stage %-6s ratio %.2f" % (k, table[k]))
    assert set(table) == {"A", "B", "C", "xctx", "q", "merged"}
    assert 2 * max(table.values()) <= A.C_CHAIN
    assert table["q"] > 0.5 and table["merged"] > 0.5


def test_chain_selector_fixtures_carry_their_traps():
    for name, p in chain_fixtures().items():
        if p.tier == "S":
            assert p.n_traps >= p.H, f"{name}: {p.n_traps} traps"
        if p.tier == "S" and p.norm != "none":
            rf = A.chain_factor(p)
            assert len(set(rf.round(6))) >= 3 and (np.log2(rf).round(3) % 1 == 0).all(), f"{name}: row factors are not distinct powers of two"
