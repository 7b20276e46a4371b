"""The reference and tolerance model of tests/_rows_ref.py on the CPU: the honest fp32 orders pass and reproduce C_ROWS, every
mutant - one broken rule each - is rejected by the tier meant to catch it, and rk_engine_create refuses d_model > 4096.  No GPU:
the "kernel" of every case is a numpy stand-in."""
import numpy as np
import pytest

import _attn_ref as A
import _rows_ref as R

f16, f32, f64 = np.float16, np.float32, np.float64


def test_honest_orders_pass_and_c_rows():
    worst, c = R.measure_c_rows()
    print({k: round(v, 2) for k, v in worst.items()}, c)
    assert set(worst) == set(R.TOLERANCED)
    assert max(worst.values()) <= R.C_ROWS
    assert c == R.C_ROWS, f"measured C_ROWS {c}, the module says {R.C_ROWS}"
    doc = R.__doc__
    for op, name in (("embed", "embed rowscale"), ("rowscale", "  rowscale"), ("rmsnorm", "rmsnorm"), ("rope", "rope"), ("qlm_lse", "qlm_lse")):
        assert f"{name} {worst[op]:.2f}" in doc, f"{op}: measured {worst[op]:.2f}, the docstring says otherwise"


def test_rope_reference_agrees_with_the_attention_references():
    """rope_expected restates what _attn_ref.rope64 (hd 128) and _attn_ref_hd64.rope_head (hd 64) hold."""
    import _attn_ref_hd64 as H64
    for hd in (128, 64):
        p = R.build_rope(3, 3, 2, 1, hd, bias=True)
        want = R.rope_expected(p)["out"]
        for t in range(p.rows):
            for h in range(p.H + p.n_kv):
                row, b = p.qkv[t, h * hd:(h + 1) * hd], p.bias[h * hd:(h + 1) * hd]
                c, s = p.cos[p.pos[t]], p.sin[p.pos[t]]
                ref = A.rope64(row, c, s, b) if hd == 128 else H64.rope_head(p.qkv[t][:p.bias.size], h * hd, c, s, p.bias)
                assert np.allclose(want[t, h * hd:(h + 1) * hd], np.asarray(ref, dtype=f64), rtol=0, atol=1e-12)


# ---- mutants: (builder, mutant) -> rejected by the random tier's bound or by an exact comparison ---------------------------------------
def _rejected_R(p, mut, key=None):
    key = key or R.TOLERANCED[p.op]
    bad = R.expected(p, mut)[key]
    bad = R.f16_sat(bad) if p.op in ("rmsnorm", "rope") and np.isfinite(bad).all() else bad
    honest = R.emulated(p)[key]
    honest = R.f16_sat(honest) if p.op in ("rmsnorm", "rope") else honest
    assert R.miss(p, honest) <= R.C_ROWS, "the honest emulation must pass where the mutant is tried"
    g = np.asarray(bad).astype(f64)
    return (not np.isfinite(g).all()) or R.miss(p, bad) > 100 * R.C_ROWS


@pytest.mark.parametrize("mut", ["no_eps", "times_xs"])
def test_embed_mutants(mut):
    assert _rejected_R(R.build_embed(1, 5, 576), mut)


def test_embed_exact_tier_sees_the_scaling():
    p = R.build_embed(2, 5, 64)
    want = R.expected(p)
    assert np.array_equal(want["out"], p.table[np.clip(p.ids, 0, p.vocab - 1)].astype(f32))
    sub = want["xraw"][2].astype(f64)                       # id 1: subnormal after scaling, and the smallest subnormal flushed to 0
    assert (sub[0::3] == 2.0 ** -17).all() and (sub[1::3] == 0).all()
    assert (np.abs(want["xraw"][3].astype(f64)) == 4094.0).all()   # id 2: 65504 / 16
    assert want["rowscale"][0] == pytest.approx(1.0 / np.sqrt(p.eps) / p.xs)   # id 0: the all-zero row


@pytest.mark.parametrize("mut", ["row_map_ignored", "weight_c4", "round_before_scale"])
@pytest.mark.parametrize("tier", ["S", "R"])
def test_rmsnorm_mutants(mut, tier):
    p = R.build_rmsnorm(5, 5, 1088 if tier == "R" else 1024, tier=tier, row_map=[4, 0, 3, 3, 1], out_scale=1088 ** -0.5 if tier == "R" else 2.0 ** -5, src_rows=6)
    if tier == "S":
        want, bad = R.expected(p)["out"], R.expected(p, mut)["out"]
        assert np.array_equal(R.f16_sat(want).astype(f64), want), "tier S must be exact in fp16"
        if mut == "round_before_scale":                      # exact products: rounding first changes nothing - the random tier's mutant
            assert np.array_equal(bad, want)
        else:
            assert not np.array_equal(bad, want)
    else:
        assert _rejected_R(p, mut)


def test_rmsnorm_exact_tier_is_exact_in_fp32():
    """mean square + eps is 4^k exactly: every fp32 order gives the reference's bits."""
    p = R.build_rmsnorm(6, 5, 2112 - 64, tier="S", row_map=[4, 0, 3, 3, 1], out_scale=0.125, src_rows=6)
    want = R.expected(p)["out"]
    ms = (p.x.astype(f64) ** 2).mean(axis=1) + p.eps
    assert set(ms) <= {1.0, 4.0, 16.0} and len(set(ms)) == 3
    for order in ("lanes", "chain", "pairwise"):
        assert np.array_equal(R.emulated(p, order)["out"].astype(f64), want)


def test_rmsnorm_hole_at_4160_and_saturation():
    """The width hole as a reference-side mutant: the mean over 4096 of 4160 columns and 64 columns never written."""
    p = R.build_rmsnorm(7, 2, 4160)
    want, bad = R.expected(p)["out"], R.expected(p, "first_4096")["out"]
    assert np.isnan(bad[:, 4096:]).all() and np.isfinite(want).all()
    q = R.build_rmsnorm(7, 2, 4160)
    q.x, q.w, q.d = p.x[:, :4096], p.w[:4096], 4096         # the written part, judged as a 4096-wide problem of the same values
    assert R.miss(q, R.f16_sat(bad[:, :4096]), want[:, :4096], R.yardstick(p)) > 100 * R.C_ROWS
    q = R.build_rmsnorm(8, 5, 1024, src_rows=6)
    assert (np.abs(R.expected(q)["out"]) > R.F16_MAX).any(), "the fixture must reach beyond 65504"
    assert _rejected_R(q, "inf")


@pytest.mark.parametrize("mut", ["next_id", "first_512"])
@pytest.mark.parametrize("tier", ["S", "R"])
def test_head_rows_mutants(mut, tier):
    p = R.build_head(9, 3, 5, 520, tier=tier)
    with pytest.raises(AssertionError):
        R.judge_head(p, R.head_expected(p, mut)["out"].astype(f32), mut)
    R.judge_head(p, R.head_expected(p)["out"].astype(f32), "honest")


def test_pair_verdict_mutants():
    p = R.build_verdict(10, 6, 64, tier="S")
    want = R.verdict_expected(p)
    lg = want["logits"]
    assert lg[0].tolist() == lg[1].tolist() and want["verdict"][0] == 0.0, "pair 0 is an exact tie: verdict 0"
    assert want["p_true"][2] == 1.0 and want["p_true"][3] < 1e-50 and want["verdict"][1] == 1.0   # exp(-128): 0 in fp32, 3e-56 in fp64
    assert R.verdict_expected(p, mut="tie_ge")["verdict"][0] == 1.0
    sw = R.verdict_expected(p, mut="swapped")["p_true"]
    assert np.abs(sw - want["p_true"]).max() > 1000 * R.P_TOL


@pytest.mark.parametrize("mut", ["last_tie", "wave_order"])
def test_argmax_mutants(mut):
    p = R.build_argmax(11, 4, 257)
    want, bad = R.expected(p)["out"], R.expected(p, mut)["out"]
    assert want[1] == p.bidx[1].min() and want[2] == 17
    assert not np.array_equal(want, bad)
    if mut == "wave_order":
        assert bad[2] == 4000 or bad[2] == 5000


@pytest.mark.parametrize("mut", ["no_rescale", "row_off_ignored", "out_idx_ignored", "sign"])
def test_qlm_mutants(mut):
    p = R.build_qlm(12, 4, 257, row_lens=[3, 0, 33, 1], out_idx=[2, 0, 3, 1])
    want = R.expected(p)["out"]
    assert want[0] == 0.0 and np.isfinite(want).all()        # the empty sequence (out_idx[1] = 0) scores 0
    bad = R.expected(p, mut)["out"]
    assert (not np.isfinite(bad).all()) or R.miss(p, bad.astype(f32)) > 100 * R.C_ROWS
    assert R.miss(p, R.emulated(p)["out"]) <= R.C_ROWS


ROPE_MUTANTS = ["partner_quarter", "sin_sign", "pos_plus1", "row_t", "bias_after", "bias_next_head", "values_no_bias", "keys_not_rotated"]


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("mut", ROPE_MUTANTS)
def test_rope_mutants_fail_the_exact_tier(mut, hd):
    p = R.build_rope(13, 7, 4, 2, hd, tier="S", bias=True)
    want, bad = R.expected(p)["out"], R.expected(p, mut)["out"]
    assert np.array_equal(R.f16_sat(want).astype(f64), want), "tier S is a signed permutation of integers: exact in fp16"
    assert not np.array_equal(want, bad), f"{mut} survives tier S"
    for order in ("lanes", "chain", "pairwise"):
        assert np.array_equal(R.emulated(p, order)["out"].astype(f64), want)


@pytest.mark.parametrize("mut", ["partner_quarter", "sin_sign", "pos_plus1", "bias_after", "values_no_bias"])
def test_rope_mutants_fail_the_random_tier(mut):
    assert _rejected_R(R.build_rope(14, 7, 4, 2, 128, bias=True), mut)


@pytest.mark.parametrize("mut", ["slots_ignored", "kv_swapped", "stride_H", "row_plus1"])
def test_kv_fill_mutants(mut):
    p = R.build_kv_fill(15, 4, 2, 64, [1, 5, 3], 6, slots=[2, -1, 0], n_slots=4)
    want, bad = R.expected(p)["out"], R.expected(p, mut)["out"]
    assert not np.array_equal(want.view(np.uint16), bad.view(np.uint16))
    c = want.reshape(2, 4, 2, 6, 64)
    pre = p.cache.reshape(c.shape)
    assert np.array_equal(c[:, 1], pre[:, 1]) and np.array_equal(c[:, 3], pre[:, 3]) and np.array_equal(c[:, 2, :, 1:], pre[:, 2, :, 1:])


# ---- the state machines --------------------------------------------------------------------------------------------------------------
def _run(machine, script, admits=None):
    states = []
    for s, am in enumerate(script):
        if admits is not None:
            machine.step(am, admits[s])
        else:
            machine.step(am)
        states.append([a.copy() for a in machine.state()])
    return states


def _differs(a, b):
    return any(not np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def greedy_case(mut=None):
    n_seq, dec_len, max_new, eos, pad = 3, 3, 4, 1, 0
    script = [[7, 8, 9], [7, 8, 9], [7, 1, 9], [1, 5, 9], [5, 5, 1], [4, 4, 4], [4, 4, 4], [4, 4, 4]]
    m = R.GreedyMachine([0, 0, eos, pad], [0, 11, 12], [0] * n_seq, [-1] * (n_seq * max_new), [-1] * n_seq, dec_len, max_new, mut)
    return m, script


def llama_case(mut=None):
    n_seq, max_new, P = 3, 5, 9
    st = [0, 0, 0, 2, max_new, 8, P, 0, 1, 2] + [0] * 6
    script = [[7, 1, 9], [7, 5, 2], [7, 5, 5], [7, 5, 5], [7, 5, 5], [3, 3, 3], [3, 3, 3]]
    return R.LlamaMachine(st, [4, 6, 5], [0] * n_seq, [0] * n_seq, [-1] * (n_seq * max_new), [-1] * n_seq, mut), script


def session_case(mut=None):
    n_slots, cap, max_len = 5, 4, 12
    st = [0, 0, 1, max_len, cap, 0, 0, 0, 1] + [0] * 7
    # slots 1 and 3 decode, slot 4 idles, slots 0 and 2 are admitted at step 1
    m = R.SessionMachine(st, [3, 5, 0, 9, 0], [0, 1, 0, 2, 0], [0, 4, 0, 9, 0], [1, 0, 1, 0, 1], [0, 5, 0, 10, 0], [-1] * (n_slots * cap),
                         [-1] * n_slots, mut)
    script = [[7, 7, 7, 7, 7], [8, 9, 0, 0, 0], [6, 6, 6, 6, 6], [6, 1, 6, 6, 6], [6, 6, 6, 6, 6], [6, 6, 6, 6, 6]]
    admits = [None, ([0, 2, 7], [4, 6, 1], [1, 4, 1]), None, None, None, None]
    return m, script, admits


@pytest.mark.parametrize("mut", ["no_pad", "finish_off_by_one", "pos_not_held"])
def test_greedy_and_llama_machine_mutants(mut):
    for case in (greedy_case, llama_case):
        m, script = case()
        b, _ = case(mut)
        assert _differs(_run(m, script), _run(b, script)), f"{case.__name__}: {mut} survives the script"


def test_greedy_machine_script():
    m, script = greedy_case()
    states = _run(m, script)
    out = states[-1][2].reshape(3, 4)
    assert out.tolist() == [[7, 1, 0, 0], [1, 0, 0, 0], [9, 9, 1, 0]]     # forced prefix of 3, pad after EOS
    assert states[-1][0][1] == 3 and states[-1][0][0] == 6                # all finished at column 2; the position held at dec_len + max_new - 1
    assert not _differs(states[-2:-1], states[-1:])                       # steps past the end: nothing but pads over pads


def test_llama_machine_script():
    m, script = llama_case()
    states = _run(m, script)
    out = states[-1][3].reshape(3, 5)
    assert out[0].tolist() == [7, 7, 7, 7, 0] and out[1].tolist() == [1, 0, 0, 0, 0] and out[2].tolist() == [9, 2, 0, 0, 0]
    assert states[-1][0][1] == 4 and states[-1][2].tolist() == [8, 8, 8]  # max_total ends row 0 at column 3; positions held at P - 1
    assert not _differs(states[-2:-1], states[-1:])


@pytest.mark.parametrize("mut", ["done_counted_twice", "admit_resets_all", "pos_not_held"])
def test_session_machine_mutants(mut):
    m, script, admits = session_case()
    b, _, _ = session_case(mut)
    assert _differs(_run(m, script, admits), _run(b, script, admits))


def test_session_machine_script():
    m, script, admits = session_case()
    states = _run(m, script, admits)
    fin = [int(s[0][0]) for s in states]
    # slot 0 (max_new 1) finishes at its admit, slot 3 at cap, slot 1 at EOS, slot 2 at its max_new; nothing is counted again
    assert fin == [0, 1, 2, 3, 4, 4], fin
    assert states[-1][4].tolist() == [1, 1, 1, 1, 1] and states[1][1].tolist() == [4, 5, 6, 9, 0]
    assert all(s[2][4] == 0 and s[7][4] == 0 for s in states)   # the idle slot: column 0, pad as its next input
    assert states[-1][5][3] == 11             # slot 3's position is held at max_len - 1


# ---- the width limit of the engine -----------------------------------------------------------------------------------------------------
def test_engine_create_refuses_d_model_above_4096():
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from llmrankers import _engine
    lib = _engine.load_library()

    def create(d_model):
        desc = _engine.RkModelDesc(vocab=1024, d_model=d_model, n_heads=8, d_kv=64, d_ff=256, n_enc_layers=1, n_dec_layers=1, n_buckets=32,
                                   max_distance=128, gated_gelu=1, tied_head=0, eps=1e-6, max_tokens=64, max_seqs=2, max_dec_len=2)
        h = C.c_void_p()
        rc = lib.rk_engine_create(C.byref(desc), 0, C.byref(h))
        msg = (lib.rk_last_error(None) or b"").decode()
        if rc == 0:
            lib.rk_engine_destroy(h)
        return rc, msg

    rc, msg = create(4160)
    assert rc == -1 and "4096" in msg and "d_model" in msg, (rc, msg)
    rc, msg = create(4096)
    assert rc in (0, -2, -3), (rc, msg)        # accepted up to the device lookup
