"""The row kernels and device state machines on an MI355X through rk_debug_rows (the launchers the production path calls, every
output between sentinel bands) against tests/_rows_ref.py: exact tiers bit for bit, random tiers inside half an fp16 ulp +
C_ROWS x E of the very problem, the three advance kernels stepped alongside their Python mirrors.  Every case also checks the
bands, that a second run gives the same bytes and that plan_only reports the grid / template parameter of the Python mirror.
Shapes are the smallest that reach each edge; most of a case's time is its fp64 reference."""
import numpy as np
import pytest

import _attn_ref as A
import _attn_ref_hd64 as H64
import _rows_ref as R
from conftest import load_state
from llmrankers import _synth

pytestmark = pytest.mark.gpu

f16, f32, f64, i32 = np.float16, np.float32, np.float64, np.int32
BAND = 256
RK_ERR_INVALID = -1


@pytest.fixture(scope="module")
def t5(ckpt_dirs):
    from llmrankers._engine import RkEngine
    dims, state = load_state(ckpt_dirs["ckpt_gated_untied"])
    e = RkEngine(dims, device=0, max_tokens=512, max_seqs=4, max_dec_len=4).load_state(state.items())
    yield e
    e.close()


def _llama_engine(dims):
    from llmrankers._engine import RkLlamaEngine
    return RkLlamaEngine(dims, device=0, max_tokens=256, max_seqs=4).load_state(_synth.synth_state_dict(dims, seed=929).items())


@pytest.fixture(scope="module")
def llama():
    e = _llama_engine(_synth.TOY_LLAMA)
    yield e
    e.close()


@pytest.fixture(scope="module")
def llama64():
    e = _llama_engine(_synth.TOY_LLAMA_HD64)
    yield e
    e.close()


def sentinel(n, dt):
    return np.full(n * np.dtype(dt).itemsize, R.SENTINEL, np.uint8).view(dt)


def is_sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == R.SENTINEL).all())


def banded(a, rows=1, seed=99):
    whole, off = R.banded(np.random.RandomState(seed), np.ascontiguousarray(a).reshape(-1, a.shape[-1]), rows)
    return (whole, off)


def spec(p):
    """Problem -> (op number, ins, outs [(pre-fill, dtype)], params) of rk_debug_rows."""
    op = p.op
    if op == "embed":
        return ([p.ids, banded(p.table)], [sentinel(p.rows * p.d, f32), sentinel(p.rows * p.d, f16), sentinel(p.rows, f32)],
                dict(rows=p.rows, d=p.d, vocab=p.vocab, kind=int(p.fold), eps=p.eps, xs=p.xs))
    if op == "rowscale":
        return [p.ssq], [sentinel(p.rows, f32)], dict(rows=p.rows, nb=p.nb, d=p.d, eps=p.eps, xs=p.xs)
    if op == "rmsnorm":
        return ([banded(p.x), p.w, None if p.row_map is None else np.asarray(p.row_map, i32)], [sentinel(p.rows * p.d, f16)],
                dict(rows=p.rows, d=p.d, src_rows=p.src_rows, eps=p.eps, out_scale=p.out_scale))
    if op == "head_rows":
        return ([banded(p.x), banded(p.head), p.out_ids], [sentinel(p.rows * p.n_out, f32)], dict(rows=p.rows, n_out=p.n_out, d=p.d, vocab=p.vocab))
    if op == "pair_verdict":
        return ([banded(p.x), banded(p.head)], [sentinel(3 * p.rows + p.rows // 2, f32)],
                dict(rows=p.rows, d=p.d, vocab=p.vocab, false_id=p.false_id, true_id=p.true_id))
    if op == "argmax_blocks":
        return [p.bval, p.bidx], [sentinel(p.rows, i32)], dict(rows=p.rows, nb=p.nb)
    if op == "qlm_lse":
        return [p.stats, p.xlab, p.row_off, p.out_idx], [sentinel(p.rows, f32)], dict(rows=p.rows, nb=p.nb, n_pos=p.n_pos)
    if op == "rope":
        return ([p.pos, p.cos, p.sin, p.bias], [p.qkv], dict(rows=p.rows, H=p.H, n_kv=p.n_kv, hd=p.hd, ld=p.ld, max_pos=p.max_pos))
    assert op == "kv_fill"
    return ([(p.qkv_whole, p.qkv_off), p.seq_off, p.slots], [p.cache],
            dict(rows=p.rows, H=p.H, n_kv=p.n_kv, hd=p.hd, ld=p.ld, P=p.P, n_slots=p.n_slots))


def launch(eng, op, ins, outs, params, want_plan=None, n_steps=1):
    """One call; bands, determinism and the plan are checked here.  Returns the interiors per step as raw bytes [n_steps, bytes]."""
    if want_plan is not None:
        pl = eng.debug_rows(op, ins=ins, outs=outs, band=BAND, n_steps=n_steps, plan_only=True, **params)
        assert (pl["grid"], pl["tparam"], pl["variant"]) == want_plan, (pl, want_plan)
    res = eng.debug_rows(op, ins=ins, outs=outs, band=BAND, n_steps=n_steps, **params)
    again = eng.debug_rows(op, ins=ins, outs=outs, band=BAND, n_steps=n_steps, **params)
    got = []
    for a, b in zip(res["all"], again["all"]):
        assert np.array_equal(a, b), "a second run gives other bytes"
        assert (a[:, :BAND] == R.SENTINEL).all() and (a[:, -BAND:] == R.SENTINEL).all(), "a band was written"
        got.append(np.ascontiguousarray(a[:, BAND:-BAND]))
    return got


def run(eng, p):
    ins, outs, params = spec(p)
    got = launch(eng, R.OPS[p.op], ins, outs, params, R.plan(p))
    return [g[0].view(o.dtype) for g, o in zip(got, outs)]


RATIOS = {}


def record(op, r):
    RATIOS[op] = max(RATIOS.get(op, 0.0), r)
    print(f"max ratio so far: {op} {RATIOS[op]:.3f}")


# ---- embed -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("d,rows", [(64, 1), (576, 4), (1024, 5)])
def test_embed(t5, d, rows, fold):
    vocab = 37
    ids = [0, vocab - 1, 1, 2, 1][:rows] if rows < 5 else [-1, vocab, 0, 2, 1]     # -1 and vocab read the clamped rows, never a band row
    p = R.build_embed(100 + d, rows, d, vocab=vocab, fold=fold, ids=ids)
    out, xraw, rowscale = run(t5, p)
    want = R.expected(p)
    assert np.array_equal(out.view(np.uint32), want["out"].reshape(-1).view(np.uint32)), "out is not the fp16 row widened"
    if not fold:
        assert is_sentinel(xraw) and is_sentinel(rowscale)
        return
    assert np.array_equal(xraw.view(np.uint16), want["xraw"].reshape(-1).view(np.uint16)), "xraw is not the row x 2^-4"
    record("embed", R.judge(p, rowscale, f"embed d={d} rows={rows}"))
    zero = np.flatnonzero(np.clip(p.ids, 0, vocab - 1) == 0)
    assert abs(float(rowscale[zero[0]]) / (1.0 / np.sqrt(p.eps) / p.xs) - 1) < R.C_ROWS * R.U24 * 2     # the all-zero row: rsqrt(eps) / xs


# ---- rowscale --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,rows", [(4, 1), (8, 256), (5, 257), (1, 5), (8, 257), (5, 1)])
def test_rowscale(t5, nb, rows):
    p = R.build_rowscale(200 + nb, rows, nb)
    record("rowscale", R.judge(p, run(t5, p)[0], f"rowscale nb={nb} rows={rows}"))


# ---- rmsnorm ---------------------------------------------------------------------------------------------------------------------------
MAPS = {"none": None, "perm": [4, 0, 3, 2, 1], "repeat": [4, 0, 3, 3, 1]}


@pytest.mark.parametrize("row_map", list(MAPS))
@pytest.mark.parametrize("d", [64, 1024, 1088, 2048, 2112, 4096])
def test_rmsnorm_random(t5, d, row_map):
    rm = MAPS[row_map]
    for rows, scale in ((5, d ** -0.5), (1, 1.0)):
        p = R.build_rmsnorm(300 + d, rows, d, row_map=None if rm is None else rm[:rows], out_scale=scale, src_rows=6)
        out = run(t5, p)[0].reshape(rows, d)
        want = R.expected(p)["out"]
        assert np.isfinite(out.astype(f64)).all(), "inf instead of saturation"
        record("rmsnorm", R.judge(p, out, f"rmsnorm d={d} rows={rows} map={row_map}"))
        over = np.abs(want) > R.F16_MAX * 1.01
        assert (np.abs(out[over].astype(f64)) == R.F16_MAX).all()
        if rows == 5:
            assert over.any(), "the fixture reaches beyond 65504"
            src = np.arange(rows) if rm is None else np.asarray(rm)
            assert (out[src == 1] == 0).all(), "the zero row"


@pytest.mark.parametrize("d,scale", [(64, 0.125), (1024, 2.0 ** -5), (1088, 1.0), (2048, 1.0), (2112, 0.5), (4096, 2.0 ** -6)])
def test_rmsnorm_exact(t5, d, scale):
    for rows, rm in ((5, [4, 0, 3, 3, 1]), (5, None), (1, [5])):
        p = R.build_rmsnorm(400 + d, rows, d, tier="S", row_map=rm, out_scale=scale, src_rows=6)
        out = run(t5, p)[0].reshape(rows, d)
        assert np.array_equal(out.astype(f64), R.expected(p)["out"]), f"rmsnorm tier S d={d} rows={rows} map={rm}"


def test_rmsnorm_refuses_d_above_4096(t5):
    p = R.build_rmsnorm(1, 1, 4160)
    ins, outs, params = spec(p)
    res = t5.debug_rows(3, ins=ins, outs=outs, band=BAND, check=False, **params)
    assert res["rc"] == RK_ERR_INVALID and all(is_sentinel(a) for a in res["all"])


# ---- head rows and the pair verdict ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["S", "R"])
@pytest.mark.parametrize("d", [64, 512, 520, 4096])
def test_head_rows(t5, d, tier):
    for rows, n_out in ((1, 1), (5, 1), (1, 5), (3, 64)):
        p = R.build_head(500 + d, rows, n_out, d, tier=tier)
        out = run(t5, p)[0].reshape(rows, n_out)
        R.judge_head(p, out, f"head_rows d={d} {rows}x{n_out} tier {tier}")


@pytest.mark.parametrize("d", [64, 520])
@pytest.mark.parametrize("n_seq", [2, 6, 5])
def test_pair_verdict(t5, n_seq, d):
    for tier in ("S", "R"):
        p = R.build_verdict(600 + d, n_seq, d, tier=tier)
        out = run(t5, p)[0]
        n = n_seq // 2 * 2
        logits, p_true, verdict = out[:2 * n].reshape(n, 2), out[2 * n_seq:2 * n_seq + n], out[3 * n_seq:3 * n_seq + n // 2]
        if n_seq % 2:                                        # the unpaired last sequence: its outputs stay sentinel
            assert is_sentinel(out[2 * n:2 * n_seq]) and is_sentinel(out[2 * n_seq + n:3 * n_seq])
        h = R.problem("head_rows", tier=tier, rows=n_seq, n_out=2, d=d, vocab=p.vocab, x=p.x, head=p.head, out_ids=np.array([p.false_id, p.true_id], i32))
        head_out = run(t5, h)[0].reshape(n_seq, 2)
        assert np.array_equal(logits.view(np.uint32), head_out[:n].view(np.uint32)), "the verdict kernel's logits are not head_rows' bytes"
        R.judge_head(h, head_out, f"pair_verdict logits n_seq={n_seq} d={d} tier {tier}")
        assert np.isfinite(p_true).all()
        want = R.verdict_expected(p, logits=logits.astype(f64))
        err = float(np.abs(p_true.astype(f64) - want["p_true"]).max())
        print(f"pair_verdict n_seq={n_seq} d={d} tier {tier}: max |P(true) - fp64| = {err:.3g}")
        assert err <= R.P_TOL
        assert np.array_equal(verdict, R.verdict_expected(p, logits=logits, p_true=p_true)["verdict"])
        if tier == "S":
            assert np.array_equal(logits[0], logits[1]) and verdict[0] == 0.0, "an exact tie gives verdict 0"
            if n_seq >= 4:
                assert p_true[2] == 1.0 and p_true[3] == 0.0 and verdict[1] == 1.0


# ---- argmax over blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3, 256, 257, 1004])
def test_argmax_blocks(t5, nb):
    p = R.build_argmax(700 + nb, 4, nb)
    assert np.array_equal(run(t5, p)[0], R.expected(p)["out"])


# ---- qlm -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 255, 257, 1004])
def test_qlm_lse(t5, nb):
    for kw in (dict(n_pos=1), dict(n_pos=33), dict(row_lens=[3, 0, 33, 1], out_idx=[2, 0, 3, 1]), dict(row_lens=[2, 5, 1, 4])):
        p = R.build_qlm(800 + nb, 4, nb, **kw)
        out = run(t5, p)[0]
        assert np.isfinite(out).all()
        record("qlm_lse", R.judge(p, out, f"qlm_lse nb={nb} {kw}"))
        if "out_idx" in kw:
            assert out[0] == 0.0, "an empty sequence scores 0"


# ---- rope ------------------------------------------------------------------------------------------------------------------------------
ROPE_SHAPES = [(128, 1, 1), (128, 4, 2), (128, 32, 8), (64, 1, 1), (64, 4, 2), (64, 32, 8), (64, 64, 8)]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("hd,H,n_kv", ROPE_SHAPES)
def test_rope(t5, hd, H, n_kv, bias):
    for T in (1, 7):
        for tier in ("S", "R"):
            p = R.build_rope(900 + hd + H + T, T, H, n_kv, hd, tier=tier, bias=bias)
            out = run(t5, p)[0].reshape(T, p.ld)
            want = R.expected(p)
            untouched = ~want["touched"]
            assert np.array_equal(out[untouched].view(np.uint16), p.qkv[untouched].view(np.uint16)), "pad columns / bias-free value heads were touched"
            assert untouched[:, -8:].all() and (bias or untouched[:, (H + n_kv) * hd:].all())
            if tier == "S":
                assert np.array_equal(out.astype(f64), want["out"]), f"rope tier S hd={hd} H={H} n_kv={n_kv} T={T} bias={bias}"
            else:
                record("rope", R.judge(p, out, f"rope hd={hd} H={H} n_kv={n_kv} T={T} bias={bias}"))


# ---- kv fill -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,n_kv", [(128, 1), (128, 8), (128, 17), (64, 1), (64, 8), (64, 33)])
def test_kv_fill(t5, hd, n_kv):
    lens = [1, 5, 3]
    for P in (5, 7, 3):                                      # the longest prompt, a longer cache, a shorter one (rows t >= P are dropped)
        for slots, n_slots in ((None, 0), ([2, -1, 0], 4), ([1, 4, 3], 4)):      # -1 and n_slots are skipped
            p = R.build_kv_fill(1000 + hd + n_kv, n_kv, n_kv, hd, lens, P, slots=slots, n_slots=n_slots)
            out = run(t5, p)[0]
            want = R.expected(p)["out"]
            assert np.array_equal(out.view(np.uint16), want.view(np.uint16)), f"kv_fill hd={hd} n_kv={n_kv} P={P} slots={slots}"
            assert not np.array_equal(out.view(np.uint16), p.cache.view(np.uint16))


def test_kv_fill_more_query_heads_than_kv_heads(t5):
    for hd in (128, 64):
        p = R.build_kv_fill(1100 + hd, 6, 2, hd, [2, 4], 4)
        assert np.array_equal(run(t5, p)[0].view(np.uint16), R.expected(p)["out"].view(np.uint16))


# ---- the advance kernels -------------------------------------------------------------------------------------------------------------------
def steps_equal(got, machine_states, what):
    for s, want in enumerate(machine_states):
        for i, w in enumerate(want):
            g = got[i][s].view(i32)
            assert np.array_equal(g, w.reshape(-1)), f"{what}: step {s}, state array {i}: {g.tolist()[:16]} != {w.reshape(-1).tolist()[:16]}"


def script_for(rs, n_seq, n_steps, vocab=50):
    return rs.randint(3, vocab, size=(n_steps, n_seq)).astype(i32)


@pytest.mark.parametrize("n_seq", [1, 3, 257])
def test_greedy_advance(t5, n_seq):
    rs = np.random.RandomState(n_seq)
    eos, pad = 1, 0
    for name, dec_len, max_new in (("prefix3", 3, 4), ("eos_first", 1, 3), ("all_at_once", 1, 5), ("nobody", 2, 3)):
        n_steps = dec_len - 1 + max_new + 2                  # two steps past the end
        script = script_for(rs, n_seq, n_steps)
        if name == "eos_first":
            script[0, 0] = eos                               # EOS at column 0
        if name == "all_at_once":
            script[1, :] = eos                               # every row finishes in one step
        if name == "prefix3":
            script[dec_len, ::2] = eos
        prefix = np.arange(11, 11 + dec_len).astype(i32)
        init = [np.array([0, 0, eos, pad], i32), np.zeros(n_seq, i32), np.full(n_seq * max_new, -1, i32), np.full(n_seq, -1, i32)]
        m = R.GreedyMachine(init[0], prefix, init[1], init[2], init[3], dec_len, max_new)
        states = []
        for s in range(n_steps):
            states.append([a.copy() for a in m.step(script[s]).state()])
        got = launch(t5, 10, [script, prefix], init, dict(kind=0, rows=n_seq, dec_len=dec_len, max_new=max_new), ((1, 1, 1), 0, 0), n_steps)
        steps_equal(got, states, f"greedy {name} n_seq={n_seq}")
        assert states[-1][0][0] == dec_len + max_new - 1 and not any(np.any(a != b) for a, b in zip(states[-1], states[-2]))
        if name == "nobody":
            assert states[-1][0][1] == max_new
        if name == "all_at_once":
            assert states[-1][0][1] == 2


@pytest.mark.parametrize("n_seq", [1, 3, 257])
def test_llama_advance(t5, n_seq):
    rs = np.random.RandomState(10 + n_seq)
    for name, max_new, max_total, P in (("eos", 4, 0, 64), ("max_total", 5, 9, 64), ("cache_end", 6, 0, 10), ("nobody", 3, 0, 64)):
        n_steps = max_new + 2
        script = script_for(rs, n_seq, n_steps)
        if name == "eos":
            script[0, 0] = 1
            script[1, :] = 2                                 # the second EOS id: everybody finishes in one step
        length = rs.randint(4, 8, size=n_seq).astype(i32)
        if name == "max_total":
            length[0] = 8                                    # prompt + 1 == max_total: finishes at column 0
        st = np.array([0, 0, 0, 2, max_new, max_total, P, 0, 1, 2, 0, 0, 0, 0, 0, 0], i32)
        init = [st, np.zeros(n_seq, i32), np.full(n_seq, -1, i32), np.full(n_seq * max_new, -1, i32), np.full(n_seq, -1, i32)]
        m = R.LlamaMachine(st, length, init[1], init[2], init[3], init[4])
        states = []
        for s in range(n_steps):
            states.append([a.copy() for a in m.step(script[s]).state()])
        got = launch(t5, 10, [script, length], init, dict(kind=1, rows=n_seq), ((1, 1, 1), 0, 1), n_steps)
        steps_equal(got, states, f"llama {name} n_seq={n_seq}")
        assert not any(np.any(a != b) for a, b in zip(states[-1], states[-2])), "a step past the end changes nothing"
        if name == "cache_end":
            assert (states[-1][2] == P - 1).any(), "a position reaches the cache's last row and is held there"
        if name == "nobody":
            assert states[-1][0][1] == max_new


@pytest.mark.parametrize("n_slots", [5, 257])
def test_session_advance(t5, n_slots):
    cap, max_len, pad, A = 4, 12, 0, 3
    st = np.array([0, pad, 1, max_len, cap, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], i32)
    length, col, max_new, done = (np.zeros(n_slots, i32) for _ in range(4))
    done[:] = 1
    length[[1, 3]], col[[1, 3]], max_new[[1, 3]], done[[1, 3]] = [5, 9], [1, 2], [4, 9], 0     # slots 1 and 3 decode, 4 idles
    pos = np.where(done == 0, length + col - 1, 0).astype(i32)
    init = [st, length, col, max_new, done, pos, np.full(n_slots * cap, -1, i32), np.full(n_slots, -1, i32)]
    n_steps = 10
    rs = np.random.RandomState(n_slots)
    script = rs.randint(3, 50, size=(n_steps, max(n_slots, A))).astype(i32)
    script[3, 1] = 1                                         # slot 1 meets EOS
    admits = np.full((n_steps, 1 + 3 * A), -1, i32)
    adm = {1: ([0, 2, n_slots], [4, 6, 1], [1, 4, 1]),       # into slots 0 (max_new 1: finishes here) and 2; one entry out of range
           4: ([0], [3], [cap + 3])}                         # slot 0 again, max_new beyond cap: ends at cap
    for s, (sl, ln, mn) in adm.items():
        admits[s, 0] = len(sl)
        admits[s, 1:1 + 3 * len(sl)] = sl + ln + mn
    admits[5, 0] = 0                                         # an empty admit list touches nothing
    m = R.SessionMachine(*init)
    states = []
    for s in range(n_steps):
        n = int(admits[s, 0])
        a = None if n < 0 else (admits[s, 1:1 + n], admits[s, 1 + n:1 + 2 * n], admits[s, 1 + 2 * n:1 + 3 * n])
        states.append([x.copy() for x in m.step(script[s], a).state()])
    got = launch(t5, 10, [script, admits], init, dict(kind=2, rows=n_slots, max_admit=A), ((1, 1, 1), 0, 2), n_steps)
    steps_equal(got, states, f"session n_slots={n_slots}")
    fin = [int(s[0][0]) for s in states]
    assert fin[1] == fin[0] + 1 and fin[-1] >= 4 and all(b >= a for a, b in zip(fin, fin[1:])), fin
    assert all(s[2][4] == 0 and s[7][4] == pad for s in states), "the idle slot"
    assert np.array_equal(states[5][6], states[4][6]) and states[5][0][0] == states[4][0][0], "an empty admit list"


def test_advance_refusals(t5):
    st = np.array([0, 0, 0, 9, 4, 0, 64, 0] + [0] * 8, i32)  # n_eos = 9
    init = [st, np.zeros(2, i32), np.zeros(2, i32), np.zeros(8, i32), np.zeros(2, i32)]
    res = t5.debug_rows(10, ins=[np.zeros((1, 2), i32), np.ones(2, i32)], outs=init, band=BAND, check=False, kind=1, rows=2)
    assert res["rc"] == RK_ERR_INVALID and all(is_sentinel(a) for a in res["all"])


# ---- either family ---------------------------------------------------------------------------------------------------------------------
def test_a_llama_engine_gives_the_same_bytes(t5, llama):
    for p in (R.build_embed(1, 5, 576), R.build_rmsnorm(2, 5, 1088, row_map=[4, 0, 3, 3, 1], src_rows=6), R.build_rope(3, 7, 4, 2, 64, bias=True),
              R.build_rope(3, 7, 4, 2, 128), R.build_kv_fill(4, 4, 2, 128, [1, 5, 3], 6, slots=[2, -1, 0], n_slots=4), R.build_qlm(5, 2, 257, n_pos=3)):
        for a, b in zip(run(t5, p), run(llama, p)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), p.op


# ---- the cached key IS the prefill's key -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("hd", [128, 64])
def test_cached_key_is_the_prefills_key(llama, llama64, hd, bias):
    """The rope op's rotated key heads and biased value heads of an unrotated row at position p are, byte for byte, what the cached
    step (rk_debug_attn kind 5) appends to the cache at p from the same row."""
    eng, mod = (llama, A) if hd == 128 else (llama64, H64)
    H, n_kv, pos, P, band = 4, 2, [0, 5, 17], 20, 8
    p = mod.build_step(77, H, n_kv, pos, P, "R", bias=bias, band=band)
    res = eng.debug_attn(A.STEP, n_seq=p.n_seq, H=H, q=p.q, out=p.out, band_rows=band, n_kv=n_kv, P=P, ldq=p.ldq, ldctx=p.ldctx, pos=p.pos,
                         cos=p.cos, sin=p.sin, qkv_bias=p.qkv_bias, cache=p.cache)
    cache = res["cache"][band * hd:-band * hd].reshape(2, p.n_seq, n_kv, P, hd)
    rows = np.ascontiguousarray(p.q[band:band + p.n_seq])
    rp = R.problem("rope", rows=p.n_seq, H=H, n_kv=n_kv, hd=hd, ld=p.ldq, max_pos=P, pos=p.pos, cos=p.cos, sin=p.sin, bias=p.qkv_bias, qkv=rows)
    out = run(eng, rp)[0].reshape(p.n_seq, p.ldq)
    for b in range(p.n_seq):
        for g in range(n_kv):
            k = out[b, (H + g) * hd:(H + g + 1) * hd]
            v = out[b, (H + n_kv + g) * hd:(H + n_kv + g + 1) * hd]
            assert np.array_equal(k.view(np.uint16), cache[0, b, g, pos[b]].view(np.uint16)), f"hd={hd} bias={bias}: key of row {b}, kv head {g}"
            assert np.array_equal(v.view(np.uint16), cache[1, b, g, pos[b]].view(np.uint16)), f"hd={hd} bias={bias}: value of row {b}, kv head {g}"


# ---- the T5 cached step (rk_debug_attn kind 6) ---------------------------------------------------------------------------------------------
CACHED_POS = [(1, 0), (18, 0), (18, 1), (18, 15), (18, 16), (18, 17), (300, 255), (300, 256), (300, 299)]


def cached_call(eng, p, **kw):
    return eng.debug_attn(6, n_seq=p.n_seq, H=p.H, q=p.step_q, out=p.out, band_rows=p.band, P=p.P, ldq=p.ldq, ldctx=p.ldctx, pos=p.pos,
                          bias_lut=p.lut, cache=p.step_cache, **kw)


@pytest.mark.parametrize("H,n_seq", [(1, 1), (6, 3)])
@pytest.mark.parametrize("P,pos", CACHED_POS)
def test_t5_cached_step(t5, P, pos, H, n_seq):
    for tier in ("S", "R"):
        p = R.build_cached_step(1200 + P + pos, H, n_seq, P, pos, tier)
        if tier == "S":
            assert p.n_traps > 0 or pos == 0
        got = {}
        for opt in (1, 0):
            t5.set_option("dec_cached_attn", opt)
            try:
                plan = cached_call(t5, p, plan_only=True)
                assert plan["kind"] == opt and plan["grid"] == ((H, n_seq, 1) if opt else (n_seq, 1, 1)) and plan["lds"] == (64 + 256 + 8 + P) * 4
                assert opt or plan["grid2"] == (1, H, n_seq)
                r1, r2 = cached_call(t5, p), cached_call(t5, p)
            finally:
                t5.set_option("dec_cached_attn", 1)
            b, cb = p.band, p.band * 64
            assert r1["out"].tobytes() == r2["out"].tobytes() and r1["cache"].tobytes() == r2["cache"].tobytes(), "a second run gives other bytes"
            assert is_sentinel(r1["out"][:b]) and is_sentinel(r1["out"][-b:]) and is_sentinel(r1["cache"][:cb]) and is_sentinel(r1["cache"][-cb:])
            ratios = A.judge(p, r1["out"][b:-b], what=f"cached step P={P} pos={pos} H={H} n_seq={n_seq} tier {tier} option {opt}")
            if tier == "R":
                record("t5_cached_step", max(ratios.values()))
            assert np.array_equal(r1["cache"][cb:-cb].view(np.uint16), R.cached_step_cache_expected(p).view(np.uint16)), "the cache after the step"
            got[opt] = (r1["out"].tobytes(), r1["cache"].tobytes())
        assert got[0] == got[1], "dec_cached_attn 0 and 1 give other bytes"


def test_t5_cached_step_refuses_pos_outside_the_cache(t5):
    from llmrankers._engine import RkError
    p = R.build_cached_step(7, 1, 1, 18, 17, "R")
    p.pos = np.array([18], i32)
    with pytest.raises(RkError) as ei:
        cached_call(t5, p)
    assert ei.value.code == RK_ERR_INVALID
