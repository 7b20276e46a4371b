"""The reference of the drafting step (tests/_attn_ref_draft.py) checked without a GPU on the very problems
tests/test_gpu_draft_attention.py runs: the documented arithmetic passes, g1 sequential plain steps of the step modules give the
same bytes, every broken rule fails, and the problems hold the edges and the poison they are meant to."""
import numpy as np
import pytest

import _attn_ref as A
import _attn_ref_draft as X

f16 = np.float16
SOME = [(128, (4, 2)), (64, (8, 2)), (128, (28, 4)), (64, (4, 4)), (128, (8, 1))]


def some_problems(tiers="SR", W=0, calls=(0, 1, 2)):
    for n, g1 in enumerate(X.G1S):
        for call in calls:
            hd, heads = SOME[(n + call) % len(SOME)]
            for tier in tiers:
                yield X.problem(hd, heads, g1, call, tier, bias=(call == 1), W=W if tier == "R" else 0), f"hd {hd} {heads} g1 {g1} call {call} {tier}"


def test_the_documented_arithmetic_passes():
    for p, what in list(some_problems()) + list(some_problems("R", W=64)) + [(X.problem(128, (4, 2), 4, 0, "R", qkn=True), "qkn")]:
        r = X.judge(p, X.emulated(p), what)
        X.judge_cache(p, X.emulated_cache(p), what)
        assert r <= 1.0 + 1e-9, (what, r)                    # the yardstick IS this arithmetic's error


def _plain_items(c):
    if c.qk_w is not None:
        import _qwen3_ref as Q
        return Q.qkn_step_items(c, True)
    return X._mod(c).items(c, None, True)


def test_sequential_plain_steps_give_the_same_bytes():
    """The contract above attn_dec_cached_body: call j of g1 plain steps feeds row (s, j) on the cache call j - 1 left; every live
    row's context and the final cache are the drafting reference's byte for byte (both in the kernels' documented arithmetic)."""
    for p, what in list(some_problems()) + [(X.problem(128, (4, 2), 8, 2, "R", qkn=True), "qkn")]:
        want, cache = X.emulated(p), p.cache.copy()
        seen = set()
        for src, c in X.sequential(p):
            c.cache = cache
            half = cache.size // 2
            nxt = cache.copy()
            for it in _plain_items(c):
                b, g, pos, knew, vnew = it["new"]
                o = ((b * c.n_kv + g) * c.P + pos) * c.hd
                nxt[o:o + c.hd], nxt[half + o:half + o + c.hd] = knew, vnew
                ctx = A.emulate_item(it).astype(f16)
                col = it["out_col"]
                assert np.array_equal(ctx.view(np.uint16)[0], want[src[b], col:col + c.hd].view(np.uint16)), (what, src[b], col)
                seen.add(int(src[b]))
            cache = nxt
        assert seen == set(np.flatnonzero(p.live).tolist())
        assert np.array_equal(cache.view(np.uint16), X.emulated_cache(p).view(np.uint16)), what


@pytest.mark.parametrize("mut", X.MUTANTS)
def test_mutants_fail(mut):
    """row j seeing key pos + 1 (the next row's key or the poison), the append ignoring `live`, the append using b instead of b // g1,
    the window's first key off by one either way: each fails the context's or the cache's check on every problem where it can show"""
    windowed = mut.startswith("lo_")
    n = 0
    for p, what in some_problems("R" if windowed else "SR", W=64 if windowed else 0):
        live = p.live.reshape(p.n_slots, p.g1)
        if mut == "append_ignores_live" and live.all():
            continue
        if windowed and not (p.pos[p.live == 1] >= p.W).any():
            continue
        fails = 0
        for check, got in ((X.judge, X.emulated(p, mut)), (X.judge_cache, X.emulated_cache(p, mut))):
            try:
                check(p, got, f"{what} mutant {mut}")
            except AssertionError:
                fails += 1
        assert fails, f"{what}: mutant {mut} passes"
        n += 1
    assert n >= 6, (mut, n)


def test_problems_hold_their_edges():
    for g1 in X.G1S:
        pos_live, pos_dead = set(), 0
        for call in range(3):
            p = X.problem(128, (4, 2), g1, call, "R", W=64)
            live, pos = p.live.reshape(p.n_slots, g1), p.pos.reshape(p.n_slots, g1)
            kc = p.cache[:p.cache.size // 2].reshape(p.n_slots, p.n_kv, p.P, p.hd).view(np.uint16)
            for s in range(p.n_slots):
                top = int(pos[s][live[s] == 1].max())
                assert (kc[s, :, top + 1:] == X.NAN16).all() and np.isfinite(kc[s, :, :top + 1].view(f16)).all(), "poison above the highest live position only"
                pos_live.update(int(t) for t in pos[s][live[s] == 1])
            pos_dead += int((live == 0).sum())
            assert live[:, 0].all() and 2 <= p.n_slots <= 3
        for a, b in ((31, 32), (63, 64), (127, 128), (255, 256), (190, 191)):
            assert a in pos_live and b in pos_live, (g1, a, b)
        assert 0 in pos_live and X.P_DRAFT - 1 in pos_live and pos_dead >= g1 - 1
        lo = {t - 63 for t in pos_live if 190 <= t <= 197}
        assert 127 in lo and 128 in lo, "the window's first key crosses 127 / 128 inside one slot's rows"
        assert -(-X.P_DRAFT // 128) == 3, "three chunks"
