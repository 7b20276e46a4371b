"""numpy restatement of the engine's FP8 K / V cache (include/rk_engine.h at rk_llama_set_kv_fp8; DESIGN.md section 3 "FP8 K/V
cache"), for the tests that hold the engine's quantiser, its step kernels and the model on such a cache against it.

The format is tests/_fp8_ref.py's with ONE vector of 128 as the group: per key or value vector of one (cache row, kv head, position)
an int8 exponent - the smallest e with absmax <= 448 * 2^e, clamped to [-15, 7], all-zero: -15 - and per value one e4m3fn byte,
x * 2^-e rounded to nearest even, saturating at +-448; the dequantised value q * 2^e is an fp16 number.

Three layers, each on the one below:
  quantize_vectors / cache_layout   the format and the byte layout of one layer's cache
  step_reference / step_judge       tests/_attn_ref.py's kind-5 problem (fp64 single-token attention) over a dequantised cache with the
                                    row's own key and value rounded through the format
  Kv8Oracle                         a family oracle (tests/_qwen2_ref.py's way: a subclass in tests/) whose decoding steps read such a
                                    cache: plain prefill over the prompt, then one row per step
Every layer takes `mut`, one broken rule (MUTANTS) - what tests/test_kv8_host.py shows the bounds of the GPU tests to catch.
Nothing here imports the engine."""
import numpy as np

import _attn_ref as A
import _fp8_ref as F
from oracle.llama_numpy import rmsnorm, rope_tables, rotate_half

f16, f32, f64 = np.float16, np.float32, np.float64
VEC = 128
MUTANTS = ("exp_plus1", "shared_heads", "own_unrounded", "k_exp_on_v", "rtz")


# ---- the format ------------------------------------------------------------------------------------------------------------------
def _encode_rtz(x):
    """e4m3fn bytes by truncation toward zero (the mutant `rtz`): the largest representable magnitude not above |x|"""
    x = np.asarray(x, dtype=f64)
    b = F.encode_e4m3fn(x)
    over = np.abs(F.decode_e4m3fn(b)) > np.abs(x)
    return np.where(over, b - 1, b).astype(np.uint8)          # magnitudes are ordered like their encodings; `over` implies magnitude > 0


def quantize_vectors(x16, mut=None):
    """[..., 128] fp16 -> (bytes uint8 [..., 128], exponents int8 [...], dequantised fp16 [..., 128]).  mut "rtz": truncated bytes."""
    x16 = np.asarray(x16, dtype=f16)
    shape = x16.shape
    assert shape[-1] == VEC
    flat = x16.reshape(-1, VEC)
    e = F.group_exponents(flat)[:, 0].astype(np.int64)
    enc = _encode_rtz if mut == "rtz" else F.encode_e4m3fn
    q = enc(np.ldexp(flat.astype(f64), -e[:, None]))
    d = np.ldexp(F.decode_e4m3fn(q), e[:, None])
    d16 = d.astype(f16)
    assert (d16.astype(f64) == d).all(), "a dequantised value is not an fp16 number"
    return q.reshape(shape), e.astype(np.int8).reshape(shape[:-1]), d16.reshape(shape)


def dequantize_vectors(q, e):
    q = np.asarray(q, dtype=np.uint8)
    return np.ldexp(F.decode_e4m3fn(q), np.asarray(e).astype(np.int64)[..., None]).astype(f16)


def quantize_cache(kc16, vc16, mut=None):
    """K and V planes [rows, n_kv, P, 128] fp16 -> ((kq, ke, kd), (vq, ve, vd)): what the writers leave and what a reader makes of it.
    The bytes and exponents are the format's (`rtz`: truncated bytes); the other cache-level mutants break the READER - kd / vd are
    what it would hand the attention: `exp_plus1` (every exponent read one too high), `shared_heads` (every kv head of a position
    read with head 0's exponent: a plane [rows][P'] where the layout has [rows][n_kv][P']), `k_exp_on_v` (V read with K's plane)."""
    K, V = quantize_vectors(kc16, mut), quantize_vectors(vc16, mut)
    ke, ve = K[1].astype(np.int64), V[1].astype(np.int64)
    if mut == "exp_plus1":
        ke, ve = ke + 1, ve + 1
    elif mut == "shared_heads":
        ke, ve = np.broadcast_to(ke[:, :1], ke.shape), np.broadcast_to(ve[:, :1], ve.shape)
    elif mut == "k_exp_on_v":
        ve = ke
    else:
        return K, V
    rd = lambda q, e: A.f16_sat(np.ldexp(F.decode_e4m3fn(q), e[..., None]))
    return (K[0], K[1], rd(K[0], ke)), (V[0], V[1], rd(V[0], ve))


def pad32(P):
    return (int(P) + 31) & ~31


def cache_layout(K, V, P):
    """One layer's cache as the engine lays it out, as bytes: K bytes [rows][n_kv][P][128] | V bytes | K exponents [rows][n_kv][P'] | V
    exponents, P' = P rounded up to 32 (the pad bytes 0 here: compare through `layout_views`)."""
    (kq, ke, _), (vq, ve, _) = K, V
    pe = pad32(P)
    out = [kq.reshape(-1), vq.reshape(-1)]
    for e in (ke, ve):
        pl = np.zeros(e.shape[:-1] + (pe,), dtype=np.int8)
        pl[..., :P] = e
        out.append(pl.reshape(-1).view(np.uint8))
    return np.concatenate(out)


def layer_bytes(rows, n_kv, P):
    return 2 * rows * n_kv * P * VEC + 2 * rows * n_kv * pad32(P)


def layout_views(raw, rows, n_kv, P):
    """bytes of one layer -> (kq, vq [rows, n_kv, P, 128] uint8, ke, ve [rows, n_kv, P] int8: the pad behind P cut off)"""
    raw = np.asarray(raw, dtype=np.uint8).reshape(-1)
    plane, pe = rows * n_kv * P * VEC, pad32(P)
    assert raw.size == layer_bytes(rows, n_kv, P)
    kq, vq = raw[:plane].reshape(rows, n_kv, P, VEC), raw[plane:2 * plane].reshape(rows, n_kv, P, VEC)
    ex = raw[2 * plane:].view(np.int8).reshape(2, rows, n_kv, pe)[..., :P]
    return kq, vq, ex[0], ex[1]


def adversarial_vectors(seed=5, n_random=200):
    """fp16 [n, 128]: the format's edges - absmax exactly 448 * 2^e and one fp16 ulp above it for e over the range, the zero vector,
    the clamp at 7 with saturation, subnormal inputs at -15, exact rounding ties, a negative zero - then random vectors of many scales."""
    rs = np.random.RandomState(seed)
    rows = []
    for e in range(F.E_MIN, F.E_MAX + 1):
        for top in (f16(448.0 * 2.0 ** e), np.nextafter(f16(448.0 * 2.0 ** e), f16(np.inf))):
            v = (rs.standard_normal(VEC) * float(top) * 0.3).astype(f16)
            v = np.clip(v, -abs(float(top)), abs(float(top))).astype(f16)
            v[rs.randint(VEC)] = top if rs.rand() < 0.5 else -top
            rows.append(v)
    rows.append(np.zeros(VEC, f16))
    v = (rs.standard_normal(VEC) * 9000).astype(f16); v[3], v[77] = f16(60000.0), f16(-65504.0); rows.append(v)      # clamp at 7, saturation
    v = (rs.standard_normal(VEC) * 3e-8).astype(f16); v[5], v[6] = f16(1e-7), f16(-2.0 ** -24); rows.append(v)         # clamp at -15
    v = np.zeros(VEC, f16); v[:9] = np.array([448.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 447.0, -17.0, -2.0 ** -10, -0.0], f16); rows.append(v)
    v = np.zeros(VEC, f16); v[127] = f16(-448.0); rows.append(v)                                                      # the maximum in the last lane
    v = np.zeros(VEC, f16); v[64] = f16(2.0 ** -24); rows.append(v)
    for _ in range(n_random):
        rows.append((rs.standard_normal(VEC) * 10.0 ** rs.uniform(-6, 4)).astype(f16))
    return np.stack(rows)


# ---- the step's attention: _attn_ref's kind 5 over a dequantised cache -----------------------------------------------------------------
def step_new16(p, qk=None):
    """The new key and value of every (row, kv head) as the fp16 cache would hold them, from the documented fp32 arithmetic
    ([n_seq, n_kv, 128] each) - what a test without the device takes for `new16`; with the device it reads the fp16 kind-5 entry's
    cache instead."""
    G = p.H // p.n_kv
    if qk is not None:
        import _qwen3_ref as Q3
        its = Q3.qkn_step_items(p, emul=True)
    else:
        its = A.items(p, emul=True)
    k = np.stack([its[b * p.H + g * G]["new"][3] for b in range(p.n_seq) for g in range(p.n_kv)]).reshape(p.n_seq, p.n_kv, VEC)
    v = np.stack([its[b * p.H + g * G]["new"][4] for b in range(p.n_seq) for g in range(p.n_kv)]).reshape(p.n_seq, p.n_kv, VEC)
    return k.astype(f16), v.astype(f16)


def step_reference(p, new16, mut=None, window=0, qk=False, g1=1):
    """The pieces of a kind-5 problem `p` (A.build_step / _qwen3_ref.build_qkn_step) on an FP8 cache: per (row, head) the fp64 and the
    emulation's query, and as keys / values the DEQUANTISED cache rows lo .. pos - 1 and the row's own key and value rounded through
    the format (`own_unrounded`: left as the fp16 values), lo = max(0, pos - window + 1).  new16 = (k16, v16) [n_seq, n_kv, 128].
    g1 > 1 (the KEYS form): row b reads cache row b // g1 and every key <= pos is in the cache already - new16 is not used.
    Returns (ref items, emulation items, the cache after the step: ((kq, ke, kd), (vq, ve, vd)))."""
    rows = p.n_seq // g1
    half = rows * p.n_kv * p.P * VEC
    c = np.asarray(p.cache).reshape(-1)
    kc16, vc16 = c[:half].reshape(rows, p.n_kv, p.P, VEC).copy(), c[half:].reshape(rows, p.n_kv, p.P, VEC).copy()
    if g1 == 1:
        for b in range(p.n_seq):
            kc16[b, :, int(p.pos[b])], vc16[b, :, int(p.pos[b])] = new16[0][b], new16[1][b]
    K, V = quantize_cache(kc16, vc16, mut)
    kd, vd = K[2].copy(), V[2].copy()
    if mut == "own_unrounded" and g1 == 1:
        for b in range(p.n_seq):
            kd[b, :, int(p.pos[b])], vd[b, :, int(p.pos[b])] = new16[0][b], new16[1][b]
    if qk:
        import _qwen3_ref as Q3
        base = {False: Q3.qkn_step_items(p), True: Q3.qkn_step_items(p, emul=True)}
    else:
        base = {False: A.items(p), True: A.items(p, emul=True)}
    G = p.H // p.n_kv
    out = {}
    for emul, its in base.items():
        lst = []
        for it in its:
            b, h = int(it["out_rows"][0]), it["out_col"] // VEC
            pos, g = int(p.pos[b]), h // G
            lo = max(0, pos - window + 1) if window > 0 else 0
            dt = f16 if emul else f64
            lst.append(dict(it, k=kd[b // g1, g, lo:pos + 1].astype(dt), v=vd[b // g1, g, lo:pos + 1].astype(dt)))
        out[emul] = lst
    return out[False], out[True], (K, V)


def step_judge(ref, em, got, what=""):
    """_attn_ref.judge's rule (tests/_qwen3_ref.py: qkn_step_judge's form of it) on the step's context rows [n_seq, H 128] fp16: half an
    fp16 ulp of the fp64 value + A.C x E, E = the chain emulation's largest error against fp64 over the problem's pieces."""
    got = np.asarray(got)
    assert got.dtype == f16 and np.isfinite(got.astype(f64)).all(), what
    want = [A.attend64(it) for it in ref]
    E = max(float(np.abs(A.emulate_item(e).astype(f64) - w).max()) for e, w in zip(em, want))
    worst = 0.0
    for it, w in zip(ref, want):
        g = got[it["out_rows"], it["out_col"]:it["out_col"] + VEC].astype(f64)
        over = np.abs(g - w) - A.half_ulp16(w)
        worst = max(worst, float(over.max()) / E if E > 0 else (0.0 if over.max() <= 0 else np.inf))   # (E = 0: one key, the context IS its value)
        assert (over <= A.C * E).all(), f"{what}: row {it['out_rows'][0]}, head column {it['out_col']}: off by {float(over.max()):.3g} beyond half an ulp, {A.C} x E = {A.C * E:.3g}"
    return worst


def merge_partials(part, n_seq, H, nch, pos, window=0):
    """The chunk partials [n_seq][H][nch][132] fp32 of a step merged in fp64 -> context [n_seq, H 128] (chunks lo // 128 .. pos // 128)"""
    part = np.asarray(part, dtype=f32).reshape(n_seq, H, nch, VEC + 4).astype(f64)
    out = np.zeros((n_seq, H * VEC))
    for b in range(n_seq):
        lo = max(0, int(pos[b]) - window + 1) if window > 0 else 0
        ch = np.arange(lo // 128, int(pos[b]) // 128 + 1)
        for h in range(H):
            m, l, a = part[b, h, ch, VEC], part[b, h, ch, VEC + 1], part[b, h, ch, :VEC]
            w = np.exp2(m - m.max())
            out[b, h * VEC:(h + 1) * VEC] = (w[:, None] * a).sum(axis=0) / (w * l).sum()
    return out


# ---- the model on an FP8 cache ------------------------------------------------------------------------------------------------------
class _Kv8Steps:
    """Mixed into a family oracle (LlamaOracle, Qwen2Oracle, MistralOracle, Qwen3Oracle: `_lin` carries the family's bias or head
    norm, dims.sliding_window the window): the prompt's plain prefill in the oracle's fp32, every layer's rotated keys and its values
    kept; then one row per step over the cache.  kv8: the cache holds each vector rounded to fp16 and through the format, the step's
    own key and value included; kv8 = False: the fp32 vectors as they are - the plain oracle in another order of evaluation."""
    mut = None

    def _layer_qkv(self, x, p, pos):
        d = self.d
        n = x.shape[0]
        cos, sin = rope_tables(int(np.max(pos)) + 1, d.head_dim, d.rope_theta, getattr(d, "rope_scaling", None))
        cos, sin = cos[np.asarray(pos)], sin[np.asarray(pos)]
        q = self._lin(x, p + ".self_attn.q_proj.weight").reshape(n, d.n_heads, d.head_dim).transpose(1, 0, 2)
        k = self._lin(x, p + ".self_attn.k_proj.weight").reshape(n, d.n_kv_heads, d.head_dim).transpose(1, 0, 2)
        v = self._lin(x, p + ".self_attn.v_proj.weight").reshape(n, d.n_kv_heads, d.head_dim).transpose(1, 0, 2)
        return q * cos[None] + rotate_half(q) * sin[None], k * cos[None] + rotate_half(k) * sin[None], v

    def _attend(self, q, k, v, qpos):
        """q [H, n, hd] at positions qpos, k / v [n_kv, L, hd] at positions 0 .. L - 1: causal, windowed by the dims"""
        d = self.d
        W = int(getattr(d, "sliding_window", 0) or 0)
        rep = d.n_heads // d.n_kv_heads
        i, j = np.asarray(qpos)[:, None], np.arange(k.shape[1])[None, :]
        hidden = (j > i) | ((j <= i - W) if W > 0 else False)
        mask = np.where(hidden, f32(np.finfo(f32).min), f32(0.0))
        s = (q @ np.repeat(k, rep, axis=0).transpose(0, 2, 1)) * f32(d.head_dim ** -0.5) + mask[None]
        s = s - s.max(axis=-1, keepdims=True)
        pr = np.exp(s)
        pr = pr / pr.sum(axis=-1, keepdims=True)
        return (pr @ np.repeat(v, rep, axis=0)).transpose(1, 0, 2).reshape(q.shape[1], d.n_heads * d.head_dim)

    def _mlp(self, h, p):
        x = rmsnorm(h, self.w[p + ".post_attention_layernorm.weight"], self.d.eps)
        g = self._lin(x, p + ".mlp.gate_proj.weight")
        return h + self._lin((g / (1.0 + np.exp(-g))) * self._lin(x, p + ".mlp.up_proj.weight"), p + ".mlp.down_proj.weight")

    def _store(self, k, v, kv8):
        """what the cache gives back for these fp32 vectors [n_kv, n, hd]"""
        if not kv8:
            return k.astype(f32), v.astype(f32)
        K, V = quantize_cache(A.f16_sat(k)[None], A.f16_sat(v)[None], None if self.mut == "own_unrounded" else self.mut)
        return K[2][0].astype(f32), V[2][0].astype(f32)

    def step_logits(self, prompt, fed, kv8=True):
        """Logits [len(fed), V] of the decoding steps that feed the tokens `fed` behind `prompt`: step j runs at position
        len(prompt) + j over the cache of the prompt and of the steps before it."""
        d = self.d
        L = len(prompt)
        head = self.w["model.embed_tokens.weight"] if d.tied_head else self.w["lm_head.weight"]
        h = self.w["model.embed_tokens.weight"][np.asarray(prompt, dtype=np.int64)]
        cache = []
        for i in range(d.n_layers):                          # the plain prefill: un-quantised attention, the cache filled behind it
            p = f"model.layers.{i}"
            q, k, v = self._layer_qkv(rmsnorm(h, self.w[p + ".input_layernorm.weight"], d.eps), p, np.arange(L))
            h = self._mlp(h + self._lin(self._attend(q, k, v, np.arange(L)), p + ".self_attn.o_proj.weight"), p)
            cache.append(list(self._store(k, v, kv8)))
        out = []
        for j, tok in enumerate(fed):
            pos = np.array([L + j])
            h = self.w["model.embed_tokens.weight"][np.asarray([tok], dtype=np.int64)]
            for i in range(d.n_layers):
                p = f"model.layers.{i}"
                q, k, v = self._layer_qkv(rmsnorm(h, self.w[p + ".input_layernorm.weight"], d.eps), p, pos)
                kd, vd = self._store(k, v, kv8)
                if kv8 and self.mut == "own_unrounded":      # the row reads its own key un-rounded; the cache keeps the rounded one
                    ko, vo = A.f16_sat(k).astype(f32), A.f16_sat(v).astype(f32)
                else:
                    ko, vo = kd, vd
                ctx = self._attend(q, np.concatenate([cache[i][0], ko], axis=1), np.concatenate([cache[i][1], vo], axis=1), pos)
                cache[i] = [np.concatenate([cache[i][0], kd], axis=1), np.concatenate([cache[i][1], vd], axis=1)]
                h = self._mlp(h + self._lin(ctx, p + ".self_attn.o_proj.weight"), p)
            out.append(rmsnorm(h, self.w["model.norm.weight"], d.eps)[0] @ head.T)
        return np.stack(out).astype(f32)

    def greedy_steps(self, prompt, max_new, kv8=True):
        """max_new greedy tokens: column 0 from the prefill (the plain oracle's), the others from steps -> (tokens, the last step's logits)"""
        toks = [int(np.argmax(self.last_logits([list(prompt)])[0]))]
        lg = None
        for _ in range(max_new - 1):
            lg = self.step_logits(prompt, toks, kv8)[-1]
            toks.append(int(np.argmax(lg)))
        return toks, lg


def families():
    """name -> (dims, family oracle class): the toy models of the GPU tests (toy-mistral: a window of 64)"""
    from llmrankers import _synth
    from oracle.llama_numpy import LlamaOracle
    from _mistral_ref import MistralOracle
    from _qwen2_ref import Qwen2Oracle
    from _qwen3_ref import Qwen3Oracle
    return {"toy-llama": (_synth.TOY_LLAMA, LlamaOracle), "toy-qwen2": (_synth.TOY_QWEN2, Qwen2Oracle),
            "toy-mistral": (_synth.TOY_MISTRAL, MistralOracle), "toy-qwen3": (_synth.TOY_QWEN3, Qwen3Oracle)}


SYNTH_SEED = 929
CHECK5 = dict(prompt_len=125, token_seed=31, max_new=6)       # the inputs of the GPU test's check against the independent reference
LOGIT_BOUND = 4e-3                                            # x logit scale: what tests/test_gpu_llama_listwise.py holds the fp16 step to


def check5_prompt(dims):
    from llmrankers import _synth
    return list(_synth.synth_token_batch(1, CHECK5["prompt_len"], CHECK5["prompt_len"], dims.vocab, seed=CHECK5["token_seed"])[0])


def check5_reference(base_cls, dims, state, prompt, fed):
    """(Kv8Oracle's logits of the last step that feeds `fed` behind `prompt`, the plain oracle's, the logit scale, D_ref, the bound)"""
    lg8 = Kv8Oracle(base_cls, dims, state).step_logits(prompt, fed)[-1]
    plain = base_cls(dims, state).last_logits([list(prompt) + [int(t) for t in fed]])[0]
    scale, d_ref = float(np.abs(plain).max()), float(np.abs(lg8 - plain).max())
    return lg8, plain, scale, d_ref, LOGIT_BOUND * scale + d_ref


def Kv8Oracle(base_cls, dims, state, mut=None):
    """`base_cls` (a family oracle) with the FP8-cache steps: an instance of a subclass made here, like Qwen2Oracle a class in tests/"""
    assert mut is None or mut in MUTANTS
    cls = type("Kv8" + base_cls.__name__, (_Kv8Steps, base_cls), {"mut": mut})
    return cls(dims, state)
