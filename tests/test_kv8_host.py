"""The FP8 K / V cache without a device (rk_llama_set_kv_fp8; DESIGN.md section 3 "FP8 K/V cache"): the format of tests/_kv8_ref.py at
its edges, what the bounds of tests/test_gpu_kv8.py are worth against the reference's mutants, and the plumbing from the command
line down to the engine's setter on stub engines."""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

import _attn_ref as A
import _fp8_ref as F
import _kv8_ref as K
from conftest import GOLD, REPO
from llmrankers import _synth

f16, f64 = np.float16, np.float64


# ---- the format ------------------------------------------------------------------------------------------------------------------------
def test_format_at_its_edges():
    x = np.zeros((40, 128), f16)
    es = list(range(F.E_MIN, F.E_MAX + 1))
    for i, e in enumerate(es):                                       # absmax exactly 448 * 2^e keeps e, byte 0x7E; one fp16 ulp above takes e + 1
        x[i, 100] = f16(-448.0 * 2.0 ** e)
    q, ex, d = K.quantize_vectors(x[:len(es)])
    assert list(ex) == es and (q[:, 100] == 0xFE).all() and (d[:, 100] == x[:len(es), 100]).all()
    up = x[:len(es)].copy()
    up[:, 100] = np.nextafter(np.abs(up[:, 100]), f16(np.inf))
    q, ex, d = K.quantize_vectors(up)
    assert list(ex) == [min(e + 1, F.E_MAX) for e in es]
    assert q[-1, 100] == 0x7E                                         # at the clamp the value above 448 * 2^7 saturates
    # the zero vector; the clamp at 7 with saturation; subnormal inputs at -15
    q, ex, d = K.quantize_vectors(np.zeros((1, 128), f16))
    assert ex[0] == -15 and not q.any() and not d.any()
    v = np.zeros((1, 128), f16); v[0, :3] = [65504.0, -60000.0, 300.0]
    q, ex, d = K.quantize_vectors(v)
    assert ex[0] == 7 and list(q[0, :3]) == [0x7E, 0xFE, F.encode_e4m3fn(300.0 / 128)] and float(d[0, 0]) == 448.0 * 128 and float(d[0, 1]) == -448.0 * 128
    v = np.zeros((1, 128), f16); v[0, :4] = [2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 1e-7]
    q, ex, d = K.quantize_vectors(v)
    assert ex[0] == -15 and list(q[0, :3]) == [1, 0x81, 3] and [float(t) for t in d[0, :4]] == [2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 2 * 2.0 ** -24]
    # ties to even at e = 0, and the sign of a zero
    v = np.zeros((1, 128), f16); v[0, :9] = [448.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 447.0, -17.0, -2.0 ** -10, -0.0]
    q, ex, d = K.quantize_vectors(v)
    assert ex[0] == 0 and [float(t) for t in d[0, :8]] == [448.0, 16.0, 20.0, 0.0, 2.0 ** -8, 448.0, -16.0, -0.0]
    assert q[0, 7] == 0x80 and q[0, 8] == 0x80 and np.signbit(d[0, 8])


def test_dequantised_values_are_fp16_fixed_points_and_bytes_are_torchs():
    x = K.adversarial_vectors()
    q, ex, d = K.quantize_vectors(x)                                  # (asserts inside: q * 2^e is an fp16 number)
    assert ex.min() == F.E_MIN and ex.max() == F.E_MAX and q.max() <= 0xFE and not ((q & 0x7F) == 0x7F).any()
    q2, ex2, d2 = K.quantize_vectors(d)                               # a fixed point IN VALUE: a vector whose maximum rounded down may take a smaller exponent
    np.testing.assert_array_equal(d2.view(np.uint16), d.view(np.uint16))
    np.testing.assert_array_equal(K.dequantize_vectors(q, ex).view(np.uint16), d.view(np.uint16))
    scaled = np.ldexp(x.astype(f64), -ex.astype(np.int64)[:, None])
    inside = np.abs(scaled) <= F.FP8_MAX                              # torch does not saturate: compare where nothing saturates
    np.testing.assert_array_equal(q[inside], F.torch_bytes(scaled)[inside])
    err = np.abs(d.astype(f64) - x.astype(f64))                       # half an FP8 ulp of the vector's scale, or saturation at the clamp
    ok = (err <= np.maximum(np.abs(x.astype(f64)) * 2.0 ** -4, 2.0 ** (ex.astype(f64)[:, None] - 10))) | (ex[:, None] == F.E_MAX)
    assert ok.all()


def test_layout_and_size():
    rs = np.random.RandomState(3)
    for rows, n_kv, P in ((1, 2, 7), (3, 1, 129), (4, 2, 300)):
        kc, vc = (rs.standard_normal((rows, n_kv, P, 128)) * 3).astype(f16), rs.standard_normal((rows, n_kv, P, 128)).astype(f16)
        Kq, Vq = K.quantize_cache(kc, vc)
        raw = K.cache_layout(Kq, Vq, P)
        assert raw.size == K.layer_bytes(rows, n_kv, P) and K.pad32(P) % 32 == 0 and K.pad32(P) - P < 32
        kq, vq, ke, ve = K.layout_views(raw, rows, n_kv, P)
        np.testing.assert_array_equal(kq, Kq[0]); np.testing.assert_array_equal(vq, Vq[0])
        np.testing.assert_array_equal(ke, Kq[1]); np.testing.assert_array_equal(ve, Vq[1])
        plane = rows * n_kv * P * 128                                 # the four regions start on multiples of 32 bytes
        assert plane % 32 == 0 and (rows * n_kv * K.pad32(P)) % 32 == 0
    for P in (16, 120, 136, 300, 4096):                               # at most 0.52 x the fp16 cache from 16 positions on
        assert K.layer_bytes(5, 2, P) <= 0.52 * (4 * 5 * 2 * P * 128), P


# ---- what the GPU bounds are worth ----------------------------------------------------------------------------------------------------------
def test_oracle_steps_without_quantisation_are_the_plain_oracle():
    for name, (dims, base) in K.families().items():
        state = _synth.synth_state_dict(dims, seed=K.SYNTH_SEED)
        prompt = K.check5_prompt(dims)
        orc = K.Kv8Oracle(base, dims, state)
        toks, _ = orc.greedy_steps(prompt, 3, kv8=False)
        plain = base(dims, state).last_logits([prompt + toks[:2]])[0]
        got = orc.step_logits(prompt, toks[:2], kv8=False)[-1]
        assert np.abs(got - plain).max() <= 1e-5 * np.abs(plain).max(), name   # the same fp32 arithmetic in another order of evaluation


def test_mutants_against_the_bound_of_the_model_check():
    """GPU check 5 holds the engine's last-step logits to 4e-3 x logit scale + D_ref of Kv8Oracle's, D_ref = max |Kv8Oracle - plain
    oracle|.  Here every mutant of the reference stands in for the engine on that check's inputs (K.CHECK5, the tokens Kv8Oracle's own
    greedy steps feed).  Measured distance / bound (seed 929):
                      toy-llama  toy-qwen2  toy-mistral  toy-qwen3
      exp_plus1          63.2       55.1        37.0        34.1
      k_exp_on_v          7.6        8.2         7.3         4.0
      shared_heads       15.0        -           4.3         2.5      (toy-qwen2 has ONE kv head: the mutant is the format itself)
      rtz                 2.6        2.0         1.6         1.4      beyond the bound everywhere, by less than a factor of 2 on three
      own_unrounded      0.025      0.010       0.042       0.028     NOT caught here: one key in 126 moves by half an FP8 ulp
    own_unrounded is what the step-attention check catches (test_own_key_mutant_is_caught_by_the_step_check below); rtz and every
    other mutant are also caught byte for byte by the quantiser and cache checks.  The bound is not widened for any of them."""
    ratios = {}
    for name, (dims, base) in K.families().items():
        state = _synth.synth_state_dict(dims, seed=K.SYNTH_SEED)
        prompt = K.check5_prompt(dims)
        toks, _ = K.Kv8Oracle(base, dims, state).greedy_steps(prompt, K.CHECK5["max_new"])
        fed = toks[:-1]
        lg8, plain, scale, d_ref, bound = K.check5_reference(base, dims, state, prompt, fed)
        print(f"{name}: logit scale {scale:.3f}, D_ref {d_ref:.4f}, bound {bound:.4f}")
        assert 0 < d_ref < 0.05 * scale, name                          # the quantisation moves the logits, by a few percent of their scale at most
        for m in K.MUTANTS:
            d = float(np.abs(K.Kv8Oracle(base, dims, state, m).step_logits(prompt, fed)[-1] - lg8).max())
            ratios[name, m] = d / bound
            print(f"    {m:14s} distance {d:.4f} = {d / bound:.3f} x bound")
    for (name, m), r in ratios.items():
        if m == "own_unrounded":
            continue
        if m == "shared_heads" and K.families()[name][0].n_kv_heads == 1:
            assert r == 0.0
            continue
        assert r > 1.0, (name, m, r)
    assert all(ratios[n, m] > 2.0 for n in K.families() for m in ("exp_plus1", "k_exp_on_v"))


def test_own_key_mutant_is_caught_by_the_step_check():
    """the step-attention check (GPU check 2: _attn_ref's kind-5 rule against fp64 on the dequantised operands with the rounded own key)
    against a kernel that reads its own key and value un-rounded: at pos 0 the row's context IS its value vector"""
    p = A.build_step(11, 4, 2, [0, 1, 31], 40, "R")
    new16 = K.step_new16(p)
    ref, em, _ = K.step_reference(p, new16)
    mref, mem, _ = K.step_reference(p, new16, mut="own_unrounded")
    honest = np.zeros((p.n_seq, p.H * 128), f16)
    broken = honest.copy()
    for it, mit in zip(em, mem):
        honest[it["out_rows"], it["out_col"]:it["out_col"] + 128] = A.f16_sat(A.emulate_item(it))
        broken[it["out_rows"], it["out_col"]:it["out_col"] + 128] = A.f16_sat(A.emulate_item(mit))
    assert K.step_judge(ref, em, honest, "honest") <= A.C / 2
    with pytest.raises(AssertionError, match="row 0"):
        K.step_judge(ref, em, broken, "own key un-rounded")
    for m in ("exp_plus1", "shared_heads", "k_exp_on_v", "rtz"):      # and the others, on a row with cached keys
        mref, mem, _ = K.step_reference(p, new16, mut=m)
        for it, mit in zip(em, mem):
            broken[it["out_rows"], it["out_col"]:it["out_col"] + 128] = A.f16_sat(A.emulate_item(mit))
        with pytest.raises(AssertionError):
            K.step_judge(ref, em, broken, m)


# ---- plumbing: the binding ---------------------------------------------------------------------------------------------------------------
class _StubLib:
    """every rk_* entry returns RK_OK and is recorded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


def test_header_table_and_binding_agree(monkeypatch):
    from llmrankers import _engine
    header = open(os.path.join(REPO, "include", "rk_engine.h")).read()
    for proto in ("int rk_llama_set_kv_fp8(rk_engine* e, int on);", "int rk_debug_kv8_step(rk_engine* e, rk_debug_kv8_step_call* call);",
                  "int rk_debug_kv8_quant(rk_engine* e, const uint16_t* x, int n, uint8_t* q_out, int8_t* exp_out, uint16_t* deq_out);"):
        assert proto in header, proto
    for name in ("rk_llama_set_kv_fp8", "rk_debug_kv8_quant", "rk_debug_kv8_step"):
        assert name in _engine.ABI
    for kv in (False, True):
        lib = _StubLib()
        monkeypatch.setattr(_engine, "load_library", lambda lib=lib: lib)
        eng = _engine.RkLlamaEngine(_synth.TOY_QWEN2, device=0, max_tokens=64, max_seqs=2, **({"kv_fp8": True} if kv else {}))
        eng.load_state([("model.norm.weight", np.ones(4, np.float32))])
        names = [n for n, _ in lib.calls]
        assert names[0] == "rk_llama_create" and eng.kv_fp8 is kv
        assert [a[1] for n, a in lib.calls if n == "rk_llama_set_kv_fp8"] == ([1] if kv else [])
        if kv:                                                        # after create, before finalize
            assert names.index("rk_llama_set_kv_fp8") < names.index("rk_engine_finalize")
        eng.h = None
    lib = _StubLib()
    monkeypatch.setattr(_engine, "load_library", lambda lib=lib: lib)
    eng = _engine.RkLlamaEngine(_synth.TOY_LLAMA, device=0, max_tokens=64, max_seqs=2, kv_fp8=True)
    q, e, d = eng.debug_kv8_quant(np.zeros((5, 128), f16))
    assert (q.shape, e.shape, d.shape, q.dtype, e.dtype, d.dtype) == ((5, 128), (5,), (5, 128), np.uint8, np.int8, f16)
    assert lib.calls[-1][0] == "rk_debug_kv8_quant" and lib.calls[-1][1][2] == 5
    eng.h = None


def test_debug_step_struct_has_the_headers_layout(tmp_path):
    import ctypes as C
    import subprocess
    from llmrankers import _engine
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    fields = ["n_seq", "plan_only", "qk_eps", "qkv", "cache", "ctx", "part", "cache_out", "out_R", "out_pe"]
    src = tmp_path / "layout.c"
    src.write_text('#include "rk_engine.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n  printf("%zu\\n", sizeof(rk_debug_kv8_step_call));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(rk_debug_kv8_step_call, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    t = _engine.RkDebugKv8StepCall
    assert got == [C.sizeof(t)] + [getattr(t, f).offset for f in fields]


# ---- plumbing: runtime and rankers ----------------------------------------------------------------------------------------------------------
class _StubEngine:
    made = []

    def __init__(self, dims, device=0, max_tokens=16384, max_seqs=16, **kw):
        self.dims, self.loaded, self.kw = dims, 0, kw
        self.weight_fp8, self.kv_fp8 = bool(kw.get("weight_fp8")), bool(kw.get("kv_fp8"))
        self.desc = type("Desc", (), {"max_tokens": max_tokens, "max_seqs": max_seqs})
        _StubEngine.made.append(self)

    def load_state(self, tensors):
        self.loaded = sum(1 for _ in tensors)
        return self

    def close(self):
        pass


def _write(tmp_path, name, cfg, tok):
    from safetensors.numpy import save_file
    path = str(tmp_path / name)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({"model.norm.weight": np.ones(8, np.float32)}, os.path.join(path, "model.safetensors"))
    for fn in os.listdir(os.path.join(GOLD, tok)):
        shutil.copy(os.path.join(GOLD, tok, fn), os.path.join(path, fn))
    return path


def test_runtime_and_rankers_forward_kv_dtype(monkeypatch, tmp_path):
    from llmrankers import _runtime
    from llmrankers._runtime import LlamaRuntime, load_runtime
    from llmrankers.listwise import ListwiseLlmRanker, R1ListwiseLlmRanker
    from llmrankers.pairwise import DuoT5LlmRanker, PairwiseLlmRanker
    from llmrankers.pointwise import MonoT5LlmRanker, PointwiseLlmRanker
    from llmrankers.setwise import RankR1SetwiseLlmRanker, SetwiseLlmRanker
    from test_mistral_host import PROMPT
    monkeypatch.setattr(_runtime, "RkLlamaEngine", _StubEngine)
    del _StubEngine.made[:]
    path = _write(tmp_path, "toy-llama", _synth.TOY_LLAMA.to_hf_config(), "tok_llama")
    assert LlamaRuntime(path, "cuda").kv_dtype == "fp16" and _StubEngine.made[-1].kw == {}
    assert LlamaRuntime(path, "cuda", kv_dtype="fp16").engine.kw == {}
    rt = LlamaRuntime(path, "cuda", kv_dtype="fp8")
    assert rt.kv_dtype == "fp8" and rt.weight_dtype == "fp16" and rt.engine.kw == {"kv_fp8": True}
    assert LlamaRuntime.from_engine(rt.engine).kv_dtype == "fp8"
    assert LlamaRuntime(path, "cuda", kv_dtype="fp8", weight_dtype="fp8").engine.kw == {"weight_fp8": True, "kv_fp8": True}
    assert load_runtime(path, "cuda", kv_dtype="fp8").engine.kw == {"kv_fp8": True}
    n = len(_StubEngine.made)
    for bad in ("fp4", "bf16", None, 8):
        with pytest.raises(ValueError, match="kv_dtype"):
            LlamaRuntime(path, "cuda", kv_dtype=bad)
        with pytest.raises(ValueError, match="kv_dtype"):
            SetwiseLlmRanker.with_kv_dtype(bad)
    assert len(_StubEngine.made) == n
    path64 = _write(tmp_path, "toy-llama-hd64", _synth.TOY_LLAMA_HD64.to_hf_config(), "tok_llama")
    with pytest.raises(NotImplementedError, match="kv_dtype='fp8' with head_dim 64"):
        LlamaRuntime(path64, "cuda", kv_dtype="fp8")
    assert len(_StubEngine.made) == n
    tokdir, r1 = os.path.join(GOLD, "tok_qwen"), os.path.join(GOLD, "rankr1_prompt.toml")
    # exactly the classes that take weight_dtype = "fp8" take kv_dtype = "fp8": the option is the class's
    builds = {
        SetwiseLlmRanker: lambda c, **kw: c(path, path, "cuda", **kw),
        PairwiseLlmRanker: lambda c, **kw: c(path, path, "cuda", method="heapsort", **kw),
        ListwiseLlmRanker: lambda c, **kw: c(path, path, "cuda", 4, 2, **kw),
        RankR1SetwiseLlmRanker: lambda c, **kw: c(path, r1, tokenizer_name_or_path=tokdir),
        R1ListwiseLlmRanker: lambda c, **kw: c(path, tokdir, PROMPT, 4, 2),
    }
    for cls, build in builds.items():
        assert cls.kv_dtype == "fp16" and cls.with_kv_dtype("fp16") is cls
        assert build(cls).llm.engine.kw == {}, cls
        c8 = cls.with_kv_dtype("fp8")
        assert issubclass(c8, cls) and c8.__name__ == cls.__name__ and c8 is cls.with_kv_dtype("fp8") and cls.kv_dtype == "fp16"
        assert build(c8).llm.engine.kw == {"kv_fp8": True}, cls
    assert builds[SetwiseLlmRanker](SetwiseLlmRanker.with_kv_dtype("fp8"), weight_dtype="fp8").llm.engine.kw == {"weight_fp8": True, "kv_fp8": True}
    both = RankR1SetwiseLlmRanker.with_weight_dtype("fp8").with_kv_dtype("fp8").with_draft_tokens(3)
    assert (both.weight_dtype, both.kv_dtype, both.draft_tokens) == ("fp8", "fp8", 3)
    assert builds[RankR1SetwiseLlmRanker](both).llm.engine.kw == {"weight_fp8": True, "kv_fp8": True}
    # the classes that refuse weight_dtype = "fp8" refuse kv_dtype = "fp8": duoT5 by name, the pointwise rankers have no such option
    with pytest.raises(NotImplementedError, match="kv_dtype='fp8' is not supported for T5 checkpoints"):
        DuoT5LlmRanker.with_kv_dtype("fp8")
    assert DuoT5LlmRanker.with_kv_dtype("fp16") is DuoT5LlmRanker
    for cls in (PointwiseLlmRanker, MonoT5LlmRanker):
        assert not hasattr(cls, "with_kv_dtype") and not hasattr(cls, "with_weight_dtype")


def test_t5_checkpoints_refuse_kv_fp8_by_name(monkeypatch, tmp_path):
    from llmrankers import _runtime
    from llmrankers._runtime import load_runtime
    from llmrankers.setwise import SetwiseLlmRanker
    made = []
    monkeypatch.setattr(_runtime, "T5Runtime", lambda *a, **kw: made.append(kw) or "t5")
    path = str(tmp_path / "t5")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "t5"}, f)
    assert load_runtime(path, "cuda", kv_dtype="fp16") == "t5" and made == [{"cache_dir": None}]
    with pytest.raises(NotImplementedError, match="kv_dtype='fp8'"):
        load_runtime(path, "cuda", kv_dtype="fp8")
    with pytest.raises(NotImplementedError, match="kv_dtype='fp8'.*setwise"):
        SetwiseLlmRanker.with_kv_dtype("fp8")(path, path, "cuda")
    with pytest.raises(ValueError, match="kv_dtype"):
        load_runtime(path, "cuda", kv_dtype="int8")
    assert len(made) == 1


# ---- plumbing: the command line --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runmod():
    spec = importlib.util.spec_from_file_location("rk_run_kv8", os.path.join(REPO, "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_passes_kv_dtype_only_when_asked(runmod, monkeypatch):
    import llmrankers.listwise as lw
    import llmrankers.pairwise as pw
    import llmrankers.setwise as sw
    made = {}

    class Stub:
        weight_dtype, kv_dtype, draft_tokens, asked = "fp16", "fp16", 0, ()

        def __init__(self, **kw):
            made.clear()
            made.update(kw, cls=type(self))

        @classmethod
        def _with(cls, **kw):
            return type(cls.__name__, (cls,), dict(kw, asked=cls.asked + tuple(kw)))

        @classmethod
        def with_weight_dtype(cls, wd):
            return cls._with(weight_dtype=wd)

        @classmethod
        def with_kv_dtype(cls, kd):
            return cls._with(kv_dtype=kd)

        @classmethod
        def with_draft_tokens(cls, n):
            return cls._with(draft_tokens=n)

    stubs = {}
    for mod, names in ((sw, ("SetwiseLlmRanker", "RankR1SetwiseLlmRanker")), (pw, ("PairwiseLlmRanker", "DuoT5LlmRanker")),
                       (lw, ("ListwiseLlmRanker", "R1ListwiseLlmRanker"))):
        for n in names:
            stubs[n] = type(n, (Stub,), {})
            monkeypatch.setattr(mod, n, stubs[n])
    parser, commands = runmod.build_parser()
    head = ["run", "--model_name_or_path", "m"]
    cases = {"SetwiseLlmRanker": (head, ["setwise"]), "PairwiseLlmRanker": (head, ["pairwise"]),
             "ListwiseLlmRanker": (head, ["listwise"]), "RankR1SetwiseLlmRanker": (head + ["--prompt_file", "p.toml"], ["setwise"]),
             "R1ListwiseLlmRanker": (head + ["--prompt_file", "p.toml"], ["listwise"])}
    for name, (run_args, tail) in cases.items():
        a = runmod.parse_args(parser, commands, run_args + tail)
        assert a.run.kv_dtype is None
        runmod.build_ranker(a)
        assert made["cls"] is stubs[name] and "kv_dtype" not in made, name      # without the flag: the class and the call as ever
        for kd in ("fp8", "fp16"):
            runmod.build_ranker(runmod.parse_args(parser, commands, run_args + ["--kv_dtype", kd] + tail))
            assert issubclass(made["cls"], stubs[name]) and made["cls"].kv_dtype == kd and made["cls"].asked == ("kv_dtype",) and "kv_dtype" not in made, name
    # it combines with --weight_dtype, --draft_tokens and --sample_seed
    runmod.build_ranker(runmod.parse_args(parser, commands, head + ["--prompt_file", "p.toml", "--kv_dtype", "fp8", "--weight_dtype", "fp8", "--draft_tokens", "3", "setwise"]))
    assert (made["cls"].weight_dtype, made["cls"].kv_dtype, made["cls"].draft_tokens) == ("fp8", "fp8", 3)
    runmod.build_ranker(runmod.parse_args(parser, commands, head + ["--kv_dtype", "fp8", "--weight_dtype", "fp8", "listwise", "--sample_seed", "5"]))
    assert made["cls"].kv_dtype == "fp8" and made["weight_dtype"] == "fp8" and made["sample_seed"] == 5
    with pytest.raises(SystemExit):
        runmod.parse_args(parser, commands, head + ["--kv_dtype", "int8", "setwise"])
    # the rankers that refuse --weight_dtype fp8 refuse --kv_dtype fp8 by name; fp16 changes nothing
    for run_args, tail in ((head, ["pointwise"]), (["run", "--model_name_or_path", "castorini/duot5-base-msmarco"], ["pairwise"])):
        with pytest.raises(NotImplementedError, match="kv_dtype fp8"):
            runmod.build_ranker(runmod.parse_args(parser, commands, run_args + ["--kv_dtype", "fp8"] + tail))
    runmod.build_ranker(runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "castorini/duot5-base-msmarco", "--kv_dtype", "fp16", "pairwise"]))
    assert made["cls"] is stubs["DuoT5LlmRanker"]
