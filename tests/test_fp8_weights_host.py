"""FP8 step weights, host side (no GPU): the properties of the format as tests/_fp8_ref.py restates it - what the GPU tests hold the
engine's quantiser and FP8 kernel against - and the plumbing from the command line down to the C ABI call."""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

import _fp8_ref as F
from conftest import GOLD
from llmrankers import _synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrices():
    rs = np.random.RandomState(11)
    yield "adversarial", F.adversarial_matrix()
    yield "normal", (rs.standard_normal((40, 528)) * 0.03).astype(np.float16)
    yield "heavy tails", (rs.standard_cauchy((33, 400)) * 0.5).clip(-6e4, 6e4).astype(np.float16)
    yield "subnormal", (rs.standard_normal((16, 144)) * 3e-7).astype(np.float16)
    yield "huge", (rs.standard_normal((16, 256)) * 2e4).clip(-65504, 65504).astype(np.float16)


# ---- the byte conversion ---------------------------------------------------------------------------------------------------------
def test_byte_conversion_against_torch_and_by_hand():
    """every fp16 number of magnitude <= 448 (torch.float8_e4m3fn on the CPU does not saturate beyond), the ties, the decode"""
    import torch
    assert hasattr(torch, "float8_e4m3fn")
    allf16 = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    x = allf16[np.isfinite(allf16) & (np.abs(allf16.astype(np.float64)) <= 448.0)].astype(np.float64)
    np.testing.assert_array_equal(F.encode_e4m3fn(x), F.torch_bytes(x))
    for v, want in ((447.0, 448.0), (17.0, 16.0), (19.0, 20.0), (0.001, 2.0 ** -9), (2.0 ** -10, 0.0), (3 * 2.0 ** -10, 2.0 ** -8),
                    (1e9, 448.0), (-1e9, -448.0), (464.0, 448.0), (2.0 ** -6, 2.0 ** -6), (0.0, 0.0)):
        assert float(F.decode_e4m3fn(F.encode_e4m3fn(np.array([v])))[0]) == want, v
    assert F.encode_e4m3fn(np.array([-0.0]))[0] == 0x80 and F.encode_e4m3fn(np.array([448.0]))[0] == 0x7E
    codes = np.array([b for b in range(256) if b & 0x7F != 0x7F], dtype=np.uint8)                 # all but the two NaN encodings
    np.testing.assert_array_equal(F.encode_e4m3fn(F.decode_e4m3fn(codes)), codes)
    t = torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    np.testing.assert_array_equal(F.decode_e4m3fn(codes), t)


# ---- the format's properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w", list(_matrices()), ids=[n for n, _ in _matrices()])
def test_dequantised_weights_are_fp16_numbers_and_a_fixed_point(name, w):
    """np.float16(d) == d everywhere (quantize asserts it on the way; here once more from the parts), and quantising the dequantised
    matrix returns the same VALUES.  Its bytes and exponents are the same too wherever the group's largest weight did not round down
    onto 448 * 2^(e - 1) - e4m3 steps by 16 between 128 and 256, so an absmax in (224, 232) x 2^e becomes 224 x 2^e = 448 x 2^(e - 1)
    and the group then takes exponent e - 1 with every byte one binade up: another spelling of the same numbers."""
    q, e, d = F.quantize(w)
    e_k = np.repeat(e.astype(np.int64), F.GROUP, axis=1)[:, :w.shape[1]]
    exact = np.ldexp(F.decode_e4m3fn(q), e_k)
    assert (np.float16(exact).astype(np.float64) == exact).all()
    assert d.tobytes() == np.float16(exact).tobytes() == F.dequantize(q, e).tobytes()
    q2, e2, d2 = F.quantize(d)
    assert d2.tobytes() == d.tobytes(), "the dequantised matrix is not a fixed point"
    n, k = w.shape
    g = e.shape[1]
    pad = np.zeros((n, g * F.GROUP))
    pad[:, :k] = np.abs(d.astype(np.float64))
    top = pad.reshape(n, g, F.GROUP).max(axis=2) / np.ldexp(1.0, e.astype(np.int64))             # the largest |q| of every group
    moved = (top <= 224.0) & (top > 0) & (e > F.E_MIN)
    same = np.repeat(~moved, F.GROUP, axis=1)[:, :k]
    assert (e2[~moved] == e[~moved]).all() and (q2[same] == q[same]).all()
    assert (e2[moved] == e[moved] - 1).all()
    if name == "normal":
        assert 0 < moved.sum() < 0.1 * moved.size, "the random matrix should hold a few such groups (8 of every 224 absmax values)"


@pytest.mark.parametrize("name,w", list(_matrices()), ids=[n for n, _ in _matrices()])
def test_one_e4m3_rounding_per_weight(name, w):
    """|d - w| <= 2^-4 |w| wherever the group's exponent is not clamped and w / 2^e is a normal e4m3 number (three mantissa bits:
    half a step of 2^-3 relative); below, the absolute step 2^-10 x 2^e; nothing moves by more than a weight's own size + a step"""
    q, e, d = F.quantize(w)
    w64, d64 = w.astype(np.float64), d.astype(np.float64)
    e_k = np.repeat(e.astype(np.int64), F.GROUP, axis=1)[:, :w.shape[1]]
    scaled = np.abs(np.ldexp(w64, -e_k))
    free = (e_k > F.E_MIN) & (e_k < F.E_MAX)
    normal = free & (scaled >= 2.0 ** -6)
    assert normal.any() or name in ("subnormal", "huge")
    assert (np.abs(d64 - w64)[normal] <= 2.0 ** -4 * np.abs(w64)[normal]).all()
    small = (e_k < F.E_MAX) & (scaled < 2.0 ** -6)
    assert (np.abs(d64 - w64)[small] <= np.ldexp(2.0 ** -10, e_k)[small]).all()
    assert (scaled[e_k < F.E_MAX] <= F.FP8_MAX).all(), "an unclamped group must fit 448 x 2^e"
    assert (np.sign(d64) * np.sign(w64) >= 0).all()


def test_exponent_rule_clamps_and_zero_groups():
    w = F.adversarial_matrix()
    q, e, d = F.quantize(w)
    assert e[1, 0] == F.E_MIN and (q[1, :128] == 0).all() and (d[1, :128] == 0).all()             # an all-zero group takes -15
    assert e[20, 3] == F.E_MIN and (q[20, 384:] == 0).all()                                       # the tail group of 16
    assert e[21, 3] == 0 and (q[21, 384:] == 0x7E).all()
    assert e[2, 1] == F.E_MAX and q[2, 130] == 0x7E and q[2, 131] == 0xFE                         # 60 000 / 128 and -65 504 / 128 saturate
    assert float(d[2, 130]) == 448.0 * 128 == 57344.0 and float(d[2, 131]) == -57344.0
    assert e[3, 2] == F.E_MIN                                                                     # absmax 1e-7: clamped at the bottom
    assert float(d[3, 261]) == -2.0 ** -24 and q[3, 261] == 0x81                                  # the smallest fp16 subnormal survives
    assert float(d[3, 260]) == 2 * 2.0 ** -24                                                     # 1e-7 = 1.68 x 2^-24 -> 2 x 2^-24
    # ties to even at e = 0
    assert [float(x) for x in d[4, :8]] == [448.0, 16.0, 20.0, 0.0, 2.0 ** -8, 448.0, -16.0, -0.0] and e[4, 0] == 0
    # the boundary: absmax = 448 x 2^e keeps e with the byte 0x7E, the next fp16 number takes e + 1
    for j, ex in enumerate((-15, -9, -3, 0, 4, 7)):
        assert e[5 + j, 1] == ex and q[5 + j, 128] == 0x7E and q[5 + j, 129] == 0xFE, ex
        assert e[12 + j, 1] == min(ex + 1, F.E_MAX), ex
    # the rule itself, by brute force over every fp16 magnitude
    mags = np.arange(1, 0x7C00, dtype=np.uint16).view(np.float16)
    got = F.group_exponents(mags.reshape(-1, 1))[:, 0].astype(np.int64)
    a = mags.astype(np.float64)
    fits = a[:, None] <= F.FP8_MAX * np.ldexp(1.0, np.arange(-40, 20))[None, :]
    want = np.clip(np.arange(-40, 20)[fits.argmax(axis=1)], F.E_MIN, F.E_MAX)
    np.testing.assert_array_equal(got, want)


# ---- plumbing: the binding ---------------------------------------------------------------------------------------------------------
class _StubLib:
    """every rk_* entry returns RK_OK and is recorded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


def test_header_library_table_and_binding_agree(monkeypatch):
    from llmrankers import _engine
    header = open(os.path.join(REPO, "include", "rk_engine.h")).read()
    for proto in ("int rk_llama_set_weight_fp8(rk_engine* e, int on);", "int rk_debug_gemm_fp8(rk_engine* e, rk_debug_gemm_call* call);",
                  "int rk_debug_quant_fp8(rk_engine* e, const uint16_t* W, int N, int K, int ldw, uint8_t* q_out, int8_t* exp_out, uint16_t* deq_out);"):
        assert proto in header, proto
    for name in ("rk_llama_set_weight_fp8", "rk_debug_gemm_fp8", "rk_debug_quant_fp8"):
        assert name in _engine.ABI
    assert len(_engine.ABI["rk_debug_quant_fp8"][1]) == 8
    for fp8 in (False, True):
        lib = _StubLib()
        monkeypatch.setattr(_engine, "load_library", lambda lib=lib: lib)
        eng = _engine.RkLlamaEngine(_synth.TOY_QWEN2, device=0, max_tokens=64, max_seqs=2, **({"weight_fp8": True} if fp8 else {}))
        eng.load_state([("model.norm.weight", np.ones(4, np.float32))])
        names = [n for n, _ in lib.calls]
        assert names[0] == "rk_llama_create" and eng.weight_fp8 is fp8
        assert [a[1] for n, a in lib.calls if n == "rk_llama_set_weight_fp8"] == ([1] if fp8 else [])
        if fp8:                                                     # after create, before the first tensor and before finalize
            assert names.index("rk_llama_set_weight_fp8") < names.index("rk_engine_load_tensor") < names.index("rk_engine_finalize")
        eng.h = None
    # the debug bindings reach their entries
    lib = _StubLib()
    monkeypatch.setattr(_engine, "load_library", lambda lib=lib: lib)
    eng = _engine.RkLlamaEngine(_synth.TOY_LLAMA, device=0, max_tokens=64, max_seqs=2)
    q, e, d = eng.debug_quant_fp8(np.zeros((6, 272), np.float16), K=256)
    assert (q.shape, e.shape, d.shape, q.dtype, e.dtype, d.dtype) == ((6, 256), (6, 2), (6, 256), np.uint8, np.int8, np.float16)
    name, args = lib.calls[-1]
    assert name == "rk_debug_quant_fp8" and tuple(args[2:5]) == (6, 256, 272)
    eng.debug_gemm_fp8(0, np.zeros((2, 64), np.float16), np.zeros((8, 64), np.float16), 2, 8, 64)
    assert lib.calls[-1][0] == "rk_debug_gemm_fp8"
    eng.debug_gemm_ex(0, 1, np.zeros((2, 64), np.float16), np.zeros((8, 64), np.float16), 2, 8, 64)
    assert lib.calls[-1][0] == "rk_debug_gemm_ex"
    eng.h = None


# ---- plumbing: runtime and rankers ---------------------------------------------------------------------------------------------------
class _StubEngine:
    made = []

    def __init__(self, dims, device=0, max_tokens=16384, max_seqs=16, **kw):
        self.dims, self.loaded, self.kw, self.weight_fp8 = dims, 0, kw, bool(kw.get("weight_fp8"))
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


def test_runtime_and_rankers_forward_weight_dtype(monkeypatch, tmp_path):
    import inspect
    from llmrankers import _runtime
    from llmrankers._runtime import LlamaRuntime, load_runtime
    from llmrankers.listwise import ListwiseLlmRanker, R1ListwiseLlmRanker
    from llmrankers.pairwise import PairwiseLlmRanker
    from llmrankers.setwise import RankR1SetwiseLlmRanker, SetwiseLlmRanker
    from test_mistral_host import PROMPT
    monkeypatch.setattr(_runtime, "RkLlamaEngine", _StubEngine)
    del _StubEngine.made[:]
    path = _write(tmp_path, "toy-llama", _synth.TOY_LLAMA.to_hf_config(), "tok_llama")
    assert list(inspect.signature(LlamaRuntime.__init__).parameters)[-1] == "weight_dtype"      # a trailing keyword
    for cls in (SetwiseLlmRanker, PairwiseLlmRanker, ListwiseLlmRanker):
        assert list(inspect.signature(cls.__init__).parameters)[-1] == "weight_dtype", cls
    # the default asks the engine for nothing new; "fp8" asks for weight_fp8; anything else is a ValueError before anything is read
    assert LlamaRuntime(path, "cuda").weight_dtype == "fp16" and _StubEngine.made[-1].kw == {}
    assert LlamaRuntime(path, "cuda", weight_dtype="fp16").engine.kw == {}
    rt = LlamaRuntime(path, "cuda", weight_dtype="fp8")
    assert rt.weight_dtype == "fp8" and rt.engine.kw == {"weight_fp8": True}
    assert LlamaRuntime.from_engine(rt.engine).weight_dtype == "fp8"
    n = len(_StubEngine.made)
    for bad in ("fp4", "bf16", None, 8):
        with pytest.raises(ValueError, match="weight_dtype"):
            LlamaRuntime(path, "cuda", weight_dtype=bad)
        with pytest.raises(ValueError, match="weight_dtype"):
            SetwiseLlmRanker(path, path, "cuda", weight_dtype=bad)
    assert len(_StubEngine.made) == n
    assert load_runtime(path, "cuda", weight_dtype="fp8").engine.kw == {"weight_fp8": True}
    tokdir, r1 = os.path.join(GOLD, "tok_qwen"), os.path.join(GOLD, "rankr1_prompt.toml")
    builds = {
        "setwise": lambda **kw: SetwiseLlmRanker(path, path, "cuda", **kw),
        "pairwise": lambda **kw: PairwiseLlmRanker(path, path, "cuda", method="heapsort", **kw),
        "listwise": lambda **kw: ListwiseLlmRanker(path, path, "cuda", 4, 2, **kw),
    }
    for name, build in builds.items():
        assert build().llm.engine.kw == {}, name
        assert build(weight_dtype="fp8").llm.engine.kw == {"weight_fp8": True}, name
    # the two R1 rankers keep the reference's constructor lists: the option is the class's
    assert RankR1SetwiseLlmRanker(path, r1, tokenizer_name_or_path=tokdir).llm.engine.kw == {}
    assert RankR1SetwiseLlmRanker.with_weight_dtype("fp8")(path, r1, tokenizer_name_or_path=tokdir).llm.engine.kw == {"weight_fp8": True}
    assert R1ListwiseLlmRanker(path, tokdir, PROMPT, 4, 2).llm.engine.kw == {}
    fp8_cls = R1ListwiseLlmRanker.with_weight_dtype("fp8")
    assert issubclass(fp8_cls, R1ListwiseLlmRanker) and fp8_cls.__name__ == "R1ListwiseLlmRanker" and R1ListwiseLlmRanker.weight_dtype == "fp16"
    assert fp8_cls(path, tokdir, PROMPT, 4, 2).llm.engine.kw == {"weight_fp8": True}
    with pytest.raises(ValueError, match="weight_dtype"):
        RankR1SetwiseLlmRanker.with_weight_dtype("int8")


def test_t5_checkpoints_refuse_fp8_by_name(monkeypatch, tmp_path):
    from llmrankers import _runtime
    from llmrankers._runtime import load_runtime
    from llmrankers.setwise import SetwiseLlmRanker
    made = []
    monkeypatch.setattr(_runtime, "T5Runtime", lambda *a, **kw: made.append(kw) or "t5")
    path = str(tmp_path / "t5")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "t5"}, f)
    assert load_runtime(path, "cuda") == "t5" and load_runtime(path, "cuda", weight_dtype="fp16") == "t5" and made == [{"cache_dir": None}] * 2
    with pytest.raises(NotImplementedError, match="weight_dtype='fp8'"):
        load_runtime(path, "cuda", weight_dtype="fp8")
    with pytest.raises(NotImplementedError, match="weight_dtype='fp8'.*setwise"):
        SetwiseLlmRanker(path, path, "cuda", weight_dtype="fp8")
    assert len(made) == 2


# ---- plumbing: the command line ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runmod():
    spec = importlib.util.spec_from_file_location("rk_run_fp8", os.path.join(REPO, "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_passes_weight_dtype_only_when_asked(runmod, monkeypatch):
    import llmrankers.listwise as lw
    import llmrankers.pairwise as pw
    import llmrankers.setwise as sw
    made = {}

    class Stub:
        weight_dtype = "fp16"

        def __init__(self, **kw):
            made.clear()
            made.update(kw, cls=type(self), cls_dtype=type(self).weight_dtype)

        @classmethod
        def with_weight_dtype(cls, wd):
            return type(cls.__name__, (cls,), {"weight_dtype": wd})

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
        assert a.run.weight_dtype is None
        runmod.build_ranker(a)
        assert made["cls"] is stubs[name] and "weight_dtype" not in made and made["cls_dtype"] == "fp16", name
        for wd in ("fp8", "fp16"):
            a = runmod.parse_args(parser, commands, run_args + ["--weight_dtype", wd] + tail)
            runmod.build_ranker(a)
            if name.startswith(("RankR1", "R1")):
                assert issubclass(made["cls"], stubs[name]) and made["cls_dtype"] == wd and "weight_dtype" not in made, name
            else:
                assert made["cls"] is stubs[name] and made["weight_dtype"] == wd, name
    with pytest.raises(SystemExit):
        runmod.parse_args(parser, commands, head + ["--weight_dtype", "int8", "setwise"])
    # the T5-only rankers: fp8 is refused by name, fp16 changes nothing
    for run_args, tail in ((head, ["pointwise"]), (["run", "--model_name_or_path", "castorini/duot5-base-msmarco"], ["pairwise"])):
        a = runmod.parse_args(parser, commands, run_args + ["--weight_dtype", "fp8"] + tail)
        with pytest.raises(NotImplementedError, match="weight_dtype fp8"):
            runmod.build_ranker(a)
    a = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", "castorini/duot5-base-msmarco", "--weight_dtype", "fp16", "pairwise"])
    runmod.build_ranker(a)
    assert made["cls"] is stubs["DuoT5LlmRanker"] and "weight_dtype" not in made
