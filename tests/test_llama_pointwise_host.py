"""PointwiseLlmRanker on decoder-only checkpoints, without a GPU: what the reference of tests/_llama_pointwise_ref.py is worth (its
mutants), the ranker's host logic for yes_no and qlm on an oracle-backed runtime (prompt ids, labels, scores, order, counters,
rerank_many, the empty query, fp16 scores), what the constructor builds for each model type (the engine behind the runtime is a stub
that records what it is asked to create), and run.py's choice between candidate sharding and query replicas."""
import importlib.util
import json
import os

import numpy as np
import pytest

import _llama_pointwise_ref as P
from conftest import GOLD, REPO
from llmrankers import _synth
from llmrankers.pointwise import QLM_PROMPT, YES_NO_PROMPT, MonoT5LlmRanker, PointwiseLlmRanker, _softmax_first
from llmrankers.rankers import SearchResult

PASSAGES = ["ocean river water climate", "solar energy policy market price trade", "neural network language model", "court law",
            "health vaccine patient study result method data science", "forest soil food", "music history city school"]
QUERIES = ["which river is the most relevant to the ocean", "neural language model", "price of solar energy ?"]
TOYS = {"tok_llama": _synth.TOY_LLAMA, "tok_qwen": _synth.TOY_QWEN2}


@pytest.fixture(scope="module")
def toys():
    """tokenizer name -> (tokenizer, dims, oracle-backed runtime): built once, never modified"""
    from transformers import AutoTokenizer
    out = {}
    for name, dims in TOYS.items():
        tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, name))
        assert len(tok) <= dims.vocab and tok.chat_template
        out[name] = (tok, dims, P.OraclePointwiseRuntime(dims, _synth.synth_state_dict(dims, seed=929)))
    return out


def _docs():
    return [SearchResult(docid=f"d{i}", score=float(-i), text=t) for i, t in enumerate(PASSAGES)]


def _prompt_ids(tok, text):
    """the spec's prompt ids, restated: one user turn through the chat template with the generation prompt, then the tokenizer"""
    return list(tok(tok.apply_chat_template([{"role": "user", "content": text}], tokenize=False, add_generation_prompt=True))["input_ids"])


def _expected(tok, rt, method, query, docs, fp16=False):
    """(scores float32 [n], prompt lengths, dec_len) from the reference directly - not through the runtime double's calls"""
    if method == "qlm":
        labels = tok.encode(query, add_special_tokens=False)
        seqs = [_prompt_ids(tok, QLM_PROMPT.format(text=d.text)) for d in docs]
        sc = [P.loglik(rt.orc, s + labels, len(labels))[0] if labels else 0.0 for s in seqs]
        return np.asarray(sc, dtype=np.float32), [len(s) for s in seqs], len(labels)
    yes, no = tok.encode("Yes", add_special_tokens=False)[0], tok.encode("No", add_special_tokens=False)[0]
    seqs = [_prompt_ids(tok, YES_NO_PROMPT.format(text=d.text, query=query)) for d in docs]
    z = np.stack([P.logits64(rt.orc, s, rows=[len(s) - 1])[0][[yes, no]] for s in seqs]).astype(np.float32)
    return _softmax_first(z[:, 0], z[:, 1], fp16), [len(s) for s in seqs], 0


def _counters(lens, dec_len, batch_size):
    compare = tokens = 0
    for s in range(0, len(lens), batch_size):
        chunk = lens[s:s + batch_size]
        compare += 1
        tokens += len(chunk) * max(chunk) + len(chunk) * dec_len
    return compare, tokens, 0


# ---- the reference against its own mutants --------------------------------------------------------------------------------------------
# (length, n_labels, seed): the label counts at which ONE wrong term is visible.  The tolerance grows with n_labels and a mutant that
# moves one term does not, so the long label runs of the GPU test (n_labels = len - 1) say nothing here and are not among the inputs.
# The seed is the first at which every mutant is more than 8 tolerances away on both toys (found on the reference alone).
MUTANT_INPUTS = [(2, 1, 1), (17, 1, 1), (17, 3, 1), (129, 1, 1), (129, 3, 1), (300, 1, 1), (300, 3, 1)]


@pytest.mark.parametrize("name", ["tok_llama", "tok_qwen"])
def test_reference_rejects_its_mutants(toys, name):
    _, dims, rt = toys[name]
    worst = {m: np.inf for m in P.MUTANTS}
    for L, n, seed in MUTANT_INPUTS:
        ids = _synth.synth_token_batch(1, L, L, dims.vocab, seed=seed)[0]
        z = P.logits64(rt.orc, ids)
        ref, scale = P.loglik_from_logits(z, ids, n)
        tol = P.qlm_tolerance(n, scale)
        # the definition, once more and independently: log_softmax rows gathered at the shifted labels
        zr = z[L - n - 1:L - 1]
        direct = float(sum((zr[j] - zr[j].max() - np.log(np.exp(zr[j] - zr[j].max()).sum()))[ids[L - n + j]] for j in range(n)))
        assert abs(ref - direct) < 1e-9
        for m in P.MUTANTS:
            if m == "first_from_p" and L == 2:
                continue                                            # (one label of a two-token sequence: "own_position" is that mutant)
            off = abs(P.loglik_from_logits(z, ids, n, m)[0] - ref)
            worst[m] = min(worst[m], off / tol)
            assert off > 5 * tol, (m, L, n, seed, off, tol)
    print({m: round(v, 1) for m, v in worst.items()}, "x tolerance: the closest each mutant comes")


def test_abi_has_rk_llama_qlm():
    """the header declares it, the ctypes table binds it with the header's argument list, the in-tree library exports it"""
    import ctypes as C
    import re
    import __graft_entry__ as g
    from llmrankers import _engine
    g.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rk_engine.h")).read(), flags=re.S)
    decl = re.search(r"int\s+rk_llama_qlm\s*\(([^)]*)\)\s*;", src)
    assert decl and [" ".join(a.split()) for a in decl.group(1).split(",")] == [
        "rk_engine* e", "const int32_t* tokens", "const int32_t* seq_offsets", "int n_seq", "const int32_t* n_labels", "float* out_scores"]
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert _engine.ABI["rk_llama_qlm"] == (C.c_int, [C.c_void_p, i32p, i32p, C.c_int, i32p, f32p])
    lib = _engine.load_library()
    assert lib.rk_llama_qlm.argtypes == _engine.ABI["rk_llama_qlm"][1]
    assert lib.rk_llama_qlm(None, None, None, 0, None, None) == -1                  # RK_ERR_INVALID without an engine: nothing is touched
    assert hasattr(_engine.RkLlamaEngine, "qlm")


def test_end_to_end_inputs_leave_no_query_out():
    """the GPU suite's ranking cases: every query's smallest reference gap exceeds E2E_MIN_GAP tolerances (0 % excluded)"""
    from transformers import AutoTokenizer
    for (toy, tok_name, method), seed in P.E2E_SEEDS.items():
        dims = _synth.NAMED_DIMS[toy]
        orc = P.family_oracle(dims, _synth.synth_state_dict(dims, seed=929))
        tok = AutoTokenizer.from_pretrained(os.path.join(GOLD, tok_name))
        queries, passages = P.e2e_inputs(seed)
        assert len(set(queries)) == len(queries) == 2 and len(passages) == 3
        for q in queries:
            scores, tol, _, _ = P.e2e_expected(tok, orc, method, q, passages)
            print(f"{toy} {method} {q!r}: smallest gap {P.min_gap(scores) / tol:.2f} tolerances ({tol:.3e})")
            assert P.min_gap(scores) > P.E2E_MIN_GAP * tol, (toy, method, q)


# ---- the ranker on the oracle-backed runtime ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tok_llama", "tok_qwen"])
@pytest.mark.parametrize("method", ["yes_no", "qlm"])
def test_ranker_scores_order_counters(toys, name, method):
    tok, _, rt = toys[name]
    for batch_size in (1, 3):
        rk = PointwiseLlmRanker.from_runtime(rt, tok, method=method, batch_size=batch_size)
        assert rk.decoder_only
        for query in QUERIES:
            docs = _docs()
            res = rk.rerank(query, docs)
            want, lens, dec_len = _expected(tok, rt, method, query, docs)
            assert [d.score for d in docs] == [float(x) for x in want]                    # scored in place, in input order
            assert [id(d) for d in res] == [id(d) for d in sorted(docs, key=lambda x: x.score, reverse=True)]   # stable descending sort
            assert (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens) == _counters(lens, dec_len, batch_size)
    if method == "qlm" or name == "tok_llama":                      # (tok_qwen maps "Yes" and "No" to one id: every P(yes) is 0.5 there)
        assert len({d.score for d in docs}) == len(docs)


@pytest.mark.parametrize("name", ["tok_llama", "tok_qwen"])
@pytest.mark.parametrize("method", ["yes_no", "qlm"])
def test_rerank_many_equals_one_by_one(toys, name, method):
    tok, _, rt = toys[name]
    rk = PointwiseLlmRanker.from_runtime(rt, tok, method=method, batch_size=3)
    queries = QUERIES + ([""] if method == "qlm" else [])
    one = []
    for q in queries:
        docs = _docs()
        res = rk.rerank(q, docs)
        one.append(([d.docid for d in res], [d.score for d in docs], (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens)))
    items = [(q, _docs()) for q in queries]
    del rt.calls[:]
    rankings, counters = rk.rerank_many(items)
    if method == "qlm":
        assert rt.calls == [("qlm_many", len(queries) * len(PASSAGES))]                # ONE runtime call for all the queries
    else:                                                                              # (a runtime without score_batches: batch by batch)
        assert {c[0] for c in rt.calls} == {"score"} and sum(c[1] for c in rt.calls) == len(queries) * len(PASSAGES)
    for (q, docs), res, cnt, (ids, scores, c1) in zip(items, rankings, counters, one):
        assert [d.docid for d in res] == ids and [d.score for d in docs] == scores and tuple(cnt) == c1
        assert {id(d) for d in res} == {id(d) for d in docs}


def test_empty_query_scores_zero(toys):
    tok, _, rt = toys["tok_llama"]
    rk = PointwiseLlmRanker.from_runtime(rt, tok, method="qlm", batch_size=2)
    docs = _docs()
    res = rk.rerank("", docs)
    assert [d.score for d in docs] == [0.0] * len(docs) and [d.docid for d in res] == [d.docid for d in docs]
    lens = [len(_prompt_ids(tok, QLM_PROMPT.format(text=d.text))) for d in docs]
    assert (rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens) == _counters(lens, 0, 2)


def test_fp16_scores(toys):
    tok, _, rt = toys["tok_llama"]
    rk = PointwiseLlmRanker.from_runtime(rt, tok, method="yes_no", batch_size=4)
    rk.fp16_scores = True
    docs = _docs()
    rk.rerank(QUERIES[0], docs)
    want, _, _ = _expected(tok, rt, "yes_no", QUERIES[0], docs, fp16=True)
    assert [d.score for d in docs] == [float(x) for x in want]
    assert all(float(np.float16(d.score)) == d.score for d in docs)                    # fp16 values, as the reference's accelerator path gives


def test_base_model_tokenizer_takes_the_plain_text(toys):
    """a tokenizer without a chat template: the prompt text itself is tokenised"""
    import copy
    tok, _, rt = toys["tok_llama"]
    bare = copy.deepcopy(tok)
    bare.chat_template = None
    rk = PointwiseLlmRanker.from_runtime(rt, bare, method="yes_no", batch_size=4)
    assert rk._prompt_ids(["a b"]) == [list(bare("a b")["input_ids"])]
    assert PointwiseLlmRanker.from_runtime(rt, tok, method="yes_no")._prompt_ids(["a b"]) == [_prompt_ids(tok, "a b")]


def test_runtime_chunks_and_empty_labels():
    """LlamaRuntime.score / qlm / qlm_many over a recording engine: capacity chunks count prompt + label tokens, an empty label
    list never reaches the engine, a decoder prefix is refused"""
    from types import SimpleNamespace
    from llmrankers._runtime import LlamaRuntime

    class Eng:
        dims, desc = _synth.TOY_LLAMA, SimpleNamespace(max_tokens=19, max_seqs=3)

        def __init__(self):
            self.calls = []

        def qlm(self, seqs, n_labels):
            self.calls.append(([list(s) for s in seqs], list(n_labels)))
            return np.asarray([float(sum(s[len(s) - n:])) for s, n in zip(seqs, n_labels)], dtype=np.float32)

        def last_logits(self, seqs, out_ids):
            self.calls.append(([list(s) for s in seqs], list(out_ids)))
            return np.asarray([[float(len(s)) + o for o in out_ids] for s in seqs], dtype=np.float32)

    eng = Eng()
    rt = LlamaRuntime.from_engine(eng)
    seqs = [[1] * 6, [2] * 6, [3] * 6, [4] * 2, [5] * 2]
    labels = [[7, 8], [], [9], [1, 1, 1], [2]]
    got = rt.qlm_many(seqs, labels)
    assert got.dtype == np.float32 and list(got) == [15.0, 0.0, 9.0, 3.0, 2.0]
    # 8 + 7 of the 19 tokens, the next 5 no longer fit; the empty one is skipped; then 5 + 3
    assert eng.calls == [([[1] * 6 + [7, 8], [3] * 6 + [9]], [2, 1]), ([[4] * 2 + [1, 1, 1], [5] * 2 + [2]], [3, 1])]
    assert list(rt.qlm(seqs[:2], [4])) == [4.0, 4.0] and list(rt.qlm(seqs[:2], [])) == [0.0, 0.0]
    del eng.calls[:]
    sc = rt.score(seqs, [], [10, 20])
    assert sc.shape == (5, 2) and [len(c[0]) for c in eng.calls] == [3, 2]             # max_seqs 3, then the rest
    assert rt.score([], [], [1, 2]).shape == (0, 2)
    # the ranker's batches of one query are merged up to the capacity and cut back
    assert [p.tolist() for p in rt.score_batches([seqs[:2], seqs[2:]], [], [10])] == [[[16.0], [16.0]], [[16.0], [12.0], [12.0]]]
    assert [p.tolist() for p in rt.qlm_batches([seqs[:1], seqs[1:3]], [4])] == [[4.0], [4.0, 4.0]]
    assert rt.score_batches([], [], [1]) == [] and rt.qlm_batches([], [4]) == []
    with pytest.raises(ValueError, match="decoder prefix"):
        rt.score(seqs, [0], [10, 20])
    with pytest.raises(ValueError):
        rt.qlm_many(seqs, labels[:2])


# ---- the constructor on stub engines (the fixture pattern of tests/test_llama_hd64_host.py) -------------------------------------------
class _StubEngine:
    """RkLlamaEngine's / RkEngine's constructor and loader, recording what the runtimes ask the engine for"""
    made = []

    def __init__(self, dims, device=0, max_tokens=16384, max_seqs=16, max_dec_len=None):
        self.dims, self.max_seqs, self.max_dec_len, self.loaded = dims, max_seqs, max_dec_len, 0
        _StubEngine.made.append(self)

    def load_state(self, tensors):
        self.loaded = sum(1 for _ in tensors)
        return self

    def close(self):
        pass


@pytest.fixture()
def stub_engine(monkeypatch):
    from llmrankers import _runtime
    monkeypatch.setattr(_runtime, "RkLlamaEngine", _StubEngine)
    monkeypatch.setattr(_runtime, "RkEngine", _StubEngine)
    del _StubEngine.made[:]
    return _StubEngine


def _write(tmp_path, name, dims, tok):
    import shutil
    from safetensors.numpy import save_file
    path = str(tmp_path / name)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dims.to_hf_config(), f)
    save_file({"model.norm.weight": np.ones(dims.hidden, np.float32)}, os.path.join(path, "model.safetensors"))
    for fn in os.listdir(os.path.join(GOLD, tok)):
        shutil.copy(os.path.join(GOLD, tok, fn), os.path.join(path, fn))
    return path


FAMILIES = {"llama": (_synth.TOY_LLAMA_HD64, "tok_llama"), "qwen2": (_synth.TOY_QWEN2, "tok_qwen"), "qwen3": (_synth.TOY_QWEN3, "tok_qwen"),
            "mistral": (_synth.TOY_MISTRAL, "tok_llama")}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_constructor_builds_a_llama_runtime(stub_engine, tmp_path, family):
    from llmrankers._runtime import LlamaRuntime
    dims, tok = FAMILIES[family]
    path = _write(tmp_path, family, dims, tok)
    for method in ("yes_no", "qlm"):
        rk = PointwiseLlmRanker(path, None, "cuda", method=method, batch_size=4)
        assert isinstance(rk.llm, LlamaRuntime) and rk.llm.model_type == family and rk.decoder_only
        assert rk.llm.max_seqs == 64 and rk.llm.engine is stub_engine.made[-1] and rk.llm.engine.max_seqs == 64 and rk.llm.engine.dims == dims
        assert rk.tokenizer.chat_template and (rk.method, rk.batch_size, rk.shard_candidates) == (method, 4, False)
    n = len(stub_engine.made)
    # what stays refused, before an engine is asked for: candidate sharding, MonoT5 on a decoder-only checkpoint
    with pytest.raises(NotImplementedError, match="shard_candidates"):
        PointwiseLlmRanker(path, None, "cuda", method="yes_no", shard_candidates=True)
    with pytest.raises(NotImplementedError, match="not supported yet"):
        MonoT5LlmRanker(path, None, "cuda", method="yes_no")
    with pytest.raises(NotImplementedError, match="shard_candidates"):
        PointwiseLlmRanker.from_runtime(rk.llm, rk.tokenizer, method="qlm", shard_candidates=True)
    assert len(stub_engine.made) == n


def test_constructor_t5_and_unknown_types(stub_engine, tmp_path, ckpt_dirs):
    from transformers import T5Tokenizer
    from llmrankers._runtime import T5Runtime
    rk = PointwiseLlmRanker(ckpt_dirs["ckpt_gated_untied"], None, "cuda", method="yes_no", batch_size=2)
    assert isinstance(rk.llm, T5Runtime) and isinstance(rk.tokenizer, T5Tokenizer) and not rk.decoder_only
    assert stub_engine.made[-1].max_seqs == 256 and stub_engine.made[-1].max_dec_len == 136     # T5Runtime's defaults, as before
    rk = PointwiseLlmRanker(ckpt_dirs["ckpt_gated_untied"], None, "cuda", method="yes_no", shard_candidates=True)
    assert rk.shard_candidates and not rk.decoder_only                                         # T5 keeps candidate sharding
    n = len(stub_engine.made)
    other = str(tmp_path / "gpt2")
    os.makedirs(other)
    with open(os.path.join(other, "config.json"), "w") as f:
        json.dump({"model_type": "gpt2"}, f)                                                   # (no tokenizer files: none is built)
    with pytest.raises(NotImplementedError, match="Model type gpt2 is not supported yet"):
        PointwiseLlmRanker(other, None, "cuda")
    assert len(stub_engine.made) == n


# ---- run.py ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runmod():
    spec = importlib.util.spec_from_file_location("rk_run_llama_pointwise", os.path.join(REPO, "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(runmod, model, *extra, method="qlm"):
    parser, commands = runmod.build_parser()
    args = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", model, "--run_path", "r", "--save_path", "s", *extra,
                                                "pointwise", "--method", method, "--batch_size", "4"])
    runmod.validate(args)
    return args


def test_run_py_runs_decoder_only_checkpoints_as_query_replicas(runmod, stub_engine, tmp_path, ckpt_dirs):
    llama = _write(tmp_path, "llama", _synth.TOY_LLAMA_HD64, "tok_llama")
    qwen = _write(tmp_path, "qwen3", _synth.TOY_QWEN3, "tok_qwen")
    t5 = ckpt_dirs["ckpt_gated_untied"]
    assert runmod.decoder_only_checkpoint(llama) and runmod.decoder_only_checkpoint(qwen) and not runmod.decoder_only_checkpoint(t5)
    assert not runmod.decoder_only_checkpoint(str(tmp_path / "nowhere"))
    for world, want_t5 in ((1, False), (2, True), (8, True)):
        assert runmod.candidates_sharded(_args(runmod, t5), world) is want_t5
        assert runmod.candidates_sharded(_args(runmod, llama), world) is False                 # replicas, decided from config.json
        assert runmod.candidates_sharded(_args(runmod, qwen), world) is False
        assert runmod.candidates_sharded(_args(runmod, llama, "--shard_candidates", "0"), world) is False
        assert runmod.candidates_sharded(_args(runmod, llama, "--shard_candidates", "1"), world) is (world > 1)   # asked for: the constructor refuses
    # build_ranker: a decoder-only pointwise ranker; fp8 stays refused with its message
    rk = runmod.build_ranker(_args(runmod, llama))
    assert isinstance(rk, PointwiseLlmRanker) and rk.decoder_only and rk.llm.max_seqs == 64 and not rk.shard_candidates
    with pytest.raises(NotImplementedError, match="--weight_dtype fp8 is not supported by the pointwise rankers"):
        runmod.build_ranker(_args(runmod, llama, "--weight_dtype", "fp8"))


def test_run_py_pointwise_qlm_through_rerank_many(runmod, toys, tmp_path, monkeypatch):
    """run.py ... pointwise --method qlm on a decoder-only ranker: the TREC round trip, several queries per runtime call"""
    tok, _, rt = toys["tok_llama"]
    monkeypatch.setattr(runmod, "build_ranker", lambda args: PointwiseLlmRanker.from_runtime(rt, tok, method=args.pointwise.method,
                                                                                            batch_size=args.pointwise.batch_size))
    (tmp_path / "q.tsv").write_text("".join(f"q{i}\t{q}\n" for i, q in enumerate(QUERIES)))
    (tmp_path / "d.jsonl").write_text("".join(json.dumps({"docid": f"d{i}", "title": "", "text": t}) + "\n" for i, t in enumerate(PASSAGES[:5])))
    (tmp_path / "in.trec").write_text("".join(f"q{q} Q0 d{i} {i + 1} {10 - i} bm25\n" for q in range(len(QUERIES)) for i in range(5)))
    args = _args(runmod, "unused", "--query_file", str(tmp_path / "q.tsv"), "--doc_file", str(tmp_path / "d.jsonl"), "--hits", "5",
                 "--queries_per_call", "3")
    args.run.run_path, args.run.save_path = str(tmp_path / "in.trec"), str(tmp_path / "out.trec")
    del rt.calls[:]
    runmod.main(args)
    out = [line.split() for line in (tmp_path / "out.trec").read_text().splitlines()]
    assert len(out) == 15 and rt.calls == [("qlm_many", 15)]
    for q in range(len(QUERIES)):
        mine = [l for l in out if l[0] == f"q{q}"]
        scores = [float(l[4]) for l in mine]
        assert scores == sorted(scores, reverse=True) and sorted(l[2] for l in mine) == [f"d{i}" for i in range(5)]
