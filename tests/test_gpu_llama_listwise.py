"""rk_llama_generate (KV-cached incremental greedy decoding on Llama checkpoints) and the listwise ranker's Llama branch on the HIP
engine: the step kernel against the fp32 oracle at every chunk count, tokens against the oracle and the re-prefill loop, batch
independence, the contract, the reference's recorded listwise cases end to end and run.py's listwise sub-command."""
import contextlib
import copy
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
FLOOR = 5e-3              # fp16 noise floor of the toy scale (test_gpu_rerank.py)
CHUNK = 128               # attn_dec_cached_kernel: keys per workgroup (csrc/llama_kernels.h: LDC_CHUNK)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "llama_listwise_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lw_ckpt(gold, tmp_path_factory):
    from llmrankers import _synth
    path = str(tmp_path_factory.mktemp("llama_listwise_gpu") / "toy-llama")
    _synth.write_checkpoint(path, gold["ckpt"], os.path.join(GOLD, gold["tokenizer"]))
    assert _synth.checkpoint_sha256(path) == gold["ckpt"]["sha256"]
    return path


def _state(path):
    from conftest import load_state
    return load_state(path)


def _engine(dims, state, **kw):
    from llmrankers._engine import RkLlamaEngine
    kw.setdefault("max_tokens", 32768)
    kw.setdefault("max_seqs", 128)
    return RkLlamaEngine(dims, device=0, **kw).load_state(state.items())


def _head(dims, state):
    return np.asarray(state["model.embed_tokens.weight"] if dims.tied_head else state["lm_head.weight"], dtype=np.float32)


def _oracle_rows(orc, seqs, max_new, eos_ids=(), max_total=0):
    from _llama_gen_stub import oracle_greedy
    return [oracle_greedy(orc, s, max_new, eos_ids, max_total) for s in seqs]


def test_step_kernel_vs_oracle_at_every_chunk_count():
    """prefixes of one 700-token sequence whose lengths straddle the kernel's chunk boundaries (and 1, 2, 3 tokens), max_new 1 .. 6,
    no EOS: exactly max_new - 1 steps run; the final-normed rows the LAST step's head read, times head^T, against the oracle's
    logits of prompt + generated[:max_new - 1] - within the bound the prefill itself is held to (4e-3 x scale)"""
    from llmrankers import _synth
    from oracle.llama_numpy import LlamaOracle
    dims = _synth.TOY_LLAMA
    state = _synth.synth_state_dict(dims, seed=929)
    base = _synth.synth_token_batch(1, 700, 700, dims.vocab, seed=17)[0]
    lens = sorted(set([1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97] + [k * CHUNK + d for k in range(1, 6) for d in (-6, -5, -2, -1, 0, 1)]
                      + [694, 700] + list(range(7, 700, 97))))
    seqs = [base[:n] for n in lens]
    orc, head = LlamaOracle(dims, state), _head(dims, state)
    eng = _engine(dims, state)
    worst = 0.0
    for max_new in range(1, 7):
        toks, steps = eng.generate(seqs, max_new, [], 0)
        assert steps == max_new and toks.shape == (len(seqs), max_new)
        last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), dims.hidden)
        got = last @ head.T
        want = orc.last_logits([list(s) + [int(t) for t in toks[b, :max_new - 1]] for b, s in enumerate(seqs)])
        scale = float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        worst = max(worst, err / scale)
        print(f"max_new {max_new}: max |logit - oracle| = {err:.3e} at scale {scale:.2f}")
        assert err < 4e-3 * scale, (max_new, err, scale)
    print(f"worst relative error {worst:.3e}")
    eng.close()


def test_tokens_vs_oracle_greedy1_and_the_reprefill_loop(gold, lw_ckpt):
    """5 synthetic prompts, 20 new tokens, on the random toy weights and on the listwise fixture's: generated tokens == the
    oracle's up to the first step whose oracle margin is under the floor; column 0 == rk_llama_greedy1; == a greedy1 re-prefill
    loop over the same steps"""
    from llmrankers import _synth
    from oracle.llama_numpy import LlamaOracle
    checked = 0
    for name in ("random", "listwise"):
        dims, state = (_synth.TOY_LLAMA, _synth.synth_state_dict(_synth.TOY_LLAMA, seed=929)) if name == "random" else _state(lw_ckpt)
        eng = _engine(dims, state)
        seqs = _synth.synth_token_batch(5, 8, 120, dims.vocab, seed=7)
        gen, steps = eng.generate(seqs, 20, [], 0)
        assert steps == 20
        np.testing.assert_array_equal(gen[:, 0], eng.greedy1(seqs))
        ref = _oracle_rows(LlamaOracle(dims, state), seqs, 20)
        for b, (toks, margins) in enumerate(ref):
            low = next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
            assert list(gen[b, :low]) == toks[:low], (name, b, low)
            cur = list(seqs[b])
            for t in range(low):                                   # the parent's only route to the same tokens
                assert int(eng.greedy1([cur])[0]) == int(gen[b, t]), (name, b, t)
                cur.append(int(gen[b, t]))
            checked += low
        eng.close()
    assert checked >= 20, checked


def test_batch_independence(lw_ckpt):
    """8 ragged prompts (3 .. 700 tokens): a row alone, in the batch, in the reversed batch - equal tokens wherever the oracle
    margins clear the floor; the final-normed rows of a no-EOS run equal bit for bit between batch and reversed batch"""
    from llmrankers import _synth
    from oracle.llama_numpy import LlamaOracle
    dims, state = _state(lw_ckpt)
    eng = _engine(dims, state)
    rs = np.random.RandomState(23)
    lens = [3, 700, 129, 47, 256, 511, 64, 390]
    seqs = [rs.randint(3, dims.vocab - 28, size=n).astype(np.int32) for n in lens]
    batch, _ = eng.generate(seqs, 12, [], 0)
    last = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), -1).copy()
    rev, _ = eng.generate(seqs[::-1], 12, [], 0)
    last_rev = eng.debug_read("llama_last", len(seqs) * dims.hidden).reshape(len(seqs), -1)
    np.testing.assert_array_equal(rev[::-1], batch)
    assert np.array_equal(last_rev[::-1].view(np.uint32), last.view(np.uint32))
    ref = _oracle_rows(LlamaOracle(dims, state), seqs, 12)
    for b, s in enumerate(seqs):
        alone, _ = eng.generate([s], 12, [], 0)
        toks, margins = ref[b]
        low = next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
        assert list(alone[0, :low]) == list(batch[b, :low]) == toks[:low], (b, low)
    # with the model's EOS: every row up to its own stop, alone == in the batch
    eos = [2]
    bt, bsteps = eng.generate(seqs, 12, eos, 0)
    for b, s in enumerate(seqs):
        at, asteps = eng.generate([s], 12, eos, 0)
        toks, margins = ref[b]
        low = next((i for i, m in enumerate(margins) if m <= FLOOR), len(margins))
        n = min(asteps, low)
        assert list(at[0, :n]) == list(bt[b, :n]) and asteps <= bsteps
    eng.close()


def test_contract(lw_ckpt, ckpt_dirs):
    """pad after EOS, early stop and out_steps, two EOS ids, max_total ending a row, n_eos = 0, every error and its code"""
    from llmrankers import _synth
    from llmrankers._engine import RkEngine, RkError
    dims, state = _state(lw_ckpt)
    eng = _engine(dims, state, max_tokens=2048, max_seqs=8)
    seqs = _synth.synth_token_batch(6, 5, 200, dims.vocab, seed=3)
    free, steps = eng.generate(seqs, 10, [], 7)
    assert steps == 10 and (free >= 0).all()
    e1 = int(free[0, 2])                                          # an EOS id that row 0 produces at column <= 2
    toks, steps = eng.generate(seqs, 10, [e1], 7)
    done_at = []
    for b, row in enumerate(toks):
        hit = np.where(row == e1)[0]
        stop = int(hit[0]) + 1 if len(hit) else 10
        done_at.append(stop)
        assert list(row[:stop]) == list(free[b, :stop])          # the same tokens up to the row's stop
        assert (row[stop:] == 7).all()                            # pad after EOS
    assert steps == max(done_at) and done_at[0] <= 3
    one, s1 = eng.generate(seqs[:1], 10, [e1], 7)                 # early stop of the whole call
    assert s1 == done_at[0] < 10 and (one[0, s1:] == 7).all()
    e2 = int(free[1, 1])
    two, s2 = eng.generate(seqs, 10, [e1, e2], 7)                 # two EOS ids: each row stops at the first of either
    stops = []
    for b, row in enumerate(two):
        hit = [i for i, t in enumerate(free[b]) if int(t) in (e1, e2)]
        stop = hit[0] + 1 if hit else 10
        stops.append(stop)
        assert list(row[:stop]) == list(free[b, :stop]) and (row[stop:] == 7).all()
    assert s2 == max(stops) and stops[1] <= 2
    total = len(seqs[0]) + 4                                      # max_total ends row 0 after 4 new tokens; the others go on
    lim, s3 = eng.generate(seqs[:2], 10, [], 7, max_total=total)
    assert list(lim[0, :4]) == list(free[0, :4]) and (lim[0, 4:] == 7).all()
    n1 = max(0, min(10, total - len(seqs[1])))
    assert list(lim[1, :n1]) == list(free[1, :n1]) and s3 == max(4, n1)
    for bad, code in ((lambda: eng.generate(seqs, 0, [], 0), -1), (lambda: eng.generate(seqs, 4, list(range(9)), 0), -1),
                      (lambda: eng.generate(seqs, 4, [dims.vocab], 0), -1), (lambda: eng.generate(seqs, 4, [], -1), -1),
                      (lambda: eng.generate(seqs, 4, [], 0, max_total=len(seqs[0])), -1),
                      (lambda: eng.generate([list(range(3, 103))] * 3, 2048 - 99, [], 0), -6),       # longest prompt + max_new > max_tokens
                      (lambda: eng.generate([[5, 6]] * 9, 4, [], 0), -6),                            # more prompts than max_seqs
                      (lambda: eng.generate([[5] * 1100, [6] * 1100], 4, [], 0), -6)):                # more tokens than max_tokens
        with pytest.raises(RkError) as ex:
            bad()
        assert ex.value.code == code, (ex.value.code, code, str(ex.value))
    eng.generate([list(range(3, 103))], 2048 - 100, [int(free[0, 0])], 0)   # 100 + 1948 = max_tokens fits (and stops at once)
    eng.close()
    # a T5 engine refuses the call
    import ctypes as C
    from llmrankers._engine import _i32p, pack_ragged
    t5dims, t5state = _state(ckpt_dirs["ckpt_gated_untied"])
    t5 = RkEngine(t5dims, device=0, max_tokens=512, max_seqs=4, max_dec_len=4).load_state(t5state.items())
    tok, off = pack_ragged([[5, 6, 7]])
    out, st = np.zeros((1, 2), np.int32), C.c_int32(0)
    rc = t5.lib.rk_llama_generate(t5.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), 1, 2, 0, None, 0, 0,
                                  out.ctypes.data_as(_i32p), C.byref(st))
    assert rc == -4
    t5.close()


def test_llama_3_8b_widths_vs_oracle():
    """Llama-3-8B widths with two layers (the oracle runs on the host), the head rows of 23 label tokens boosted x 6 as the 8B
    goldens do (random heads are too flat for the floor of this scale), one 1 500-token and one 45-token prompt, 8 new tokens:
    tokens == the oracle's up to the first step whose oracle margin is under 0.02 x scale, == the greedy1 re-prefill loop there.
    The oracle alone (seed 929): 8 clear steps on the short prompt (smallest margin 1.73), 2 on the long one (6.16, 3.18, then
    0.28 < 0.36)."""
    from llmrankers import _synth
    from oracle.llama_numpy import LlamaOracle
    dims = _synth.LlamaDims(vocab=128256, hidden=4096, n_heads=32, n_kv_heads=8, head_dim=128, intermediate=14336, n_layers=2,
                            bos_token_id=128000, eos_token_id=128001)
    state = _synth.synth_state_dict(dims, seed=929, threads=16)
    ids = np.arange(32, 32 + 23)
    w = state["lm_head.weight"].copy()
    w[ids] = (w[ids] * np.float32(6.0)).astype(np.float16).astype(np.float32)
    state["lm_head.weight"] = w
    eng = _engine(dims, state, max_tokens=4096, max_seqs=8)
    seqs = [s for n in (1500, 45) for s in _synth.synth_token_batch(1, n, n, dims.vocab, seed=100 + n)]
    gen, steps = eng.generate(seqs, 8, [], 0)
    assert steps == 8
    np.testing.assert_array_equal(gen[:, 0], eng.greedy1(seqs))
    orc = LlamaOracle(dims, state)
    scale = float(np.abs(orc.last_logits(seqs)).max())
    total = 0
    for b, (toks, margins) in enumerate(_oracle_rows(orc, seqs, 8)):
        low = next((i for i, m in enumerate(margins) if m <= 0.02 * scale), len(margins))
        print(f"prompt of {len(seqs[b])}: margins {[round(m, 3) for m in margins]}, scale {scale:.2f}, checked {low}")
        assert list(gen[b, :low]) == toks[:low], (b, low)
        cur = list(seqs[b])
        for t in range(low):
            assert int(eng.greedy1([cur])[0]) == int(gen[b, t]), (b, t)
            cur.append(int(gen[b, t]))
        total += low
    assert total >= 2, total
    np.testing.assert_array_equal(eng.generate(seqs[::-1], 8, [], 0)[0][::-1], gen)
    eng.close()


def _ranking(case):
    from llmrankers.rankers import SearchResult
    return [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]]


def test_listwise_golden_cases_on_the_engine(gold, lw_ckpt):
    from transformers import AutoTokenizer
    from llmrankers._runtime import LlamaRuntime
    from llmrankers.listwise import ListwiseLlmRanker
    assert gold["min_margin"] > FLOOR
    rt = LlamaRuntime(lw_ckpt, "cuda", max_tokens=16384, max_seqs=16)
    assert rt.generation["eos_token_ids"] == [gold["model_eos"]]
    tok = AutoTokenizer.from_pretrained(lw_ckpt)
    tok.use_default_system_prompt = False
    for case in gold["cases"]:
        rk = ListwiseLlmRanker.from_runtime(rt, tok, window_size=case["window_size"], step_size=case["step_size"],
                                            scoring=case["scoring"], num_repeat=case["num_repeat"])
        outs = []
        real = rk.compare
        rk.compare = lambda q, docs: outs.append(real(q, docs)) or outs[-1]
        ranking = _ranking(case)
        res = rk.rerank(case["query"], ranking)
        tag = case["qid"]
        assert outs == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [d.docid for d in ranking] == [d for d, _ in case["docs"]], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
    # lockstep == one query at a time, every query of the fixture three times
    case = next(c for c in gold["cases"] if c["window_size"] == 4)
    rk = ListwiseLlmRanker.from_runtime(rt, tok, window_size=4, step_size=2, num_repeat=2)
    items = [(c["query"], _ranking(c)) for c in gold["cases"]] * 3
    want, wc = [], []
    for q, r in copy.deepcopy(items):
        want.append([(d.docid, d.score) for d in rk.rerank(q, r)])
        wc.append((rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens))
    got, counters = rk.rerank_many(items)
    assert [[(d.docid, d.score) for d in res] for res in got] == want
    assert counters == wc
    assert [d.docid for d in got[gold["cases"].index(case)]] == case["docids"]
    rt.engine.close()


def test_run_py_listwise_on_a_llama_checkpoint(gold, lw_ckpt, tmp_path):
    """run.py ... listwise --window_size 4 --step_size 2 --num_repeat 2 on the Llama checkpoint: the reference's recorded ranking
    for that case, and the same run file one query at a time as in lockstep"""
    import importlib.util
    from conftest import REPO
    spec = importlib.util.spec_from_file_location("rk_run_llama_lw_gpu", os.path.join(REPO, "run.py"))
    runmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(runmod)
    case = next(c for c in gold["cases"] if c["window_size"] == 4)
    (tmp_path / "q.tsv").write_text(f"{case['qid']}\t{case['query']}\nqx\t{case['query']} river\n")
    (tmp_path / "d.tsv").write_text("".join(f"{d}\t{t}\n" for d, t in case["docs"]))
    lines = [f"{q} Q0 {d} {r + 1} {100 - r} bm25" for q in (case["qid"], "qx") for r, (d, _) in enumerate(case["docs"])]
    (tmp_path / "in.trec").write_text("\n".join(lines) + "\n")
    parser, commands = runmod.build_parser()

    def run(save, extra):
        args = runmod.parse_args(parser, commands, ["run", "--model_name_or_path", lw_ckpt, "--run_path", str(tmp_path / "in.trec"),
                                                    "--save_path", str(save), "--query_file", str(tmp_path / "q.tsv"),
                                                    "--doc_file", str(tmp_path / "d.tsv"), "--hits", "8", "--passage_length", "512",
                                                    "--query_length", "64", *extra, "listwise", "--window_size", "4",
                                                    "--step_size", "2", "--num_repeat", "2"])
        runmod.validate(args)
        with contextlib.redirect_stdout(io.StringIO()):
            runmod.main(args)
        return save.read_text()

    one = run(tmp_path / "one.trec", ["--queries_per_call", "1"])
    many = run(tmp_path / "many.trec", [])
    assert one == many
    rows = [l.split() for l in one.splitlines() if l.split()[0] == case["qid"]]
    assert [r[2] for r in rows] == case["docids"]
