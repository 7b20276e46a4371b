"""rk_t5_generate (KV-cached incremental greedy decoding) and the listwise ranker on the HIP engine: the cached attention kernel
against attn_dec_kernel, the new entry point against rk_t5_greedy and the fp32 oracle, batch independence, the contract, flan-t5-large
dims, the reference's recorded listwise cases end to end and run.py's listwise sub-command."""
import contextlib
import copy
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
MARGIN_FLOOR = 5e-3       # fp16 noise floor of the toy scale (test_gpu_rerank.py)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "listwise_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lw_ckpt(gold, tmp_path_factory):
    from llmrankers import _synth
    path = str(tmp_path_factory.mktemp("listwise_gpu") / "ckpt")
    _synth.write_checkpoint(path, gold["ckpt"], os.path.join(GOLD, gold["tokenizer"]))
    assert _synth.checkpoint_sha256(path) == gold["ckpt"]["sha256"]
    return path


def _engine(dims, state, **kw):
    from llmrankers._engine import RkEngine
    kw.setdefault("max_tokens", 4096)
    kw.setdefault("max_seqs", 32)
    kw.setdefault("max_dec_len", 24)
    return RkEngine(dims, device=0, **kw).load_state(state.items())


def _state(path):
    from conftest import load_state
    return load_state(path)


def _oracle_steps(orc, seqs, prefix, max_new, eos=1):
    """fp32 oracle greedy per row: tokens and the top-1 / top-2 margin of every step"""
    out = []
    for ids in seqs:
        enc = orc.encode(ids)
        cur, toks, margins = list(prefix), [], []
        for _ in range(max_new):
            lg = orc.decode(enc, cur)[-1]
            s = np.sort(lg)
            margins.append(float(s[-1] - s[-2]))
            nxt = int(np.argmax(lg))
            toks.append(nxt)
            cur.append(nxt)
            if nxt == eos:
                break
        out.append((toks, margins))
    return out


def _prompts(vocab, n, lo, hi, seed):
    from llmrankers import _synth
    return _synth.synth_token_batch(n, lo, hi, vocab, seed=seed)


def test_cached_attention_matches_attn_dec_kernel(lw_ckpt):
    """attn_dec_cached_kernel against attn_dec_kernel (tree form) over the same cache rows (option dec_cached_attn = 0): every
    context row of every step and layer feeds the rest of the chain, so identical tokens AND a bit-identical residual stream after
    the last step mean bit-identical context rows"""
    dims, state = _state(lw_ckpt)
    eng = _engine(dims, state)
    seqs = _prompts(dims.vocab, 6, 5, 150, seed=41)
    for prefix in ([0], [0, 186]):
        want, wsteps = eng.generate(seqs, prefix, 20)
        h_want = eng.debug_read("dec_hidden", len(seqs) * dims.d_model)
        eng.set_option("dec_cached_attn", 0)
        got, gsteps = eng.generate(seqs, prefix, 20)
        h_got = eng.debug_read("dec_hidden", len(seqs) * dims.d_model)
        eng.set_option("dec_cached_attn", 1)
        np.testing.assert_array_equal(got, want)
        assert gsteps == wsteps
        assert np.array_equal(h_got.view(np.uint32), h_want.view(np.uint32))
    eng.close()


@pytest.mark.parametrize("name", ["ckpt_gated_untied", "ckpt_relu_tied", "listwise"])
def test_generate_vs_greedy_and_oracle(name, ckpt_dirs, lw_ckpt):
    """max_new = 20, dec_len 1 and 2: tokens of rk_t5_generate = rk_t5_greedy's = the oracle's up to the first step whose oracle
    margin is below the floor; out_steps equal wherever every row clears it"""
    from oracle.t5_numpy import T5Oracle
    dims, state = _state(lw_ckpt if name == "listwise" else ckpt_dirs[name])
    eng = _engine(dims, state)
    orc = T5Oracle(dims, state)
    seqs = _prompts(dims.vocab, 5, 8, 120, seed=7)
    checked = 0
    for prefix in ([0], [0, 186]):
        gen, gsteps = eng.generate(seqs, prefix, 20)
        grd, rsteps = eng.greedy(seqs, prefix, 20)
        ref = _oracle_steps(orc, seqs, prefix, 20)
        clear = True
        for b, (toks, margins) in enumerate(ref):
            low = next((i for i, m in enumerate(margins) if m <= MARGIN_FLOOR), len(margins))
            clear = clear and low == len(margins)
            assert list(gen[b, :low]) == toks[:low], (name, prefix, b)
            assert list(grd[b, :low]) == toks[:low], (name, prefix, b)
            checked += low
        if clear:
            assert gsteps == rsteps
            np.testing.assert_array_equal(gen[:, :gsteps], grd[:, :rsteps])
    assert checked >= 20
    eng.close()


def test_generate_batch_independence(lw_ckpt):
    dims, state = _state(lw_ckpt)
    eng = _engine(dims, state)
    seqs = _prompts(dims.vocab, 8, 3, 250, seed=19)            # ragged: 1 .. 4 key chunks
    for prefix in ([0], [0, 186]):
        batch, bsteps = eng.generate(seqs, prefix, 20)
        for b, s in enumerate(seqs):
            alone, steps = eng.generate([s], prefix, 20)
            np.testing.assert_array_equal(alone[0, :steps], batch[b, :steps])
            assert (batch[b, steps:] == 0).all() and steps <= bsteps
    eng.close()


def test_generate_contract(lw_ckpt):
    """pad after EOS, early stop, capacity error"""
    from llmrankers._engine import RkError
    dims, state = _state(lw_ckpt)
    eng = _engine(dims, state, max_dec_len=24)
    seqs = _prompts(dims.vocab, 8, 5, 200, seed=3)
    toks, steps = eng.generate(seqs, [0], 20, eos_id=1, pad_id=0)
    grd, gsteps = eng.greedy(seqs, [0], 20, eos_id=1, pad_id=0)
    assert steps == gsteps
    for row in toks:
        hit = np.where(row == 1)[0]
        if len(hit):
            assert (row[hit[0] + 1:] == 0).all()
    done_at = [int(np.where(r == 1)[0][0]) + 1 if (r == 1).any() else 20 for r in toks]
    assert steps == max(done_at)
    # early stop: EOS forced as the last prefix token's continuation is not possible, so take rows that stop on their own
    stoppers = [s for s, d in zip(seqs, done_at) if d < 20]
    if stoppers:
        t2, s2 = eng.generate(stoppers, [0], 20)
        assert s2 < 20 and (t2[:, s2:] == 0).all()
    # another eos id: every row that produces it stops there
    t3, s3 = eng.generate(seqs, [0], 20, eos_id=int(toks[0, 0]), pad_id=5)
    assert t3[0, 0] == toks[0, 0] and (t3[0, 1:] == 5).all()
    assert (t3[:, s3:] == 5).all()
    with pytest.raises(RkError) as ex:
        eng.generate(seqs, [0, 186], 24)                       # 2 + 24 - 1 > 24
    assert ex.value.code == -6
    with pytest.raises(RkError) as ex:
        eng.greedy(seqs, [0, 186], 24)
    assert ex.value.code == -6
    eng.generate(seqs, [0, 186], 23)                           # 2 + 23 - 1 = 24 fits
    eng.close()


def test_generate_flan_t5_large_dims():
    """flan-t5-large dims, seeded synthetic weights, 4 prompts of 300-500 tokens: tokens = the oracle's up to the first step whose
    oracle margin is below the noise floor of this scale, and = rk_t5_greedy's there"""
    from llmrankers import _synth
    from oracle.t5_numpy import T5Oracle
    dims = _synth.FLAN_T5_LARGE
    state = _synth.synth_state_dict(dims, seed=929, threads=16)
    eng = _engine(dims, state, max_tokens=4096, max_seqs=8, max_dec_len=24)
    seqs = _synth.synth_token_batch(4, 300, 500, dims.vocab, seed=931)
    gen, gsteps = eng.generate(seqs, [0], 20)
    grd, rsteps = eng.greedy(seqs, [0], 20)
    ref = _oracle_steps(T5Oracle(dims, state), seqs, [0], 20)
    total = 0
    for b, (toks, margins) in enumerate(ref):
        floor = 8e-3 * 8.0                                      # 8e-3 of the logit scale (test_gpu_rerank.py), logits of |x| <~ 8
        low = next((i for i, m in enumerate(margins) if m <= floor), len(margins))
        assert list(gen[b, :low]) == toks[:low], (b, low)
        assert list(grd[b, :low]) == toks[:low], (b, low)
        total += low
    assert total >= 8, total
    eng.close()


def _ranking(case):
    from llmrankers.rankers import SearchResult
    return [SearchResult(docid=d, score=None, text=t) for d, t in case["docs"]]


@pytest.fixture(scope="module")
def lw_stack(lw_ckpt):
    from transformers import T5Tokenizer
    from llmrankers._runtime import T5Runtime
    return T5Runtime(lw_ckpt, "cuda", max_tokens=8192, max_seqs=32, max_dec_len=24), T5Tokenizer.from_pretrained(lw_ckpt)


def test_listwise_golden_cases_on_the_engine(gold, lw_stack):
    from llmrankers.listwise import ListwiseLlmRanker
    rt, tok = lw_stack
    assert gold["min_margin"] > MARGIN_FLOOR
    for case in gold["cases"]:
        rk = ListwiseLlmRanker.from_runtime(rt, tok, window_size=case["window_size"], step_size=case["step_size"],
                                            scoring=case["scoring"], num_repeat=case["num_repeat"], max_new=gold["max_new"])
        outs = []
        real = rk.compare
        rk.compare = lambda q, docs: outs.append(real(q, docs)) or outs[-1]
        ranking = _ranking(case)
        res = rk.rerank(case["query"], ranking)
        tag = (case["scoring"], case["qid"])
        assert outs == [c["output"] for c in case["compares"]], tag
        assert [d.docid for d in res] == case["docids"] and [d.score for d in res] == case["scores"], tag
        assert [d.docid for d in ranking] == [d for d, _ in case["docs"]], tag
        assert [rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens] == case["counters"], tag
    # lockstep = one query at a time.  generation: every query of the fixture (rows of rk_t5_generate are batch-independent bit for
    # bit, whatever the windows); likelihood: the recorded walk itself, three times (a few-row rk_t5_score call and a larger one
    # differ in the last bits - DESIGN.md section 4 - so equality is demanded where the recorded margins clear the floor)
    for scoring in ("generation", "likelihood"):
        case = next(c for c in gold["cases"] if c["scoring"] == scoring and c["window_size"] == 4)
        rk = ListwiseLlmRanker.from_runtime(rt, tok, window_size=4, step_size=2, scoring=scoring, num_repeat=2, max_new=gold["max_new"])
        pool = [c for c in gold["cases"] if c["scoring"] == scoring] if scoring == "generation" else [case]
        items = [(c["query"], _ranking(c)) for c in pool] * 3
        want, wc = [], []
        for q, r in copy.deepcopy(items):
            want.append([(d.docid, d.score) for d in rk.rerank(q, r)])
            wc.append((rk.total_compare, rk.total_prompt_tokens, rk.total_completion_tokens))
        got, counters = rk.rerank_many(items)
        assert [[(d.docid, d.score) for d in res] for res in got] == want, scoring
        assert counters == wc, scoring
        assert [d.docid for d in got[pool.index(case)]] == case["docids"], scoring


def test_run_py_listwise_on_the_engine(gold, lw_ckpt, tmp_path):
    """run.py ... listwise --window_size 4 --step_size 2 --num_repeat 2 on the engine: the reference's recorded ranking for that
    case, and the same run file one query at a time as in lockstep"""
    import importlib.util
    from conftest import REPO
    spec = importlib.util.spec_from_file_location("rk_run_lw_gpu", os.path.join(REPO, "run.py"))
    runmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(runmod)
    case = next(c for c in gold["cases"] if c["scoring"] == "generation" and c["window_size"] == 4)
    lik = next(c for c in gold["cases"] if c["scoring"] == "likelihood" and c["window_size"] == 4)
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
    lik_run = run(tmp_path / "lik.trec", ["--scoring", "likelihood"])
    rows = [l.split() for l in lik_run.splitlines() if l.split()[0] == case["qid"]]
    assert lik["qid"] == case["qid"] and [r[2] for r in rows] == lik["docids"]
