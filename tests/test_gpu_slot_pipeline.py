"""The two-slot pipeline of the T5 engine (csrc/rk_engine.hip: the table at Slot): an encoder chain starts while the decoder of the
slot's previous launch still runs and waits for it only in front of the buffers that decoder reads; a slot is staged again without
waiting for its decoder (two generations of the staged arrays).  Everything here is bit for bit against blocking calls of the same
batches: the pipeline changes when kernels run, never what they compute.  Toy checkpoint: its encoder is short and its decoder
latency-bound, so a slot's next encoder reaches its last kernels while the previous decoder is still running."""
import numpy as np
import pytest

from conftest import load_state

pytestmark = pytest.mark.gpu
IDS = [21, 22]
RK_ERR_INVALID, RK_ERR_STATE, RK_ERR_CAPACITY = -1, -4, -6
# decoder prefixes: one position, two, and 17 (> XA_MAX_LD = 16: the encoder materialises the cross-attention K / V)
DEC = {1: [0], 2: [0, 7], 17: [0] + [5 + 3 * i for i in range(16)]}
N_SEQ = (3, 16, 1, 9, 16, 2, 11, 5)                       # one launch each, alternating over the two slots
N_TWINS = 5                                               # batches 8 .. 12: the lengths of batch 1 (16 sequences), other tokens


def _engine(dims, state, **kw):
    from llmrankers._engine import RkEngine
    return RkEngine(dims, device=0, **kw).load_state(state.items())


@pytest.fixture(scope="module")
def toy(ckpt_dirs):
    """(dims, state, {enc_serial: engine}): one engine per setting of the option, so that none is ever left in the other one."""
    dims, state = load_state(ckpt_dirs["ckpt_gated_untied"])
    engs = {v: _engine(dims, state, max_tokens=4096, max_seqs=64, max_dec_len=40) for v in (0, 1)}
    engs[1].set_option("enc_serial", 1)
    yield dims, state, engs
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def batches(toy):
    from llmrankers import _synth
    dims = toy[0]
    out = [_synth.synth_token_batch(n, 3, 120, dims.vocab, seed=700 + i) for i, n in enumerate(N_SEQ)]
    for k in range(N_TWINS):
        rs = np.random.RandomState(800 + k)
        twin = [rs.randint(3, dims.vocab - 28, size=len(s)).astype(np.int32) for s in out[1]]
        for t in twin:
            t[-1] = 1
        out.append(twin)
    return out


@pytest.fixture(scope="module")
def blocking(toy, batches):
    """dec_len -> the blocking score() of every batch, computed once (the option under test does not reach a blocking call)."""
    eng, memo = toy[2][0], {}

    def get(dec_len):
        if dec_len not in memo:
            memo[dec_len] = [eng.score(b, DEC[dec_len], IDS) for b in batches]
        return memo[dec_len]
    return get


@pytest.mark.parametrize("enc_serial", [0, 1])
@pytest.mark.parametrize("dec_len", [1, 2, 17])
def test_restaged_launches_over_both_slots_match_blocking_calls(toy, batches, blocking, dec_len, enc_serial):
    """Eight launches, every one staged with other tokens, lengths and n_seq, no sync() anywhere: a slot's scores are read just
    before the slot is staged again, the last two at the end.  (Every launch here has another n_seq than the slot's previous one,
    so its index buffers are uploaded again and the launch itself waits for the slot's decoder: this is the re-staging with
    changing shapes.  The launches that overtake a running decoder are the two tests below.)"""
    eng = toy[2][enc_serial]
    want = blocking(dec_len)
    got = [None] * len(N_SEQ)
    for i, b in enumerate(batches[:len(N_SEQ)]):
        slot = i % 2
        if i >= 2:
            got[i - 2] = eng.read_scores(slot)
        eng.stage(b, slot=slot)
        eng.score_staged(DEC[dec_len], IDS, slot=slot)
    for i in (len(N_SEQ) - 2, len(N_SEQ) - 1):
        got[i] = eng.read_scores(i % 2)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (N_SEQ[i], len(IDS))
        np.testing.assert_array_equal(g, w, err_msg=f"launch {i} (slot {i % 2}, n_seq {N_SEQ[i]})")


def _launch_appended(eng, batches, plan, dec_len):
    """stage + score + append for every (slot, batch index) of `plan`, nothing read in between; one gather -> the flat scores"""
    off = 0
    for slot, i in plan:
        eng.stage(batches[i], slot=slot)
        eng.score_staged(DEC[dec_len], IDS, slot=slot)
        n = len(batches[i]) * len(IDS)
        eng.comm_append(n, off, slot=slot)
        off += n
    return eng.comm_all_gather_appended(off)[0]


@pytest.mark.parametrize("enc_serial", [0, 1])
@pytest.mark.parametrize("dec_len", [1, 17])
def test_scores_consumed_on_the_device_survive_the_next_encoder(toy, batches, blocking, dec_len, enc_serial):
    """What the narrowed wait is for: slot 0, slot 1, slot 0 again with new tokens, each launch's scores appended to the send
    buffer on the device and nothing read in between - the third launch's encoder must not overwrite enc_out / cross_kv / the
    decoder's offsets under the first launch's decoder.  One gather at the end; all three blocks are the blocking calls' bits.
    The two launches of slot 0 MUST have the same n_seq, lengths, decoder prefix and output ids (batch 1 and a twin of it): then
    the second one uploads no index buffer and does not wait on the host for the first one's decoder (DecIndex::put) - with
    another shape the host itself would order the two.  Four rounds: a slot's decoder chain is replayed as a graph from its third
    sighting on.  This is the sequence of a sharded query's chunks; with 16 sequences the toy decoder is through before the host
    has enqueued two more encoder chains, so the window is narrow here - test_back_to_back_launches_on_one_slot_under_a_long_decoder
    is the one that fails on this checkpoint when wait_prev_decoder is taken out."""
    eng = toy[2][enc_serial]
    plan = ((0, 1), (1, 6), (0, 8))
    want = np.concatenate([blocking(dec_len)[i].reshape(-1) for _, i in plan])
    eng.comm_init(eng.comm_unique_id(), 0, 1, 256)
    try:
        for rnd in range(4):
            np.testing.assert_array_equal(_launch_appended(eng, batches, plan, dec_len), want, err_msg=f"round {rnd}")
    finally:
        eng.comm_destroy()


@pytest.mark.parametrize("enc_serial", [0, 1])
@pytest.mark.parametrize("dec_len", [1, 17])
def test_a_stream_of_equal_shapes_is_restaged_under_launches_in_flight(toy, batches, blocking, dec_len, enc_serial):
    """The pipeline as a stream of full calls drives it: six launches over both slots, all of one shape and every one staged with
    other tokens, no read and no sync in between - every staging writes the generation beside the one the slot's launch in
    flight reads, every launch overtakes the host (no index upload), and every score block is consumed on the device."""
    eng = toy[2][enc_serial]
    plan = tuple((k % 2, i) for k, i in enumerate((1, 8, 9, 10, 11, 12)))
    want = np.concatenate([blocking(dec_len)[i].reshape(-1) for _, i in plan])
    eng.comm_init(eng.comm_unique_id(), 0, 1, 256)
    try:
        for rnd in range(3):
            np.testing.assert_array_equal(_launch_appended(eng, batches, plan, dec_len), want, err_msg=f"round {rnd}")
    finally:
        eng.comm_destroy()


def test_back_to_back_launches_on_one_slot_under_a_long_decoder(toy):
    """The widest window the toy checkpoint gives the hazard: 64 short sequences (an encoder of a few microseconds per kernel) and
    40 decoder positions over the materialised K / V (2 560 decoder rows), four launches of ONE shape back to back on ONE slot,
    then the other, nothing read in between.  The host enqueues an encoder chain faster than the GPU replays the decoder graph in
    front of it, so every encoder chain reaches its last kernels while the slot's previous decoder is still running."""
    from llmrankers import _synth
    dims, _, engs = toy
    dec = [0] + [4 + 2 * i for i in range(39)]
    base = _synth.synth_token_batch(64, 3, 12, dims.vocab, seed=990)
    fam = [base]
    for k in range(3):
        rs = np.random.RandomState(991 + k)
        fam.append([np.concatenate([rs.randint(3, dims.vocab - 28, size=len(s) - 1), [1]]).astype(np.int32) for s in base])
    want = np.concatenate([engs[0].score(b, dec, IDS).reshape(-1) for b in fam])
    for v, eng in engs.items():
        eng.comm_init(eng.comm_unique_id(), 0, 1, 1024)
        try:
            for rnd in range(4):
                slot = rnd % 2
                off = 0
                for b in fam:
                    eng.stage(b, slot=slot)
                    eng.score_staged(dec, IDS, slot=slot)
                    eng.comm_append(len(b) * len(IDS), off, slot=slot)
                    off += len(b) * len(IDS)
                np.testing.assert_array_equal(eng.comm_all_gather_appended(off)[0], want, err_msg=f"enc_serial {v} round {rnd}")
        finally:
            eng.comm_destroy()


def test_staging_twice_without_a_launch_keeps_the_last_batch(toy, batches, blocking):
    """A slot staged twice in a row holds the second batch - with nothing in flight, and behind a launch that is still running,
    whose scores stay what they were."""
    import ctypes as C
    eng = toy[2][0]
    want = blocking(1)
    for slot in (0, 1):
        eng.stage(batches[0], slot=slot)
        eng.stage(batches[3], slot=slot)
        eng.score_staged(DEC[1], IDS, slot=slot)           # batch 3 in flight
        eng.stage(batches[1], slot=slot)
        eng.stage(batches[6], slot=slot)
        # (RkEngine.read_scores takes its shape from the last staging: the launch in flight is read through the C ABI)
        out = np.empty((N_SEQ[3], len(IDS)), dtype=np.float32)
        eng._chk(eng.lib.rk_t5_read_scores_slot(eng.h, slot, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        np.testing.assert_array_equal(out, want[3])
        eng.score_staged(DEC[1], IDS, slot=slot)
        np.testing.assert_array_equal(eng.read_scores(slot), want[6])


def test_staging_at_capacity_and_its_refusals(toy):
    """max_seqs sequences of max_tokens tokens in all, through both slots and both generations; one sequence or one token more is
    RK_ERR_CAPACITY, an empty sequence RK_ERR_INVALID, a launch behind a refused staging RK_ERR_STATE - and neither disturbs the
    launch in flight nor the slot's next staging."""
    from llmrankers import _synth
    from llmrankers._engine import RkError
    dims, state, _ = toy
    eng = _engine(dims, state, max_tokens=512, max_seqs=16, max_dec_len=4)
    try:
        full = [_synth.synth_token_batch(16, 32, 32, dims.vocab, seed=900 + i) for i in range(4)]
        want = [eng.score(b, DEC[1], IDS) for b in full]
        got = []
        for i, b in enumerate(full):
            if i >= 2:
                got.append(eng.read_scores(i % 2))
            eng.stage(b, slot=i % 2)
            eng.score_staged(DEC[1], IDS, slot=i % 2)
        # slot 0 and slot 1 are in flight (batches 2 and 3)
        for bad, code in ((full[0] + [full[0][0]], RK_ERR_CAPACITY), (full[0][:15] + [list(full[0][15]) + [1]], RK_ERR_CAPACITY),
                          ([[1, 2], []], RK_ERR_INVALID), ([[1, dims.vocab]], RK_ERR_INVALID)):
            with pytest.raises(RkError) as ei:
                eng.stage(bad, slot=0)
            assert ei.value.code == code, (ei.value.code, code)
            with pytest.raises(RkError) as ei:
                eng.score_staged(DEC[1], IDS, slot=0)
            assert ei.value.code == RK_ERR_STATE
        got += [eng.read_scores(0), eng.read_scores(1)]
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        eng.stage(full[1], slot=0)
        eng.score_staged(DEC[1], IDS, slot=0)
        np.testing.assert_array_equal(eng.read_scores(0), want[1])
    finally:
        eng.close()
