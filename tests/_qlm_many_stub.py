"""Test doubles for grouped qlm (PointwiseLlmRanker.rerank_many -> qlm_many): the runtimes of tests/_stub.py plus the
per-sequence-label call, recorded.  Every sequence is scored on the fp32 oracle ONE AT A TIME, so what a double returns
cannot depend on how the ranker batches."""
import numpy as np

from _stub import FakeCommEngine, OracleRuntime


def _one_at_a_time(orc, seqs, labels_per_seq):
    assert len(seqs) == len(labels_per_seq)
    return np.asarray([orc.qlm([s], l)[0] for s, l in zip(seqs, labels_per_seq)], dtype=np.float32)


class RecordingQlmManyRuntime(OracleRuntime):
    """OracleRuntime + qlm_many; keeps every call's arguments."""

    def __init__(self, dims, state):
        super().__init__(dims, state)
        self.qlm_calls, self.qlm_many_calls = [], []

    def qlm(self, seqs, labels):
        self.qlm_calls.append(([list(s) for s in seqs], list(labels)))
        return super().qlm(seqs, labels)

    def qlm_many(self, seqs, labels_per_seq):
        self.qlm_many_calls.append(([list(s) for s in seqs], [list(l) for l in labels_per_seq]))
        return _one_at_a_time(self.orc, seqs, labels_per_seq)


class FakeCommEngineQlmMany(FakeCommEngine):
    """FakeCommEngine + the engine-level qlm_many (rk_t5_qlm_many): scores left in 'slot 0' like every blocking call."""

    def qlm_many(self, seqs, labels_per_seq):
        assert 0 < len(seqs) <= self.desc.max_seqs
        self.calls["qlm_many"] = self.calls.get("qlm_many", 0) + 1
        out = _one_at_a_time(self.orc, seqs, labels_per_seq)
        self._last = out.reshape(-1).copy()
        return out
