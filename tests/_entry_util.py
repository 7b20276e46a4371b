"""What the entry-sequence tests share (test_gpu_entry_sequence.py, test_gpu_llama_entry_sequence.py): the order of the calls and
the form their results are compared in."""
import numpy as np


def _each_after_each(n):
    """n * n + 1 kinds out of 0 .. n-1 in which every kind directly follows every kind (itself included) exactly once: an
    Euler circuit of the complete directed graph with loops (Hierholzer)."""
    out = [list(range(n)) for _ in range(n)]
    stack, circuit = [0], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def _bytes(res):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (res if isinstance(res, tuple) else (res,)))
