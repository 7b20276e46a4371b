"""Advance independent dependency chains together: the one loop behind every "several compares per engine call" path.

A chain is a generator that yields a list of windows whose compares do not depend on each other, is sent their labels (one
per window, in order) and may return a value.  The windows of ONE chain depend on the labels before them; different chains do
not know of each other, so their pending windows can share an engine call.  The driver only moves windows and labels: which
call answers them, and any counting, is the caller's business.

`drive` runs one chain alone, `Lockstep` advances several together, `heapsort_steps` is the heapsort of every sorting ranker as
such a chain, and `alternate` runs two groups of chains over an engine's two batch slots.
"""


def drive(steps, answer):
    """Run ONE chain to its end: every yielded list of windows goes through `answer(windows) -> answers`; -> its return value."""
    answers = None
    while True:
        try:
            windows = steps.send(answers)
        except StopIteration as stop:
            return stop.value
        answers = answer(windows)


class Lockstep:
    def __init__(self, chains):
        """chains: {key: generator}; every chain is run to its first yield, in sorted key order."""
        self._chains = dict(chains)
        self._pending = {}                  # live chains only: key -> the windows it waits for
        self.returned = {}                  # finished chains: key -> the generator's return value
        for key in sorted(self._chains):
            self._step(key, None)

    def _step(self, key, labels):
        try:
            self._pending[key] = self._chains[key].send(labels)
        except StopIteration as stop:
            self.returned[key] = stop.value

    def __bool__(self):
        return bool(self._pending)

    def live(self):
        return sorted(self._pending)

    def pending(self):
        """-> (keys, windows): the pending windows of all live chains, chains in sorted key order; keys[i] owns windows[i]."""
        order = self.live()
        return [key for key in order for _ in self._pending[key]], [w for key in order for w in self._pending[key]]

    def advance(self, labels):
        """labels[i] answers pending()'s windows[i]: every chain is sent its slice and runs to its next yield or its end."""
        waiting, self._pending = self._pending, {}
        pos = 0
        for key in sorted(waiting):
            n = len(waiting[key])
            self._step(key, labels[pos:pos + n])
            pos += n

    def absorb(self, other, keys=None):
        """Take over live chains of another driver (all of them, or `keys`) with their pending windows, and what it collected."""
        for key in other.live() if keys is None else keys:
            self._chains[key] = other._chains.pop(key)
            self._pending[key] = other._pending.pop(key)
        self.returned.update(other.returned)


def heapsort_steps(arr, k, arity, sift, level_batched):
    """The heapsort of the sorting rankers (ref: setwise.py:219-232, pairwise.py:149-162) over an `arity`-ary max-heap, in place;
    `sift(arr, n, i)` is the ranker's sift-down of node i of arr[:n], itself a chain.  The build phase sifts the nodes
    n // arity .. 0.  Reference order: one after another.  Level order: that walk goes level by level from the deepest one, and
    the nodes of a level root disjoint subtrees, so their sift-downs touch disjoint array slots and commute - they advance in
    lock step, one list of windows per step: the array, the set of compares and every counter end up identical, only the order
    of compares inside a level differs.  Extraction is a chain: one sift-down after another, until k documents are ranked."""
    n = len(arr)
    if level_batched:
        levels, first, width = [], 0, 1                       # the nodes of depth d occupy [first, first + arity^d)
        while first <= n // arity:
            levels.append(range(min(first + width - 1, n // arity), first - 1, -1))
            first, width = first + width, width * arity
        for level in reversed(levels):
            build = Lockstep({j: sift(arr, n, i) for j, i in enumerate(level)})
            while build:
                build.advance((yield build.pending()[1]))
    else:
        for i in range(n // arity, -1, -1):
            yield from sift(arr, n, i)
    ranked = 0
    for m in range(n - 1, 0, -1):
        arr[m], arr[0] = arr[0], arr[m]
        ranked += 1
        if ranked == k:
            break
        yield from sift(arr, m, 0)


def alternate(chains, launch, collect, blocking):
    """Run the live chains of `chains` (a Lockstep) to their ends as two groups that alternate over an engine's batch slots 0
    and 1: while one group's call is on the GPU the host advances the other group's chains, builds its next call and launches
    it.  The chains are dealt to the groups round-robin in sorted key order, and the turns go 0, 1, 0, 1, ...  At group g's turn
    its call in flight (if any) is collected first, `collect(keys, launched) -> answers`; its pending windows then go out through
    `launch(keys, windows, slot=g)`, which returns at once with whatever `collect` needs.  A launch that returns None did not fit
    one engine call: the other group's call is collected too, THIS round of this group is answered by `blocking(keys, windows)
    -> answers`, and the next round is launched as usual.  Nothing else runs on the engine while a slot is in flight (the
    contract of a runtime's asynchronous calls), so when anything raises, every call still in flight is collected once, its own
    errors swallowed, before the exception leaves.  At the end the chains (all finished) are handed back to `chains`."""
    groups = [Lockstep({}), Lockstep({})]
    for i, key in enumerate(chains.live()):
        groups[i % 2].absorb(chains, [key])
    inflight = {}                                             # group -> (keys, launched): at most one call per slot

    def settle(g):
        keys, launched = inflight.pop(g)
        groups[g].advance(collect(keys, launched))

    try:
        while groups[0] or groups[1]:
            for g in (0, 1):
                if g in inflight:
                    settle(g)
                if not groups[g]:
                    continue
                keys, windows = groups[g].pending()
                launched = launch(keys, windows, slot=g)
                if launched is not None:
                    inflight[g] = (keys, launched)
                    continue
                if 1 - g in inflight:
                    settle(1 - g)
                groups[g].advance(blocking(keys, windows))
    finally:
        for keys, launched in inflight.values():
            try:
                collect(keys, launched)
            except Exception:
                pass
    for group in groups:
        chains.absorb(group)
