"""Advance independent dependency chains together: the one loop behind every "several compares per engine call" path.

A chain is a generator that yields a list of windows whose compares do not depend on each other, is sent their labels (one
per window, in order) and may return a value.  The windows of ONE chain depend on the labels before them; different chains do
not know of each other, so their pending windows can share an engine call.  The driver only moves windows and labels: which
call answers them, and any counting, is the caller's business.
"""


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
