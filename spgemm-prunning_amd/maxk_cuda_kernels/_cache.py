"""The one cache the binding keeps per-graph work in: plans, range checks, scaled entries.

An entry belongs to the tensor *objects* it was built from and to the contents they had then:
it is found by their id()s, trusted only while each is still that object at that version
counter, and dropped when any of them dies.
"""
from __future__ import annotations

import weakref


class TensorCache:
    """build() results keyed on the identity of `tensors` plus the hashables `extra`."""

    def __init__(self):
        self._entries: dict = {}

    def __len__(self) -> int:
        return len(self._entries)

    def lookup(self, tensors: tuple, extra: tuple):
        """The value kept for these tensor objects (at their current versions) and `extra`,
        or None."""
        hit = self._entries.get((*map(id, tensors), *extra))
        if hit is not None:
            refs, versions, value = hit
            for ref, version, t in zip(refs, versions, tensors):
                # the weakref tells a live key tensor from a new one at a recycled id()
                if ref() is not t or version != t._version:
                    return None
            return value
        return None

    def get(self, tensors: tuple, extra: tuple, build, use: bool = True):
        """lookup(), and on a miss the value of build() (never None), which is kept.
        use=False only calls build(): no lookup, no entry."""
        if not use:
            return build()
        value = self.lookup(tensors, extra)
        if value is not None:
            return value
        value = build()
        # Inference tensors have no version counter (reading it raises), so nothing is kept on
        # one: the plan or check is redone per call, which is always correct.
        if any(t.is_inference() for t in tensors):
            return value
        key = (*map(id, tensors), *extra)
        if key not in self._entries:  # else every key tensor already carries the finalizer
            for t in tensors:
                weakref.finalize(t, self._entries.pop, key, None)
        self._entries[key] = (tuple(map(weakref.ref, tensors)),
                              tuple(t._version for t in tensors), value)
        return value
