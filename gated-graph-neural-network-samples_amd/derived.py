"""Values derived from tensors -- stage images of weights, transposes, dropout masks, maxima -- and the ONE rule by which they
stay good: a derived value is valid while the very same tensor object sits at the same version.

Key     per source tensor (id(base), data_ptr, shape, stride), base = t._base or t (views share their base's version counter),
        then the caller's hashable `extra` (kind, format, nx, dims ...).  The version is not in the key: a new version REPLACES
        the entry.
Valid   every stored weak reference resolves to the very same base object and every source's _version equals the stored one: a
        pointer or an id recycled by the allocator for another model's weights never hits.
Values  a CUDA tensor carries an event recorded after `make` on the stream that made it; a hit from another stream waits for the
        event on the device (no host synchronisation) and records the stream on the tensor.  Anything else is stored as it is.
Evict   an entry goes the moment one of its sources dies (the weak reference's callback: no scan of the table, ever, and a chain
        such as variable -> masked copy -> image unravels by itself); a live tensor's entry stays until the table reaches its cap,
        at which the whole table is cleared.  So the table changes not only inside store(): the callback runs in whatever thread
        or collector pass drops a source's last reference.  It removes only the entry its own reference guards; its get-then-pop is
        not atomic against a store() under the same key from another thread, and the worst that costs is one spurious miss.

This module imports nothing of the package: ops, backward, formats and autograd import it.
"""
from __future__ import annotations

import weakref
from typing import Any, Callable, Hashable, Sequence

import torch


def stamp(t: torch.Tensor):
    """The identity and version of the tensor OBJECT t (not of its base), to be kept next to a statement about t."""
    return (weakref.ref(t), t._version)


def stamp_holds(s, t: torch.Tensor) -> bool:
    """Whether the stamp `s` (or None) was taken of this very object at its present version."""
    return s is not None and s[0]() is t and s[1] == t._version


class _SourceRef(weakref.ref):
    """The weak reference to a source's base, which knows the entry it guards: one callback serves every entry of every cache."""
    __slots__ = ("cache", "key")


def _source_died(ref: _SourceRef):
    cache = ref.cache()                                      # (weak: a cache nobody holds goes at once, values included)
    if cache is not None:
        entry = cache._t.get(ref.key)
        if entry is not None and any(r is ref for r in entry[0]):   # (this entry, not a later one under the same key)
            cache._t.pop(ref.key, None)


class Cache:
    def __init__(self, cap: int):
        self.cap = cap
        self._t = {}
        self._weak_self = weakref.ref(self)

    def __len__(self):
        return len(self._t)

    @staticmethod
    def _identify(sources: Sequence[torch.Tensor], extra: Hashable):
        """The sources' bases and the key, worked out once per request."""
        bases, key = [], [extra]
        for t in sources:
            b = t._base
            if b is None:
                b = t
            bases.append(b)
            key.append((id(b), t.data_ptr(), t.shape, t.stride()))
        return bases, tuple(key)

    def _lookup(self, key, bases, sources):
        entry = self._t.get(key)
        if entry is None:
            return None
        refs, versions, value, ready, stream_id = entry
        for r, v, b, t in zip(refs, versions, bases, sources):
            if r() is not b or v != t._version:
                return None
        # the value was written on another stream: order this stream after the launch that made it (an event wait on the device --
        # a host synchronisation here used to drain the GPU queue once per layer and training step)
        if ready is not None:
            cur = torch.cuda.current_stream()
            if cur.cuda_stream != stream_id:
                if not ready.query():
                    cur.wait_event(ready)
                value.record_stream(cur)                     # (its memory belongs to the making stream's pool)
        return value

    def _store(self, key, bases, sources, value):
        if len(self._t) >= self.cap:
            self._t.clear()
        ready, stream_id = None, 0
        if isinstance(value, torch.Tensor) and value.is_cuda:
            ready = torch.cuda.Event()
            ready.record()                                   # after the launch of `make`, on the stream that ran it
            stream_id = torch.cuda.current_stream().cuda_stream
        refs = []
        for b in bases:
            r = _SourceRef(b, _source_died)
            r.cache, r.key = self._weak_self, key
            refs.append(r)
        self._t[key] = (refs, [t._version for t in sources], value, ready, stream_id)
        return value

    def lookup(self, sources: Sequence[torch.Tensor], extra: Hashable = ()):
        """The value stored for these sources at their present versions, or None."""
        bases, key = self._identify(sources, extra)
        return self._lookup(key, bases, sources)

    def store(self, sources: Sequence[torch.Tensor], extra: Hashable, value: Any):
        bases, key = self._identify(sources, extra)
        return self._store(key, bases, sources, value)

    def get(self, sources: Sequence[torch.Tensor], extra: Hashable, make: Callable[[], Any]):
        bases, key = self._identify(sources, extra)
        hit = self._lookup(key, bases, sources)
        return self._store(key, bases, sources, make()) if hit is None else hit
