"""The one rule for values derived from tensors (derived.py): a value is valid while the very same tensor object sits at the same
version; a new version replaces the entry; a dead source takes its entry with it.  CPU tensors only, no library."""
import gc
import weakref

import torch


class _Make:
    """A `make` that counts its calls and returns a fresh object each time."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return ["value", self.calls]


def test_hit_returns_the_same_object(pkg):
    c, make, W = pkg.derived.Cache(16), _Make(), torch.ones(4, 4)
    a = c.get((W,), "k", make)
    assert c.get((W,), "k", make) is a and make.calls == 1 and len(c) == 1


def test_new_version_replaces_the_entry(pkg):
    c, make, W = pkg.derived.Cache(16), _Make(), torch.zeros(4, 4)
    for i in range(300):
        W.add_(1)
        assert c.get((W,), "k", make) == ["value", i + 1]
        assert len(c) == 1
    assert make.calls == 300


def test_views_share_by_geometry_not_by_object(pkg):
    c, make, var = pkg.derived.Cache(16), _Make(), torch.randn(32, 8)
    a = c.get((var.view(4, 8, 8),), "k", make)
    assert c.get((var.view(4, 8, 8),), "k", make) is a and make.calls == 1
    lo = c.get((var[:16].view(2, 8, 8),), "k", make)
    hi = c.get((var[16:].view(2, 8, 8),), "k", make)
    assert lo is not hi and lo is not a and make.calls == 3 and len(c) == 3


def test_other_strides_are_another_entry(pkg):
    c, make, W = pkg.derived.Cache(16), _Make(), torch.randn(4, 8, 8)
    a = c.get((W,), "k", make)
    b = c.get((W.transpose(1, 2),), "k", make)
    assert a is not b and make.calls == 2
    assert c.get((W,), "k", make) is a and c.get((W.transpose(1, 2),), "k", make) is b and make.calls == 2


def test_other_extra_is_another_entry(pkg):
    c, make, W = pkg.derived.Cache(16), _Make(), torch.randn(4, 4)
    a, b = c.get((W,), ("edge", 2), make), c.get((W,), ("edge", 3), make)
    assert a is not b and make.calls == 2 and c.get((W,), ("edge", 2), make) is a and make.calls == 2


def test_two_sources_and_plain_values(pkg):
    c, a, b = pkg.derived.Cache(16), torch.ones(3), torch.ones(3)
    assert c.lookup((a, b), "ok") is None
    assert c.store((a, b), "ok", False) is False and c.lookup((a, b), "ok") is False      # (a stored False is a hit)
    assert c.lookup((b, a), "ok") is None
    b.add_(1)
    assert c.lookup((a, b), "ok") is None


def test_dead_sources_leave_and_live_ones_stay(pkg):
    """An entry goes the moment a source of it dies (the weak reference's callback; derived.py scans nothing, so there is no
    amortisation slack): the table never holds more than the live sources' entries."""
    c, make = pkg.derived.Cache(1024), _Make()
    live = [torch.full((4,), float(i)) for i in range(3)]
    first = [c.get((t,), "k", make) for t in live]
    for i in range(500):
        t = torch.full((4,), float(i))
        c.get((t,), "k", make)
        assert len(c) <= len(live) + 1
        del t
        assert len(c) <= len(live)
    assert make.calls == 503
    assert all(c.get((t,), "k", make) is v for t, v in zip(live, first)) and make.calls == 503


def test_a_cache_nobody_holds_frees_its_values_at_once(pkg):
    c, W = pkg.derived.Cache(16), torch.ones(4)
    value = weakref.ref(c.get((W,), "k", lambda: torch.zeros(4)))
    assert value() is not None
    del c                                    # (no reference cycle through the sources' callbacks: no wait for the collector)
    assert value() is None and W.sum() == 4


def test_a_recycled_id_never_hits(pkg):
    c, make = pkg.derived.Cache(16), _Make()
    for i in range(50):                      # the allocator hands the same address (and CPython the same id) out again
        t = torch.zeros(4)
        c.get((t,), "k", make)
        assert make.calls == i + 1
        del t
    assert len(c) == 0


def test_cap_clears_and_still_answers(pkg):
    c, make = pkg.derived.Cache(8), _Make()
    live = [torch.full((4,), float(i)) for i in range(9)]
    vals = [c.get((t,), "k", make) for t in live]
    assert vals == [["value", i + 1] for i in range(9)] and len(c) <= 8
    for t in live:                           # every get answers: a hit, or a fresh make of the same thing
        n = make.calls
        v = c.get((t,), "k", make)
        assert v[0] == "value" and make.calls in (n, n + 1) and c.get((t,), "k", make) is v
    assert len(c) <= 8


def test_maxima_are_measured_in_one_call_per_request(pkg, monkeypatch):
    f = pkg.formats
    calls = []
    real = f.absmax
    monkeypatch.setattr(f, "absmax", lambda ts: calls.append(len(ts)) or real(ts))
    t0, t1, t2 = torch.tensor([1.0, -4.0]), torch.tensor([[0.5, 2.0]]), torch.tensor([-7.0])
    assert f.weight_absmax([t0, t1, t2]) == [float(t.abs().max()) for t in (t0, t1, t2)] and calls == [3]
    assert f.weight_absmax([t0, t1, t2]) == [4.0, 2.0, 7.0] and calls == [3]
    t1.mul_(2)
    assert f.weight_absmax([t0, t1, t2]) == [4.0, float(t1.abs().max()), 7.0] == [4.0, 4.0, 7.0] and calls == [3, 1]


def test_stamps(pkg):
    d = pkg.derived
    t = torch.ones(4)
    s = d.stamp(t)
    assert d.stamp_holds(s, t) and not d.stamp_holds(None, t)
    assert not d.stamp_holds(s, torch.ones(4))               # an equal-valued other tensor
    assert not d.stamp_holds(s, t.view(4))                   # (the object, not its base)
    t.add_(1)
    assert not d.stamp_holds(s, t)


def test_transposed_is_shared_by_views_and_replaced_on_a_new_version(pkg):
    b = pkg.backward
    var = torch.randn(32, 8)
    Wt = b.transposed(var.view(4, 8, 8), (1, 2))
    assert torch.equal(Wt, var.view(4, 8, 8).transpose(1, 2).contiguous()) and Wt.is_contiguous()
    assert b.transposed(var.view(4, 8, 8), (1, 2)) is Wt
    assert torch.equal(b.transposed(var), var.t().contiguous())
    old = weakref.ref(Wt)
    del Wt
    var.add_(1)
    new = b.transposed(var.view(4, 8, 8), (1, 2))
    assert torch.equal(new, var.view(4, 8, 8).transpose(1, 2).contiguous())
    gc.collect()
    assert old() is None                                     # the stale transpose is not kept
