"""deeplip_amd/train_loop.py on the host (no GPU): the ring of cached batches, the prefetch's CPU pass-through, the epoch's metrics
and the order of an optimisation step's calls."""
import types

import torch

from deeplip_amd import train_loop as tl


def test_batch_ring_makes_each_cached_batch_once_and_walks_them_cyclically():
    made = []

    def make(k):
        made.append(k)
        return object()
    ring = tl.BatchRing(make, 2)
    got = [ring.get(i) for i in range(5)]
    assert made == [0, 1]
    assert got[2] is got[0] and got[4] is got[0] and got[3] is got[1] and got[0] is not got[1]


def test_batch_ring_without_a_cache_makes_every_batch():
    made = []
    ring = tl.BatchRing(lambda i: made.append(i) or object(), 0)
    got = [ring.get(i) for i in range(5)]
    assert made == [0, 1, 2, 3, 4] and len({id(g) for g in got}) == 5


def test_batch_ring_hands_the_callers_arguments_to_make():
    ring = tl.BatchRing(lambda k, rng, ladder: (k, rng, ladder), 2)
    assert ring.get(3, "rng", [60]) == (1, "rng", [60]) and ring.get(1, "other", [72]) == (1, "rng", [60])      # cached: made once


def test_prefetch_on_the_cpu_hands_the_batch_back_by_name():
    pf = tl.Prefetch(torch.device("cpu"))
    assert pf.stream is None
    lengths = [5, 3]
    host = {"x": torch.arange(6.0).reshape(2, 3), "lab": torch.tensor([1, 0]), "lengths": lengths, "names": ("a", "b")}
    got = pf.take(pf.stage(host))
    assert sorted(got) == sorted(host)
    assert torch.equal(got["x"], host["x"]) and torch.equal(got["lab"], host["lab"])
    assert got["lengths"] is lengths and got["names"] == ("a", "b")


def test_epoch_meter_sums_exactly_in_float64():
    m = tl.EpochMeter(torch.device("cpu"))
    m.add(torch.tensor(0.5), torch.tensor(3), 8)                      # an integer count, as (pred == labels).sum() is
    m.add(torch.tensor(0.25, requires_grad=True), torch.tensor(2.5, dtype=torch.float64), 4)      # a weighted one, as mixup's is
    m.add(torch.tensor(2.0), 1, 2)
    assert m.acc.dtype == torch.float64
    assert m.read() == [0.5 * 8 + 0.25 * 4 + 2.0 * 2, 3 + 2.5 + 1, 14.0]


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **kw: self.calls.append((name, kw) if kw else name)


class _Loss:
    def __init__(self, calls):
        self.calls = calls

    def backward(self):
        self.calls.append("backward")


def _step_on(rec, buckets, after=True):
    def forward_loss(x, lab):
        rec.calls.append(("forward", x, lab))
        return _Loss(rec.calls), "aux"
    return tl.optim_step(forward_loss, types.SimpleNamespace(zero_grad=rec.zero_grad, step=rec.step), buckets,
                         after=(lambda: rec.calls.append("after")) if after else None)


def test_optim_step_call_order_with_buckets():
    rec = _Recorder()
    buckets = types.SimpleNamespace(zero=rec.zero, finish=rec.finish)
    loss, aux = _step_on(rec, lambda: buckets)("x", "lab")
    assert isinstance(loss, _Loss) and aux == "aux"
    assert rec.calls == ["zero", ("forward", "x", "lab"), "backward", "finish", "step", "after"]


def test_optim_step_without_buckets_drops_the_gradients():
    for buckets in (None, lambda: None):
        rec = _Recorder()
        _step_on(rec, buckets, after=False)("x", "lab")
        assert rec.calls == [("zero_grad", {"set_to_none": True}), ("forward", "x", "lab"), "backward", "step"]


def test_optim_step_uses_buckets_assigned_after_it_was_built():
    rec = _Recorder()
    owner = types.SimpleNamespace(buckets=None)
    step = _step_on(rec, lambda: owner.buckets)
    owner.buckets = types.SimpleNamespace(zero=rec.zero, finish=rec.finish)
    step("x", "lab")
    assert rec.calls == ["zero", ("forward", "x", "lab"), "backward", "finish", "step", "after"]
