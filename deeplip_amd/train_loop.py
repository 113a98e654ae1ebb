"""The step loop train_video.py, train_audio.py and train_fusion.py share: step body, recorded steps, ring of cached host batches,
prefetch behind the running step, the epoch's metrics on the device.  Host-only at import (no GPU, no library)."""
import os

import torch


def optim_step(forward_loss, optim, buckets=None, after=None):
    """``(*inputs) -> (loss, aux)``: one optimisation step, launches only (what a recorded step replays).  ``buckets``: a callable that
    returns the trainer's GradBuckets or None, asked on every step (the trainers build their buckets with the first epoch)."""
    def step(*inputs):
        b = buckets() if buckets is not None else None
        if b is None:
            optim.zero_grad(set_to_none=True)
        else:
            b.zero()                    # the gradients are views into the buckets: cleared in place
        loss, aux = forward_loss(*inputs)
        loss.backward()                 # bucket all-reduces start from the hooks as the gradients land
        if b is not None:
            b.finish()                  # wait for them, average
        optim.step()
        if after is not None:
            after()
        return loss, aux
    return step


def records_with(buckets):
    """Whether steps are recorded with these gradient buckets: the graph then captures their RCCL all-reduces (tests/test_rccl_gpu.py);
    DLIP_GRAPH_WITH_BUCKETS=0 keeps such runs eager.  Such a step keeps its branches on one stream (``branch_streams=buckets is None``): a
    bucket's all-reduce is enqueued behind the CURRENT stream of the hook that completes it, not behind another branch stream's writes."""
    return buckets is None or os.environ.get("DLIP_GRAPH_WITH_BUCKETS", "1") != "0"


def recorded_steps(fn, modules, optimizers, buckets, device, branch_streams):
    """``fn`` as one recorded step per batch shape (and key): a shape's first step runs eagerly, its second records (train_plan.py)."""
    from .train_plan import ShapeKeyedSteps, grad_witness, step_state
    return ShapeKeyedSteps(fn, eager_steps=1, device=device, branch_streams=branch_streams,
                           state=step_state(modules, optimizers, buckets), witness=grad_witness(modules, buckets))


class BatchRing:
    """``get(i, *args)`` -> ``make(i, *args)``; with ``n_cache`` > 0 (``data_cache``) the first n_cache batches are made once (``make``
    pins them) and walked cyclically: a run that measures the trainer, not the source."""

    def __init__(self, make, n_cache):
        self.make, self.n, self.cache = make, int(n_cache or 0), {}

    def get(self, i, *args):
        if self.n <= 0:
            return self.make(i, *args)
        k = i % self.n
        if k not in self.cache:
            self.cache[k] = self.make(k, *args)
        return self.cache[k]


class Prefetch:
    """Host batches (name-keyed dicts) to the device on ONE copy stream for the owner's lifetime: torch's caching allocator keeps a pool
    per stream, so a stream per epoch left every epoch's batch buffers reserved (tools/probes/leak_check_eager.py).  cpu: a pass-through."""

    def __init__(self, device):
        self.device = device
        self.stream = torch.cuda.Stream(device=device) if device.type != "cpu" else None

    def stage(self, host):
        """Start the copies of every tensor of ``host`` (other values pass through) behind the running step -> what ``take`` wants."""
        if self.stream is None:
            return host, None
        with torch.cuda.stream(self.stream):
            dev = {k: v.to(self.device, non_blocking=True) if isinstance(v, torch.Tensor) else v for k, v in host.items()}
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return dev, ev

    def take(self, staged):
        """The staged batch by name, its tensors ordered into (and kept alive for) the current stream."""
        dev, ev = staged
        if ev is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            for v in dev.values():
                if isinstance(v, torch.Tensor):
                    v.record_stream(cur)
        return dev


class EpochMeter:
    """sum loss * n, sum hits, sum n in float64 on the device; ``add`` right behind a step (the next replay rewrites its outputs)."""

    def __init__(self, device):
        self.acc = torch.zeros(3, dtype=torch.float64, device=device)

    def add(self, loss, hits, n):
        self.acc[0] += loss.detach().double() * n
        self.acc[1] += hits
        self.acc[2] += n

    def read(self):
        return self.acc.tolist()
