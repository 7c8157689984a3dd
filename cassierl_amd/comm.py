"""The collectives of the data-parallel learning loop and their timer.  One process per GPU, each with its own shard of environments; every
gradient, Fisher-vector product, normal equation and statistic is averaged or summed with all_reduce (RCCL on MI355X, gloo in the CPU tests), so
all ranks take the identical step."""
import torch
import torch.distributed as dist


def _world():
    return dist.get_world_size() if dist.is_initialized() else 1


class CommTimer:
    """Per-collective timing of the data-parallel loop without host synchronisation: a pair of HIP events on the current stream
    around every collective (the RCCL kernel runs on the communicator's stream, which the current stream waits for), read once by
    `summary()`.  bench.py sets `trpo.COMM = CommTimer()` for configs[3]'s line; None (default) costs nothing."""

    def __init__(self):
        self.spans = {}

    def run(self, name, fn, t):
        if not t.is_cuda:
            import time
            t0 = time.perf_counter()
            fn()
            self.spans.setdefault(name, []).append(time.perf_counter() - t0)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self.spans.setdefault(name, []).append((e0, e1))

    def summary(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        out = {}
        for name, sp in self.spans.items():
            ms = [x * 1e3 if isinstance(x, float) else x[0].elapsed_time(x[1]) for x in sp]
            out[name] = dict(calls=len(ms), total_ms=float(sum(ms)), mean_ms=float(sum(ms) / max(1, len(ms))), max_ms=float(max(ms)))
        return out


def _all_reduce_sum(t, name):
    # The timer's slot is the global COMM of trpo.py, where bench.py installs it by assignment (`trpo.COMM = CommTimer()`): an assignment rebinds
    # that module's name only, so the slot is read there, at call time (trpo.py imports this module, hence not at the top of this file).
    from . import trpo
    if trpo.COMM is None:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    else:
        trpo.COMM.run(name, lambda: dist.all_reduce(t, op=dist.ReduceOp.SUM), t)


def all_mean_(t, name="all_reduce"):
    """In-place mean over ranks (no-op single process)."""
    if _world() > 1:
        _all_reduce_sum(t, name)
        t /= _world()
    return t


def all_sum_(t, name="all_reduce"):
    if _world() > 1:
        _all_reduce_sum(t, name)
    return t
