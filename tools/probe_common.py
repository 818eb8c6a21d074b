"""What the device probes share (``tools/*_probe.py``): timing between device events, host wall time, the summary of a
series, and a HIP graph of back-to-back calls.  Imported by the probes as scripts; the package and the tests do not use it."""
import statistics
import time

import torch


def timed(fn):
    """Milliseconds between two device events around ``fn()``, the device idle before and after."""
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def wall(fn):
    """Milliseconds of host wall time of ``fn()`` up to the end of its device work."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs)}


def graph_of(call, calls):
    """``calls`` back-to-back ``call()`` captured into a HIP graph (the host's enqueue cost is not part of a replay),
    replayed once."""
    call()                                   # warm-up: code object, workspace
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            call()
    g.replay()
    return g
