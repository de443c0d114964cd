"""Tools of tests/test_gpu_streams.py: a stream held back by queued work that ends by itself, the precondition that it still was held
when the competing work went in, and allocations that turn a block handed out too early into NaNs.

A cross-stream handoff (an event wait, a `wait_stream`, a `record_stream`) only matters while the producing or reading stream is
behind; at test shapes it never is -- it has drained before the other stream's first kernel starts.  `hold` puts it behind on purpose."""
import time

import torch

_CAL = {}                  # device index -> (kind, units per second)
_HOLDS = {}                # id(event) -> [start event, end event, host time of the enqueue, asked seconds, host ms until the check]
_MM_N = 2048


def _calibrate(device):
    """(kind, units of work per second of stream time), measured once per device against the clock with two events: `sleep` --
    torch.cuda._sleep cycles; `mm` -- products of two [2048, 2048] matrices, where _sleep is missing or does not spin"""
    key = torch.device(device).index or 0
    if key in _CAL:
        return _CAL[key]
    with torch.cuda.device(device):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kind, rate = "mm", None
        if hasattr(torch.cuda, "_sleep"):
            try:
                torch.cuda._sleep(1_000_000)                              # (first launch: code object load, not timed)
                torch.cuda.synchronize()
                cycles = 20_000_000
                t0.record()
                torch.cuda._sleep(cycles)
                t1.record()
                torch.cuda.synchronize()
                ms = t0.elapsed_time(t1)
                if ms > 0.5:                                              # a counter of any plausible rate spins for milliseconds here
                    kind, rate = "sleep", cycles / (ms * 1e-3)
            except (RuntimeError, AttributeError):
                pass
        if rate is None:
            a = torch.ones(_MM_N, _MM_N, device=device)
            torch.mm(a, a)
            torch.cuda.synchronize()
            reps = 50
            t0.record()
            for _ in range(reps):
                torch.mm(a, a)
            t1.record()
            torch.cuda.synchronize()
            rate = reps / (t0.elapsed_time(t1) * 1e-3)
    _CAL[key] = (kind, rate)
    print(f"[streams] hold calibrated on the clock: {kind}, {rate:.4g} units per second")
    return _CAL[key]


def hold(stream, seconds=0.25):
    """enqueue work on `stream` that keeps it busy for about `seconds`; returns an event recorded behind that work"""
    kind, rate = _calibrate(stream.device)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record(stream)
        if kind == "sleep":
            left = int(seconds * rate)
            while left > 0:                                               # (pieces of at most 2^30 cycles: the argument's range is not ours)
                piece = min(left, 1 << 30)
                torch.cuda._sleep(piece)
                left -= piece
        else:
            a = torch.ones(_MM_N, _MM_N, device=stream.device)
            for _ in range(max(1, int(seconds * rate))):
                torch.mm(a, a)
        end.record(stream)
    _HOLDS[id(end)] = [start, end, time.perf_counter(), float(seconds), None]
    return end


def assert_still_held(event, what):
    """the precondition of a held-stream test, checked on the host directly after the competing work was enqueued: the held stream had
    not reached what was queued behind the hold.  A condition, not a measurement: a failure says the hold was too short."""
    rec = _HOLDS.get(id(event))
    if rec is not None:
        rec[4] = (time.perf_counter() - rec[2]) * 1e3
    took = "" if rec is None else f" (the enqueue took {rec[4]:.1f} ms of host time, the hold was asked to last {rec[3] * 1e3:.0f} ms)"
    assert not event.query(), f"{what}: the hold was too short -- the held stream had drained before the competing work was in{took}"


def report(event, what):
    """after a synchronisation: print the hold's measured length against the host time of the enqueue it had to outlast"""
    start, end, _, asked, host_ms = _HOLDS.pop(id(event))
    held_ms = start.elapsed_time(end)
    line = f"[streams] {what}: hold {held_ms:.0f} ms (asked {asked * 1e3:.0f})"
    if host_ms is not None:
        line += f", competing work enqueued within {host_ms:.1f} ms of host time: margin x{held_ms / max(host_ms, 1e-3):.0f}"
    print(line)
    return held_ms, host_ms


def poison(stream, nbytes_list):
    """under `stream`: uint8 tensors of the given sizes filled with 0xFF -- every float32 in them is a NaN.  Returned so that the caller
    keeps them alive: a block the caching allocator hands out while another stream still reads it shows up in that stream's output."""
    out = []
    with torch.cuda.stream(stream):
        for n in nbytes_list:
            out.append(torch.full((int(n),), 0xFF, dtype=torch.uint8, device=stream.device))
    return out


def landed_on(poisoned, addresses):
    """how many of `addresses` (old data_ptr values) lie inside one of the poisoned tensors"""
    spans = [(t.data_ptr(), t.data_ptr() + t.numel()) for t in poisoned]
    return sum(any(lo <= a < hi for lo, hi in spans) for a in addresses)
