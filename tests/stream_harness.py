"""A harness that turns a launch on the wrong stream into a wrong answer (tests/test_stream_contract_gpu.py).

The contract (include/gomoku_hip.h, Conventions): an entry that takes a `stream` does all of its device work on that stream and, if it returns
host values, waits for that stream first; an entry without a `stream` that touches a handle is ordered after everything already enqueued for
that handle, on any stream, and has finished when it returns.

A scenario is a list of calls over one handle, built by a factory so that it can be built twice from identical initial state.  It runs twice:

  eager    every call on the current stream, torch.cuda.synchronize() after each.  The reference: nothing here that the rest of the suite does
           not already hold to the oracle.  The host time of every call is measured.
  delayed  the calls are cut into segments, a segment ending at each call the header documents as waiting for its stream.  Each segment is
           enqueued on a non-blocking side stream S behind a fresh delay (torch.cuda._sleep), and nothing else synchronises.  A launch that
           leaves S runs during the delay, against the state of the last host wait: a valid state, so nothing faults, but the wrong one.

Every output of the two runs is then compared bit for bit.  The delay is 10 x the eager enqueue time of the segment's asynchronous calls, at
least 5 ms and at most 250 ms; what guards it is an event recorded right behind the delay, which must not have completed when the segment's
last asynchronous call has returned to the host.  If it has, the segment proved nothing: that is a failure.

At most three streams (S, T for the sensitivity check, and the NULL stream), no threads, nothing is retried."""
import json
import os
import time

import numpy as np

MIN_MS, MAX_MS, FACTOR = 5.0, 250.0, 10.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.environ.get("GMK_STREAM_CONTRACT_JSON") or os.path.join(ROOT, "profiles", "stream_contract.json")


class Call:
    """fn(stream) with stream a hipStream_t as an int; torch's current stream is that stream while fn runs.  waits: the header says the entry
    waits for its stream (or it has no stream argument and returns host values), so a segment of the delayed run ends behind it."""
    __slots__ = ("fn", "waits")

    def __init__(self, fn, waits=False):
        self.fn, self.waits = fn, waits


class Scenario:
    """calls: [Call]; outputs() -> {name: tensor / array / number}, asked for once everything is drained; close() frees the handles."""

    def __init__(self, calls, outputs, close=None):
        self.calls, self.outputs, self.close = list(calls), outputs, close or (lambda: None)

    def segments(self):
        out, cur = [], []
        for c in self.calls:
            cur.append(c)
            if c.waits:
                out.append(cur)
                cur = []
        if cur:
            out.append(cur)
        return out


def bits(value):
    """An output as bytes: what is compared is the bit pattern, so NaNs and signed zeros count"""
    import torch
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(np.asarray(value))
    return a.reshape(-1).view(np.uint8)


def differing(a, b):
    """the names of a's outputs whose bits differ from b's"""
    assert sorted(a) == sorted(b), "the two runs report different outputs: %s / %s" % (sorted(a), sorted(b))
    return [k for k in sorted(a) if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]


def snapshot(outputs):
    return {k: bits(v).copy() for k, v in outputs.items()}


class Harness:
    def __init__(self):
        import torch
        self.torch = torch
        self.S = torch.cuda.Stream()                              # (torch's streams do not synchronise with the NULL stream)
        self.T = torch.cuda.Stream()
        for stream in (self.S, self.T):                           # (a stream's first launch sets up its queue, which takes longer than a short delay)
            with torch.cuda.stream(stream):
                torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
        self.cycles_per_ms, self.calibration = self._calibrate()
        self.report = {"cycles_per_ms": self.cycles_per_ms, "calibration": self.calibration, "min_ms": MIN_MS, "max_ms": MAX_MS, "factor": FACTOR,
                       "scenarios": {}, "sensitivity": {}}

    # ---- the delay ----
    def _sleep_ms(self, cycles):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(int(cycles))
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def _calibrate(self):
        """cycles of torch.cuda._sleep per millisecond, from two lengths (the slope: the launch's own cost drops out), and a 5 ms delay measured"""
        self._sleep_ms(1000000)                                   # the kernel is loaded
        c1, c2 = 2000000, 22000000
        t1, t2 = self._sleep_ms(c1), self._sleep_ms(c2)
        assert t2 > t1 > 0.0, "torch.cuda._sleep does not scale with its argument: %r ms, %r ms" % (t1, t2)
        per_ms = (c2 - c1) / (t2 - t1)
        check = self._sleep_ms(MIN_MS * per_ms)
        assert check >= 0.8 * MIN_MS, "a calibrated %g ms delay took %g ms" % (MIN_MS, check)
        return per_ms, {"cycles": [c1, c2], "ms": [t1, t2], "delay_5ms_measured_ms": check}

    def delay_ms(self, enqueue_seconds):
        return min(max(FACTOR * enqueue_seconds * 1e3, MIN_MS), MAX_MS)

    def delay(self, ms):
        """A delay of `ms` on the current stream, and the event right behind it"""
        torch = self.torch
        torch.cuda._sleep(int(ms * self.cycles_per_ms))
        ev = torch.cuda.Event()
        ev.record()
        return ev

    # ---- the two runs ----
    def _eager(self, make):
        torch = self.torch
        torch.cuda.synchronize()
        sc = make()
        torch.cuda.synchronize()
        times = []
        try:
            for seg in sc.segments():
                t = 0.0
                for c in seg:
                    stream = torch.cuda.current_stream().cuda_stream
                    t0 = time.perf_counter()
                    c.fn(stream)
                    if not c.waits:
                        t += time.perf_counter() - t0
                    torch.cuda.synchronize()
                times.append(t)
            return snapshot(sc.outputs()), times
        finally:
            torch.cuda.synchronize()
            sc.close()

    def _delayed(self, make, times):
        torch = self.torch
        torch.cuda.synchronize()
        sc = make()
        torch.cuda.synchronize()
        delays, held = [], []
        try:
            segs = sc.segments()
            assert len(segs) == len(times)
            with torch.cuda.stream(self.S):
                for seg, t in zip(segs, times):
                    ms = self.delay_ms(t)
                    ev = self.delay(ms)
                    for c in seg:
                        if c.waits:
                            held.append(not ev.query())           # the last asynchronous call of the segment has returned
                        c.fn(self.S.cuda_stream)
                    if not seg[-1].waits:
                        held.append(not ev.query())
                    delays.append(ms)
            torch.cuda.synchronize()
            return snapshot(sc.outputs()), delays, held
        finally:
            torch.cuda.synchronize()
            sc.close()

    def check(self, name, make):
        """Runs the scenario eagerly and delayed and holds the second to the first, bit for bit."""
        eager, times = self._eager(make)
        delayed, delays, held = self._delayed(make, times)
        self.report["scenarios"][name] = {"segments": len(times), "eager_enqueue_ms": [t * 1e3 for t in times], "delay_ms": delays, "delay_outlasted_enqueue": held}
        assert all(held), "%s: the delay of segment(s) %s had ended before the segment was enqueued (%s ms for %s ms of calls): the run proved nothing" % (
            name, [i for i, h in enumerate(held) if not h], delays, [t * 1e3 for t in times])
        bad = differing(eager, delayed)
        assert not bad, "%s: behind a delayed producer these outputs differ from the eager run's: %s" % (name, bad)
        return eager

    def sensitivity(self, name, buf, decoy, real, entry, outputs):
        """The harness sees a misplaced call: buf holds the valid decoy, a delayed copy on S overwrites it with the real input, and entry is called
        on T on purpose.  Its result must be f(decoy), not f(real), both known from eager runs.  (Stateless entries only.)"""
        torch = self.torch

        def eager(src):
            buf.copy_(src)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            entry(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return snapshot(outputs()), time.perf_counter() - t0
        eager(decoy)                                              # (the first call of a shape may allocate, and wait)
        f_decoy, t = eager(decoy)
        f_real, _ = eager(real)
        assert differing(f_decoy, f_real), "%s: the decoy and the real input give the same outputs" % name
        buf.copy_(decoy)
        torch.cuda.synchronize()
        ms = self.delay_ms(t)
        with torch.cuda.stream(self.S):
            ev = self.delay(ms)
            buf.copy_(real, non_blocking=True)
        with torch.cuda.stream(self.T):
            entry(self.T.cuda_stream)
        self.T.synchronize()
        held = not ev.query()
        torch.cuda.synchronize()
        got = snapshot(outputs())
        saw = "decoy" if not differing(got, f_decoy) else "real" if not differing(got, f_real) else "neither"
        self.report["sensitivity"][name] = {"eager_ms": t * 1e3, "delay_ms": ms, "delay_outlasted_call": held, "result": "f(%s)" % saw}
        assert held, "%s: the %g ms delay had ended before the misplaced call finished" % (name, ms)
        assert saw == "decoy", "%s: a call on another stream than its producer's gave f(%s), not f(decoy)" % (name, saw)
        assert torch.equal(buf, real)

    def write(self):
        try:
            os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
            with open(PROFILE, "w") as f:
                json.dump(self.report, f, indent=1, sort_keys=True)
                f.write("\n")
        except OSError:
            pass                                                  # (a read-only checkout: the assertions have been made all the same)
