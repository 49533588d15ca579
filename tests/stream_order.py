"""Stream-contract checks for the kernel tests (tests/test_stream_*.py; DESIGN.md "Stream contract").

include/kemr.h: "all launches are asynchronous on the hipStream_t passed".  The numerics and the memory-contract tests call on the
default stream and synchronise the device before they compare, so a launch on another stream, a hipMemsetAsync given 0, a copy that
blocks the host or a hidden device synchronisation passes all of them.  Here a call is described once, in tests/footprint.py's
In / IntIn / Out / Work / SizeOf form, and made twice:

  plain call   default stream, tight tensors, roomy zeroed workspace, full synchronisation: the reference bits (and the host time);
  late call    on a side stream, ENQUEUED WHILE ITS INPUTS DO NOT EXIST YET.  Float inputs start as 0xff bytes (NaN in every format),
               the workspace (exactly the stated size) as 0xff, outputs as 0xa5, index inputs as a different VALID instance of the
               same shape (`stale`; default: the items in reverse order).  Then, all on the side stream: a device-side delay, copies of
               the real inputs into the argument buffers, 0xa5 over every output (without initial content) and 0xff over the
               workspace ONCE MORE, the call, a copy of every output, the same poison over every input again, an event.

  S1  right after the call returns, the delay's end event is still pending: everything was enqueued while no input existed and the
      host was not blocked (not asserted for HOST_SYNC_CALLS, whose contract needs a host value);
  S2  after side.synchronize() every output -- as a copy queued on the side stream right behind the call holds it -- has the plain
      call's bits.  A kernel, memset or copy on any stream but the side stream runs before the inputs arrive, after they are poisoned
      again or behind that copy, and fails this.  That holds for a write that depends on no input as well -- a memset of pad rows
      or of a counter given stream 0: issued while the delay runs, it is overwritten by the second fill of the outputs and the
      workspace before the call's own work starts, so the rows keep 0xa5 where the plain call left zeros, and the kernels find 0xff in the counter;
  S3  an event recorded on the default stream before the late call is complete, and the default stream is idle, when the call returns.

A failed case raises StreamOrderError naming the call and EVERY assertion that failed (`.failed`), so tests/
test_stream_order_selftest_gpu.py can tell which one caught a planted defect.

Not covered (the stale content equals the real one, because validity is tied to sizes passed by value): the CSR row offsets of a
bonus list (tied to the length of the column array), and the host arrays of the batch transforms and of kemr_panel_build (read on
the host during the call).  `row_start` and `lens` ARE covered where a case passes the same lengths in another order (the same
`rows` in all); a case that cannot must pass the real tensor as `stale` and say so.

Side streams: one pool of three per process (`streams`), shared by every test of the stream contract -- with the default stream the
four hardware queues a process gets by default -- instead of a fresh stream per call.

Delay: torch.cuda._sleep, calibrated once per process with events (`calibration`); a chain of matmuls if _sleep does not scale with
its argument.  Length per case: max(20 ms, 10 x the plain call's host time); a case that would need more than 250 ms is too big.
"""
import time

import torch

import footprint as F
from footprint import In, IntIn, Out, SizeOf, Work

MIN_DELAY_MS = 20.0
MAX_DELAY_MS = 250.0

# Calls whose contract needs a host value: exempt from S1 only.  The same list: include/kemr.h "Stream contract".
HOST_SYNC_CALLS = (
    "ClipEngine.encode_text(device ids, no lens)",     # one device-to-host copy of B lengths sizes the packed launches (engine.py)
    "kemr_profile_end",                                # returns the measured times
    "kemr_model_finalize",                             # uploads the packed weights: a device synchronisation and a blocking copy
    "kemr_model_destroy",                              # frees the weights: hipFree waits for the device (found by reading, csrc/model.hip)
    "kemr_debug_sim_lists",                            # returns the list counters of a finished kemr_sim_topk
    "kemr_debug_gemm_stamps",                          # returns the cycle stamps of finished GEMMs (include/kemr_debug.h)
)


class StreamOrderError(AssertionError):
    def __init__(self, what, failures):
        self.what, self.failures = what, dict(failures)
        self.failed = set(self.failures)
        super().__init__(f"{what}: " + "; ".join(f"{k}: {v}" for k, v in sorted(self.failures.items())))


# ------------------------------------------------------------------------------------------------ streams and the delay
_STREAMS = {}
_CAL = {}


def streams(device):
    """The process's three side streams on `device`, each after one launch of its own: a stream's first launch sets up its queue,
    which costs the host milliseconds that are not the call's (they would count against a gate that the first enqueue sits behind)."""
    key = torch.device(device)
    if key not in _STREAMS:
        made = tuple(torch.cuda.Stream(key) for _ in range(3))
        for s in made:
            with torch.cuda.stream(s):
                torch.zeros(16, device=key).add_(1)
            s.synchronize()
        _STREAMS[key] = made
    return _STREAMS[key]


def _timed(device, queue):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    a.record()
    queue()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calibration(device):
    """{"kind": "sleep", "per_ms": cycles per millisecond} or {"kind": "matmul", "per_ms": matmuls per millisecond, "x": operand}."""
    key = torch.device(device)
    if key in _CAL:
        return _CAL[key]
    with torch.cuda.device(key):
        cal = None
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)
            t1 = _timed(key, lambda: torch.cuda._sleep(2_000_000))
            t4 = _timed(key, lambda: torch.cuda._sleep(8_000_000))
            if t1 > 0.05 and 3.0 <= t4 / t1 <= 5.0:          # scales with its argument
                cal = {"kind": "sleep", "per_ms": 8_000_000 / t4}
        if cal is None:
            x = torch.randn(1024, 1024, device=key)
            torch.mm(x, x)
            reps = 64
            ms = _timed(key, lambda: [torch.mm(x, x) for _ in range(reps)])
            cal = {"kind": "matmul", "per_ms": reps / ms, "x": x}
    _CAL[key] = cal
    print(f"stream_order delay calibration: {cal['kind']} {cal['per_ms']:.1f} per ms")
    return cal


def queue_delay(device, ms):
    """`ms` milliseconds of device-side delay on the current stream."""
    cal = calibration(device)
    n = max(1, int(cal["per_ms"] * ms))
    if cal["kind"] == "sleep":
        torch.cuda._sleep(n)
    else:
        for _ in range(n):
            torch.mm(cal["x"], cal["x"])


def delay_for(host_ms, what=""):
    ms = max(MIN_DELAY_MS, 10.0 * host_ms)
    assert ms <= MAX_DELAY_MS, f"{what}: a plain call of {host_ms:.2f} ms on the host needs a delay of {ms:.0f} ms: the case is too big"
    return ms


# ------------------------------------------------------------------------------------------------ the late-input call
def _fill(t, byte):
    t.view(torch.uint8).fill_(byte)


def _stale_of(spec, given):
    """The valid other instance an index argument holds while the real one does not exist."""
    if given is not None:
        s = given.to(torch.int32)
        assert tuple(s.shape) == tuple(spec.t.shape), (tuple(s.shape), tuple(spec.t.shape))
        return s
    return spec.t.flip(0) if spec.t.dim() else spec.t.clone()


class Late:
    """What run_late measured and holds: .plain / .late (tensors per argument, None for scalars), .host_ms (plain call), .late_host_ms,
    .delay_ms, .pending (S1's observation)."""


def run_late(fn, specs, device, as_arg=None, what="", name=None, stale=None):
    """fn(*args) launches on torch.cuda.current_stream(device); tensor arguments are converted by as_arg (default: ctypes void
    pointers).  name: the call's name when it is one of HOST_SYNC_CALLS (S1 is then not asserted).  stale: {argument index: tensor}
    for IntIn arguments whose reverse is not a valid instance.  Raises StreamOrderError; returns a Late."""
    if as_arg is None:
        import ctypes
        as_arg = lambda t: ctypes.c_void_p(t.data_ptr())         # noqa: E731
    device = torch.device(device)
    specs, stale = list(specs), dict(stale or {})
    assert name is None or name in HOST_SYNC_CALLS, name
    side = streams(device)[0]
    default = torch.cuda.default_stream(device)

    def plain_buffers():
        out = []
        for s in specs:
            if isinstance(s, In):
                out.append(s.t.contiguous().to(device).clone())
            elif isinstance(s, Out):
                p = torch.empty(s.shape, dtype=s.dtype, device=device)
                _fill(p, F.GUARD)
                if s.init is not None:
                    p.copy_(s.init.to(device))
                out.append(p)
            elif isinstance(s, Work):
                out.append(torch.zeros(max(s.nbytes, s.plain_bytes, 256), dtype=torch.uint8, device=device))
            else:
                out.append(None)
        return out

    def arguments(bufs):
        return [bufs[s.index].numel() if isinstance(s, SizeOf) else (s if b is None else as_arg(b)) for s, b in zip(specs, bufs)]

    res = Late()
    with torch.cuda.device(device):
        # ---- plain call (twice: the first pays for whatever a first launch loads; the second is timed)
        for _ in range(2):
            plain = plain_buffers()
            args = arguments(plain)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            fn(*args)
            res.host_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize(device)
        res.plain = plain
        res.delay_ms = delay_for(res.host_ms, what)

        # ---- late call: buffers and the staged real inputs, made on the default stream
        late, real, poison, refill = [], [], [], []
        for i, s in enumerate(specs):
            if isinstance(s, In):
                src = s.t.contiguous().to(device).clone()
                buf = torch.empty_like(src)
                if isinstance(s, IntIn):
                    old = _stale_of(s, stale.get(i)).contiguous().to(device)
                    poison.append((buf, old))
                else:
                    poison.append((buf, F.POISON))
                real.append((buf, src))
                late.append(buf)
            elif isinstance(s, Out):
                buf = torch.empty(s.shape, dtype=s.dtype, device=device)
                _fill(buf, F.GUARD)
                if s.init is not None:
                    real.append((buf, s.init.to(device).to(s.dtype).clone()))
                else:
                    refill.append((buf, F.GUARD))
                late.append(buf)
            elif isinstance(s, Work):
                buf = torch.empty(max(s.nbytes, 1), dtype=torch.uint8, device=device)
                _fill(buf, F.POISON)
                refill.append((buf, F.POISON))
                late.append(buf)
            else:
                late.append(None)
        res.late = late

        def spoil():
            for buf, with_what in poison:
                buf.copy_(with_what) if torch.is_tensor(with_what) else _fill(buf, with_what)

        spoil()
        args = arguments(late)
        before = torch.cuda.Event()
        before.record(default)
        torch.cuda.synchronize(device)
        delay_end, done = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(side):
            queue_delay(device, res.delay_ms)
            delay_end.record(side)
            for buf, src in real:
                buf.copy_(src, non_blocking=True)
            for buf, byte in refill:                                  # whatever reached an output or the workspace while the delay ran is gone
                _fill(buf, byte)
            t0 = time.perf_counter()
            fn(*args)
            res.late_host_ms = (time.perf_counter() - t0) * 1e3
            res.pending = not delay_end.query()                       # S1
            default_idle = before.query() and default.query()         # S3
            snaps = [b.clone() if isinstance(s, Out) else None for s, b in zip(specs, late)]      # the outputs at the call's place in the stream
            spoil()
            done.record(side)
        side.synchronize()
        torch.cuda.synchronize(device)

    print(f"stream_order {what}: host {res.host_ms:.3f} ms plain, {res.late_host_ms:.3f} ms late, delay {res.delay_ms:.0f} ms")
    failures = {}
    if not res.pending and name is None:
        failures["S1"] = (f"the delay of {res.delay_ms:.0f} ms had ended when the call returned after {res.late_host_ms:.2f} ms on the "
                          f"host (plain call: {res.host_ms:.2f} ms): the call waited for the device")
    if not default_idle:
        failures["S3"] = "the default stream was not idle when the call returned"
    for i, (s, p, w) in enumerate(zip(specs, plain, snaps)):
        if not isinstance(s, Out):
            continue
        try:
            if s.init is None:
                assert any(bool((F.bits(a) != F.GUARD).any()) for a in F._parts(s.written, p)), "the plain call wrote nothing"
            for a, b in zip(F._parts(s.written, w), F._parts(s.written, p)):
                F.same_bits(a, b)
        except AssertionError as e:
            failures["S2"] = f"argument {i}: late call != plain call: {e}"
            break
    if failures:
        raise StreamOrderError(what, failures)
    return res
