"""GPU: the stream-contract helper (tests/stream_order.py) binds.  Torch stand-ins for a kernel call, no library code: the correct
stand-in -- two ops on the current stream -- passes, and every planted defect is caught by the assertion that is there for it."""
import pytest
import torch

import stream_order as SO
from footprint import In, IntIn, Out

pytestmark = pytest.mark.gpu

N = 4096


def _specs():
    g = torch.Generator().manual_seed(0)
    return [In(torch.randn(N, generator=g)), In(torch.randn(N, generator=g)), IntIn(torch.randperm(N, generator=g)), Out((N,), torch.float32)]


def _run(device, fn, what):
    return SO.run_late(fn, _specs(), device, as_arg=lambda t: t, what=what)


def _caught(device, fn, what):
    with pytest.raises(SO.StreamOrderError) as e:
        _run(device, fn, what)
    print(e.value)
    return e.value.failed


def correct(x, y, idx, out):
    tmp = x * 2
    torch.add(tmp[idx.long()], y, out=out)


def test_the_correct_stand_in_passes(device):
    res = _run(device, correct, "correct stand-in")
    assert res.pending and res.delay_ms >= SO.MIN_DELAY_MS
    want = torch.randn(N, generator=torch.Generator().manual_seed(0))           # x: the first draw of _specs
    assert torch.equal(res.plain[3].cpu(), (want * 2)[_specs()[2].t.long()] + _specs()[1].t)


def test_an_op_on_the_default_stream_fails_s2(device):
    def fn(x, y, idx, out):
        with torch.cuda.stream(torch.cuda.default_stream(device)):
            tmp = x * 2                                                         # reads x before it exists
        torch.add(tmp[idx.long()], y, out=out)
    failed = _caught(device, fn, "default-stream op")
    assert "S2" in failed and "S1" not in failed


def test_an_input_read_on_another_stream_fails_s2(device):
    def fn(x, y, idx, out):
        with torch.cuda.stream(SO.streams(device)[1]):
            tmp = x.clone()
        torch.add((tmp * 2)[idx.long()], y, out=out)
    failed = _caught(device, fn, "input read on another stream")
    assert "S2" in failed and "S1" not in failed


def test_a_stale_index_read_fails_s2(device):
    """The index argument read early holds the reversed permutation: a wrong answer, no out-of-range index."""
    def fn(x, y, idx, out):
        with torch.cuda.stream(SO.streams(device)[1]):
            early = idx.long()
        torch.add((x * 2)[early], y, out=out)
    failed = _caught(device, fn, "index read on another stream")
    assert "S2" in failed and "S1" not in failed


PAD = 256


def padded(x, y, idx, out, fill_stream=None):
    """A stand-in whose second op depends on no input: the last PAD elements of out are zero-filled (as the pad rows of kemr_op_layernorm_x3)."""
    torch.add((x * 2)[idx.long()][:N - PAD], y[:N - PAD], out=out[:N - PAD])
    with torch.cuda.stream(fill_stream or torch.cuda.current_stream()):
        out[N - PAD:].zero_()


def test_a_constant_fill_on_the_call_s_stream_passes(device):
    res = _run(device, padded, "stand-in with a constant fill")
    assert res.pending and not bool(res.plain[3][N - PAD:].any())


def test_a_constant_fill_on_the_default_stream_fails_s2(device):
    """The fill reads no input, so it writes the same zeros whenever it runs: only the second fill of the outputs, queued behind the
    delay, shows that it ran before its turn."""
    def fn(x, y, idx, out):
        padded(x, y, idx, out, fill_stream=torch.cuda.default_stream(device))
    failed = _caught(device, fn, "constant fill on the default stream")
    assert "S2" in failed and "S1" not in failed


def test_a_device_synchronisation_fails_s1(device):
    def fn(x, y, idx, out):
        torch.cuda.synchronize(device)
        correct(x, y, idx, out)
    assert _caught(device, fn, "torch.cuda.synchronize") == {"S1"}


def test_a_host_round_trip_fails_s1(device):
    def fn(x, y, idx, out):
        correct(x.cpu().to(device), y, idx, out)
    assert _caught(device, fn, ".cpu() round trip") == {"S1"}


def test_a_result_written_from_a_second_stream_fails_s2(device):
    """The result leaves from a second stream that waits for the first and is never waited for (here behind 5 ms of its own work, as
    behind a busy queue): the caller's stream does not know of it."""
    def fn(x, y, idx, out):
        tmp = (x * 2)[idx.long()] + y
        ready = torch.cuda.Event()
        ready.record()
        other = SO.streams(device)[2]
        with torch.cuda.stream(other):
            other.wait_event(ready)
            SO.queue_delay(device, 5.0)
            out.copy_(tmp)
        tmp.record_stream(other)
    failed = _caught(device, fn, "result from a second stream")
    assert "S2" in failed and "S1" not in failed
