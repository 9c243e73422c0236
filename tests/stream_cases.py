"""What tests/test_gpu_streams.py needs to tell a call's stream from the null
stream: a delay that can be queued on a torch stream, a side stream that is
shown to run while the null stream is held, the held null stream itself, and
inputs that arrive on a stream after a delay.  Test infrastructure only; torch
is imported on first use, so the restated size classes import without it.

Why a held null stream tells: torch's side streams are non-blocking, so work
that the library queues on the null stream by mistake -- a kernel, a memset, a
copy given 0 instead of the call's stream -- neither waits for the side
stream's work nor is waited for by it.  With the null stream held such work
has not run when the call returns, and its output is what the warm-up on the
*decoy* left there: a wrong table.  A blocking ``hipMemcpy``, or anything that
waits for the device, returns only once the hold is over, which
``NullBusy.still_pending()`` shows right after.

The hold is no tolerance on any result: it only has to outlast the call
(HOLD_FACTOR times the call's own time on the idle device, between HOLD_MIN_MS
and HOLD_MAX_MS), and every test asserts that it did."""
import contextlib
import time

HOLD_FACTOR = 20
HOLD_MIN_MS = 100.0
HOLD_MAX_MS = 1000.0
STAGE_MS = 5.0            # the delay in front of staged()'s copies
PROBE_MS = 50.0           # the hold of the side-stream probe
MAX_SIDE_STREAMS = 4      # GPU_MAX_HW_QUEUES=4 may fold two streams onto one hardware queue

_state = {'cycles_per_ms': None, 'side': None, 'side_log': []}


def _torch():
    import torch
    return torch


def pool_round_up(b):
    """csrc/ctg_pool.h: pool_round_up -- the size class of a request of b bytes
    (tests/test_pool.py pins this restatement against tools/pool_check.cpp)."""
    r = 256
    while r < b:
        r = r * 2 if r < (1 << 20) else r + (r >> 2)
    return r


def same_block_class(a, b):
    """A cached block freed by a request of ``a`` bytes serves one of ``b``
    bytes (csrc/ctg_pool.h: DevicePool::alloc -- the smallest cached block of
    at least b's class and at most twice it)."""
    ca, cb = pool_round_up(a), pool_round_up(b)
    return cb <= ca <= 2 * cb


def hold_ms_for(call_seconds):
    """The hold of a test whose call took ``call_seconds`` on the idle device."""
    return min(max(HOLD_FACTOR * call_seconds * 1e3, HOLD_MIN_MS), HOLD_MAX_MS)


def _cycles_per_ms():
    """torch.cuda._sleep counts device clock ticks: one timed call, with
    events, on first use."""
    if _state['cycles_per_ms'] is None:
        torch = _torch()
        s = torch.cuda.current_stream()
        torch.cuda._sleep(100000)                      # (loads the kernel)
        s.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20000000
        a.record(s)
        torch.cuda._sleep(n)
        b.record(s)
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.5, 'torch.cuda._sleep(%d) took %.3f ms: cannot calibrate the hold' % (n, ms)
        _state['cycles_per_ms'] = n / ms
    return _state['cycles_per_ms']


def hold(stream, ms):
    """Queue a delay of ``ms`` milliseconds on the torch stream ``stream``."""
    torch = _torch()
    cycles = int(_cycles_per_ms() * ms)
    with torch.cuda.stream(stream):
        while cycles > 0:                              # (_sleep takes a 32-bit count on some builds)
            step = min(cycles, 1 << 30)
            torch.cuda._sleep(step)
            cycles -= step


class NullBusy:
    def __init__(self, ms):
        self.ms = ms

    def still_pending(self):
        return not _torch().cuda.default_stream().query()


@contextlib.contextmanager
def null_busy(ms):
    """Hold the null stream for ``ms`` milliseconds from here on; the block runs
    meanwhile.  On the way out the device is idle again (nothing that was
    queued on the null stream by mistake outlives the test)."""
    torch = _torch()
    torch.cuda.synchronize()
    nb = NullBusy(ms)
    hold(torch.cuda.default_stream(), ms)
    try:
        yield nb
    finally:
        torch.cuda.synchronize()


def side_stream():
    """A torch side stream that provably runs while the null stream is held:
    a trivial kernel on it finishes while a hold on the null stream is pending.
    At most MAX_SIDE_STREAMS are tried; the first that passes serves the whole
    session.  None passing is an error that names the premise -- no test may
    pass without it."""
    if _state['side'] is not None:
        return _state['side']
    torch = _torch()
    for k in range(MAX_SIDE_STREAMS):
        s = torch.cuda.Stream()
        x = torch.zeros(64, device='cuda')
        with torch.cuda.stream(s):
            x.add_(1)                                  # (the kernel loaded, the stream's queue made)
        torch.cuda.synchronize()
        with null_busy(PROBE_MS) as nb:
            with torch.cuda.stream(s):
                x.add_(1)
            s.synchronize()
            overlapped = nb.still_pending()
        _state['side_log'].append((k, overlapped))
        if overlapped:
            assert float(x[0].item()) == 2.0
            print('stream_cases: side stream %d of %d overlaps the null stream' % (k + 1, MAX_SIDE_STREAMS))
            _state['side'] = s
            return s
    raise AssertionError('premise of the stream tests not met: none of %d torch side streams ran while the null '
                         'stream was held (%r)' % (MAX_SIDE_STREAMS, _state['side_log']))


def second_stream(first):
    """Another side stream than ``first`` (Protocol B needs two; they need not
    overlap each other, only not be the null stream)."""
    torch = _torch()
    for _ in range(MAX_SIDE_STREAMS):
        s = torch.cuda.Stream()
        if s.cuda_stream != first.cuda_stream and s.cuda_stream != 0:
            return s
    raise AssertionError('no second side stream')


def to_device(arrays, stream):
    """numpy arrays -> CUDA tensors, copied on ``stream`` (uint64 / uint32 as
    the signed views the wrappers take)."""
    import numpy as np
    torch = _torch()
    out = []
    with torch.cuda.stream(stream):
        for a in arrays:
            if a is None:
                out.append(None)
                continue
            a = np.ascontiguousarray(a)
            if a.dtype == np.uint64:
                a = a.view(np.int64)
            elif a.dtype == np.uint32:
                a = a.view(np.int32)
            out.append(torch.from_numpy(a.copy()).cuda())
    return out


def staged(decoy, true, stream, ms=STAGE_MS):
    """Device tensors that hold the arrays of ``decoy`` now, and the arrays of
    ``true`` once what is queued on ``stream`` here has run: a short hold, then
    device-to-device copies.  A read that does not wait for the stream sees the
    decoy -- well-formed data of the same shape and dtype with another answer."""
    torch = _torch()
    assert len(decoy) == len(true)
    for d, t in zip(decoy, true):
        assert (d is None) == (t is None) and (d is None or (d.shape == t.shape and d.dtype == t.dtype))
    dev = to_device(decoy, stream)
    src = to_device(true, stream)
    stream.synchronize()
    hold(stream, ms)
    with torch.cuda.stream(stream):
        for d, t in zip(dev, src):
            if d is not None:
                d.copy_(t)
    return dev


def timed(fn):
    """(fn(), seconds) on the device as it is -- call it on the idle device."""
    torch = _torch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0
