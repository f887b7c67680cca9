"""A producer that really is late, for the tests of the stream-ordering contract of the device-pointer calls (include/mi355_msm.h):
every such call either enqueues its work on the hipStream_t on which its input becomes ready, or (the context's codec, check and
set_bases calls) synchronises the device first.  A test of that promise is worth something only while the input is NOT yet there when
the call is made, so the helpers here put tens of milliseconds of device work in front of the bytes and let the test prove on the host
that the window was open: a launch on any other stream reads poison.

Nothing here needs a GPU to import; torch is handed in by the caller."""
import math

POISON = 0x5A          # what the memory of a late input holds until its producer has run
OUT_POISON = 0x33      # what the producer of a late output writes over it
# The delay the calibration aims at.  It has to dwarf a launch latency, and it has to outlast what the host does between enqueuing it and
# making the call under test (a second upload, a few hundred launches), also on a busy host that is descheduled for some milliseconds:
# 20 ms, cut to about 15 by the time the enqueuing itself took, was seen to run out there; 40 ms behind a pass that costs the device
# some twenty times what it costs the host to enqueue leaves nearly all of the 40.
TARGET_MS = 40.0
MIN_MS = 10.0          # what every test asserts between `started` and `produced`
SCRATCH_BYTES = 64 << 20


class Delay:
    """`count` element-wise passes into a scratch tensor of 64 MiB, calibrated once on `stream`: a pass is timed between two events (as
    the mean of PROBE passes: one pass alone drowns in what the events themselves cost), `count` is what reaches 1.25 x TARGET_MS, and
    the whole chain is timed again; if that falls short of TARGET_MS the count is doubled, once.  Beyond that nothing is retried: a
    test whose window was not open fails.  The pass is digamma of a constant vector written into the scratch tensor: bound by
    arithmetic, not by memory, so it keeps the device busy for many times what its launch costs the host (a plain add over 64 MiB takes
    the device 20 us and the host 4), and its time does not depend on what earlier passes left behind."""

    PROBE = 32

    def __init__(self, torch, stream):
        self.torch = torch
        self.source = torch.full((SCRATCH_BYTES // 4,), 2.5, dtype=torch.float32, device="cuda")
        self.scratch = torch.empty_like(self.source)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            self._op()                                   # (the first launch loads the kernel)
            self.per_op_ms = max(self._timed(stream, self.PROBE) / self.PROBE, 1e-3)
            self.count = int(math.ceil(1.25 * TARGET_MS / self.per_op_ms))
            self.measured_ms = self._timed(stream, self.count)
            if self.measured_ms < TARGET_MS:
                self.count *= 2
                self.measured_ms = self._timed(stream, self.count)
        print("stream_cases.Delay: %.1f us a pass, %d passes, %.1f ms enqueued" % (1e3 * self.per_op_ms, self.count, self.measured_ms))

    def _op(self):
        self.torch.digamma(self.source, out=self.scratch)

    def _timed(self, stream, count):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(count):
            self._op()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    def enqueue(self):
        """the delay, on the current stream"""
        for _ in range(self.count):
            self._op()


def _events(torch):
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def poisoned(torch, shape):
    """a uint8 GPU tensor full of POISON, written and synchronised on the default stream (whatever stream the caller has made current)"""
    default = torch.cuda.default_stream()
    with torch.cuda.stream(default):
        t = torch.full(tuple(shape), POISON, dtype=torch.uint8, device="cuda")
    default.synchronize()
    return t


def late(torch, raw, stream, delay, shape=None, fill=()):
    """`raw` (bytes or a NumPy uint8 array) as a GPU tensor that is not there yet: its memory holds POISON, written and synchronised on
    the default stream, and `stream` has enqueued the event `started`, the delay, a device-to-device copy of the true bytes from a
    staging tensor uploaded beforehand, and the event `produced`.  The two events are attributes of the tensor.  `fill`: tensors of
    poisoned() that the same producer fills with OUT_POISON after the delay, as late_out does behind a delay of its own; they get the
    same two events."""
    if isinstance(raw, (bytes, bytearray)):
        host = torch.frombuffer(bytearray(raw) if len(raw) else bytearray(1), dtype=torch.uint8)[:len(raw)]
    else:
        host = torch.from_numpy(raw.reshape(-1).copy())
    default = torch.cuda.default_stream()
    with torch.cuda.stream(default):                     # (whatever stream the caller has made current)
        staging = host.cuda()
        t = torch.full_like(staging, POISON)
    default.synchronize()
    started, produced = _events(torch)
    with torch.cuda.stream(stream):
        started.record(stream)
        delay.enqueue()
        for o in fill:
            o.fill_(OUT_POISON)
        t.copy_(staging)
        produced.record(stream)
    staging.record_stream(stream)
    for o in fill:
        o.started, o.produced = started, produced
    if shape is not None:
        t = t.reshape(shape)
    t.started, t.produced = started, produced
    return t


def late_many(torch, raws, stream, delay, fill=()):
    """several byte strings behind ONE producer: 1-D views of one late tensor, each carrying its events.  Inputs of one call are made
    this way, so that none of them is produced while the next is still being uploaded."""
    whole = late(torch, b"".join(bytes(r) for r in raws), stream, delay, fill=fill)
    views, at = [], 0
    for r in raws:
        v = whole[at:at + len(r)]
        v.started, v.produced = whole.started, whole.produced
        views.append(v)
        at += len(r)
    return views


def late_out(torch, shape, stream, delay):
    """an `out=` tensor whose producer is late: POISON now, and after the delay on `stream` a fill with OUT_POISON -- a result written
    on any other stream is overwritten afterwards (write after write)"""
    t = poisoned(torch, shape)
    started, produced = _events(torch)
    with torch.cuda.stream(stream):
        started.record(stream)
        delay.enqueue()
        t.fill_(OUT_POISON)
        produced.record(stream)
    t.started, t.produced = started, produced
    return t


def window_open(produced):
    """asserted on the host immediately before the library call: the producer has not finished, so the call cannot have found its
    input by luck"""
    return not produced.query()


def delay_ms(t):
    """milliseconds between `started` and `produced` of a late tensor, once both have happened; every test asserts >= MIN_MS"""
    return t.started.elapsed_time(t.produced)


def closed(*tensors):
    """after the call and a synchronisation: every producer took at least MIN_MS (else the test proved nothing and must fail)"""
    return all(delay_ms(t) >= MIN_MS for t in tensors)


# Every device-pointer entry point of include/mi355_msm.h and the test that pins its ordering (tests/test_stream_coverage.py keeps this
# table equal to the header): "module::test".
_ORDER = "test_gpu_stream_order"
COVERED = {
    "mi355_msm_set_bases_device": _ORDER + "::test_set_bases_after_a_late_producer_on_any_stream",
    "mi355_msm_check_bases_device": _ORDER + "::test_check_bases_after_a_late_producer_on_any_stream",
    "mi355_msm_decompress_points_device": _ORDER + "::test_codec_after_a_late_producer_on_any_stream",
    "mi355_msm_compress_points_device": _ORDER + "::test_codec_after_a_late_producer_on_any_stream",
    "mi355_msm_run_device": _ORDER + "::test_run_with_late_scalars",
    "mi355_msm_run_async": "test_gpu_async::test_async_call_returns_at_once_and_other_streams_overlap",
    "mi355_msm_fixed_mul_device": _ORDER + "::test_mul_points_and_window_table_with_late_inputs",
    "mi355_msm_mul_points_device": _ORDER + "::test_mul_points_and_window_table_with_late_inputs",
    "mi355_msm_domain_transform_device": _ORDER + "::test_transforms",
    "mi355_msm_domain_mul_device": _ORDER + "::test_mul_and_vec_ops",
    "mi355_msm_domain_batch_inverse_device": _ORDER + "::test_batch_inversion",
    "mi355_msm_domain_vec_op_device": _ORDER + "::test_mul_and_vec_ops",
    "mi355_msm_domain_evaluate_device": _ORDER + "::test_evaluate_and_divide_by_linear",
    "mi355_msm_domain_divide_by_linear_device": _ORDER + "::test_evaluate_and_divide_by_linear",
    "mi355_msm_domain_lagrange_device": _ORDER + "::test_lagrange_and_vanishing",
    "mi355_msm_domain_divide_by_vanishing_on_coset_device": _ORDER + "::test_lagrange_and_vanishing",
    "mi355_msm_domain_scan_device": _ORDER + "::test_scans",
    "mi355_msm_domain_permutation_product_device": _ORDER + "::test_permutation_product",
    "mi355_msm_domain_plonk_quotient_device": _ORDER + "::test_plonk_quotient",
    "mi355_msm_domain_linear_combination_device": _ORDER + "::test_linear_combination",
    "mi355_msm_fft_points_device": _ORDER + "::test_fft_points",
}
