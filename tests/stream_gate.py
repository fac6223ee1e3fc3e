"""The stream contract of the C ABI, made testable (tests/test_gpu_stream_order.py, tests/test_gpu_graph_capture.py; the logic
is checked on CPU tensors in tests/test_stream_contract_cpu.py).

include/nsr.h: "`stream` is a hipStream_t passed as void*; work is only ENQUEUED on it, the library never synchronises the device
or the host", with the exceptions the headers name.  Two things follow for every entry point that takes a stream:

  order      everything the call does to device memory happens ON that stream, behind what the caller enqueued before it;
  no wait    an enqueue-only call returns without waiting for the stream.

``TABLE`` has one row per entry point whose prototype in include/*.h has a ``void* stream`` parameter: ``ENQUEUE_ONLY``, or
``WAITS`` with the header and the sentence that documents the wait.  tests/test_stream_contract_cpu.py parses the headers and
asserts that the rows are exactly those prototypes.

The protocol (``run_ordered``) makes a launch that left the stream, or a hidden wait, show deterministically:

  1. a case has two fully valid input sets A and B of the same shapes (indices in range, weights in the packed ranges: a stray
     early read gives a wrong result, never an out-of-range access);
  2. serially: run A, keep the bits of every output, of the state updated in place and the status words; run B in the same
     buffers; the two must differ (else the case shows nothing).  Every buffer now holds what B left: the stale state;
  3. the run of B once more on the side stream, ungated (``warm_up``: torch's allocator then serves the wrapper's own
     allocations from that stream's pool); then on the side stream, behind a GATE (a kernel that spins for a calibrated time): copy A's inputs and the pristine in-place
     state into the buffers, put the stale bytes back into the outputs and -- moved on by some words -- into the scratch (so
     that a memset that ran early is overwritten again), make the call, timing it on the host, and ask whether the stream is still busy;
  4. enqueue-only: the stream must still be busy (the gate is closed: the call did not wait) and the call must have taken
     less than half the gate on the host;
  5. after a synchronize: every output and in-place buffer has A's bits, and the status words are the serial ones.

Anything that ran before the gate opened read B, or was overwritten by the stale bytes: the result carries B's bits or a mixture.

The streams are behind a small interface (``TorchStreams`` here; a deferred queue on CPU tensors in the CPU test), so the
bookkeeping -- A / B staleness, the non-degeneracy assertion, the verdicts -- is tested without a GPU."""
import json
import os
import time
from collections import OrderedDict
from typing import Callable, Dict, List, NamedTuple, Optional

import torch

from tests import scratch_state as ss

ENQUEUE_ONLY, WAITS = "ENQUEUE_ONLY", "WAITS"
GATE_FLOOR_MS = 100.0       # ordinary host jitter is a few milliseconds: far from half of this
GATE_FACTOR = 20.0          # a call that ran unordered cannot finish after the gate by accident


class Row(NamedTuple):
    kind: str
    header: Optional[str] = None      # WAITS: the header that documents the wait ...
    sentence: Optional[str] = None    # ... and words of the sentence, as they stand in it (whitespace aside)
    capture: bool = False             # an ENQUEUE_ONLY row a caller would capture into a graph (tests/test_gpu_graph_capture.py)


def _e(capture: bool = False) -> Row:
    return Row(ENQUEUE_ONLY, capture=capture)


_SAVED_TRAIN = "the call waits for the stream to read the header"
_SAVED_REFINE = "The backward reads the header back (it waits for the stream)"

TABLE: "OrderedDict[str, Row]" = OrderedDict([
    # ---- include/nsr.h
    ("nsr_pack_weights", Row(WAITS, "nsr.h", "the call WAITS for `stream`")),
    ("nsr_pack_weights_async", _e()),
    ("nsr_weights_status", Row(WAITS, "nsr.h", "and WAITS for `stream`")),
    ("nsr_weights_set_options", _e()),
    ("nsr_weights_set_gamma", _e()),
    ("nsr_gen_rays", _e()),
    ("nsr_gen_rays_range", _e()),
    ("nsr_posenc", _e()),
    ("nsr_posenc_e", _e()),
    ("nsr_sample_along_rays", _e()),
    ("nsr_mlp_forward", _e()),
    ("nsr_render_rays", _e()),
    ("nsr_render_rays_composited", _e()),
    ("nsr_render_rays_density", _e()),
    ("nsr_forward_rays_density_coarse", _e(True)),
    ("nsr_render_rays_composited_ert", _e()),
    ("nsr_forward_rays_ert", _e(True)),
    ("nsr_composite", _e()),
    ("nsr_resample_along_rays", _e()),
    ("nsr_forward_rays", _e(True)),
    ("nsr_forward_rays_profiled", _e(True)),
    ("nsr_sr_mean", _e()),
    ("nsr_unflatten", _e()),
    # ---- include/nsr_data.h
    ("nsr_rayset_batch", _e()),
    ("nsr_gen_rays_opt", _e()),
    # ---- include/nsr_image.h
    ("nsr_resample_pass_u8", _e()),
    ("nsr_image_to_targets", _e()),
    ("nsr_rgba_premultiply_u8", _e()),
    ("nsr_image_to_targets_rgba", _e()),
    # ---- include/nsr_losses.h
    ("nsr_tv_loss", _e(True)),
    ("nsr_tv_loss_backward", _e(True)),
    ("nsr_gradient_loss", _e(True)),
    ("nsr_gradient_loss_backward", _e(True)),
    ("nsr_laplacian_loss", _e(True)),
    ("nsr_laplacian_loss_backward", _e(True)),
    # ---- include/nsr_metrics.h
    ("nsr_ssim", _e(True)),
    ("nsr_ssim_backward", _e(True)),
    ("nsr_psnr", _e(True)),
    # ---- include/nsr_refine.h
    ("nsr_refine_pack_weights", _e()),
    ("nsr_refine_forward", _e(True)),
    ("nsr_refine_pack_weights_noref", _e()),
    ("nsr_refine_forward_noref", _e(True)),
    ("nsr_refine_train_forward", _e()),
    ("nsr_refine_train_backward", Row(WAITS, "nsr_refine.h", _SAVED_REFINE)),
    ("nsr_refine_train_forward_p", _e()),
    ("nsr_refine_train_backward_p", Row(WAITS, "nsr_refine.h", _SAVED_REFINE)),
    ("nsr_refine_train_backward_w", Row(WAITS, "nsr_refine.h", _SAVED_REFINE)),
    ("nsr_refine_tile", _e()),
    ("nsr_refine_gather", _e()),
    ("nsr_refine_stitch", _e()),
    # ---- include/nsr_refine_data.h
    ("nsr_refine_patch_batch", _e()),
    ("nsr_refine_aug_bbox", _e()),
    ("nsr_refine_warp_image", _e()),
    # ---- include/nsr_train.h
    ("nsr_train_loss_and_grads", _e()),
    ("nsr_train_loss_and_grads_var", _e()),
    ("nsr_train_forward", _e(True)),
    ("nsr_train_backward", Row(WAITS, "nsr_train.h", _SAVED_TRAIN)),
    ("nsr_train_status_reset", _e()),
    ("nsr_train_status", Row(WAITS, "nsr_train.h", "nsr_train_status copies the word to the host (waits for the stream)")),
    ("nsr_adam_step", _e()),
    ("nsr_train_arch_forward", _e()),
    ("nsr_train_arch_backward", Row(WAITS, "nsr_train.h", _SAVED_TRAIN)),
    ("nsr_adam_step_n", _e(True)),
    ("nsr_arch_fused_pack", _e()),
    ("nsr_arch_fused_forward", _e()),
    ("nsr_arch_fused_render_rays", _e()),
    ("nsr_train_arch_forward_e", _e(True)),
    ("nsr_train_arch_backward_e", Row(WAITS, "nsr_train.h", _SAVED_TRAIN)),
    ("nsr_arch_fused_pack_e", _e()),
    ("nsr_arch_fused_forward_e", _e()),
    ("nsr_arch_fused_render_rays_e", _e(True)),
    ("nsr_train_arch_backward_r", Row(WAITS, "nsr_train.h", _SAVED_TRAIN)),
    ("nsr_train_backward_r", Row(WAITS, "nsr_train.h", _SAVED_TRAIN)),
    ("nsr_linear", _e()),
    ("nsr_split_weights", _e()),
    ("nsr_linear_f16x3", _e()),
    # ---- include/nsr_warp.h
    ("nsr_depth_warp", _e()),
])


# ------------------------------------------------------------------------------------------------------------------ a case
class Case:
    """One call and every device buffer it touches.

    ``call(host)``      makes the call on torch's CURRENT stream; ``host`` is ``host_A`` or ``host_B`` (arguments that live on
                        the host: poses, option words).  It may return a dict of further output tensors (a Python wrapper's own
                        allocations); those are compared like ``outs``.
    ``bufs``            name -> device buffer the call READS; ``A`` / ``B``: name -> the two contents (same shape and dtype).
    ``state``           name -> device buffer the call UPDATES IN PLACE (Adam moments, running statistics, a status block);
                        its content at construction is the pristine state both runs start from.
    ``outs``            name -> device buffer the call WRITES.
    ``scratch``         name -> workspace and the like: contents unspecified, re-dirtied behind the gate, never compared.
    ``status(host)``    after a synchronize: the status words as a tuple of ints (may clear them), or None.
    ``waits``           the row is WAITS, or the Python wrapper in front of it waits and says so (``documented``): step 4 is skipped."""

    def __init__(self, name: str, entry: str, call: Callable, bufs=None, A=None, B=None, state=None, outs=None, scratch=None,
                 host_A=None, host_B=None, status: Optional[Callable] = None, waits: bool = False):
        self.name, self.entry, self.call = name, entry, call
        self.bufs, self.A, self.B = dict(bufs or {}), dict(A or {}), dict(B or {})
        self.state, self.outs, self.scratch = dict(state or {}), dict(outs or {}), dict(scratch or {})
        self.host_A, self.host_B = host_A, host_B
        self.status, self.waits = status, bool(waits)
        self.documented: Optional[str] = None     # a wrapper's own wait: the key of stream_cases.WRAPPER_WAITS that documents it
        if set(self.bufs) != set(self.A) or set(self.bufs) != set(self.B):
            raise ValueError(f"{name}: bufs, A and B must have the same keys")
        for k, b in self.bufs.items():
            for which, src in (("A", self.A[k]), ("B", self.B[k])):
                if src.shape != b.shape or src.dtype != b.dtype:
                    raise ValueError(f"{name}: {which}[{k!r}] is {tuple(src.shape)} {src.dtype}, the buffer {tuple(b.shape)} {b.dtype}")
        self.pristine = {k: v.clone() for k, v in self.state.items()}


class Want(NamedTuple):
    bits: "OrderedDict[str, torch.Tensor]"      # outputs and in-place state after the run
    status: Optional[tuple]
    gpu_ms: float


class Serial(NamedTuple):
    want_A: Want
    want_B: Want
    stale: Dict[str, torch.Tensor]              # what B left in outs, and in scratch (displaced, see ``displaced``)


class SerialStreams:
    """Everything at once on the current stream / on CPU tensors: step 2."""

    def copy(self, dst, src):
        dst.copy_(src)

    def synchronize(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def timed(self, fn):
        """(result, GPU milliseconds) of fn()."""
        if not torch.cuda.is_available():
            t0 = time.perf_counter()
            return fn(), (time.perf_counter() - t0) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        return res, float(e0.elapsed_time(e1))


def _load(case: Case, streams, which: str):
    src = case.A if which == "A" else case.B
    for k, b in case.bufs.items():
        streams.copy(b, src[k])
    for k, b in case.state.items():
        streams.copy(b, case.pristine[k])


def _collect(case: Case, returned) -> "OrderedDict[str, torch.Tensor]":
    bits = OrderedDict()
    for k, v in case.outs.items():
        bits[f"out {k}"] = v.detach().clone()
    for k, v in case.state.items():
        bits[f"state {k}"] = v.detach().clone()
    for k, v in (returned or {}).items():
        if v is not None:
            bits[f"ret {k}"] = v.detach().clone()
    if not bits:
        raise ValueError(f"{case.name}: the case compares nothing")
    return bits


def differing(a: "OrderedDict[str, torch.Tensor]", b: "OrderedDict[str, torch.Tensor]") -> List[str]:
    """The names whose bits differ between two collections of the same case."""
    return [k for k in a if k not in b or not ss.same_bits(a[k], b[k])]


def run_serial(case: Case, streams=None) -> Serial:
    """Step 2.  Raises AssertionError when A and B give the same bits (the case would show nothing)."""
    streams = streams or SerialStreams()
    wants = []
    for which, host in (("A", case.host_A), ("B", case.host_B)):
        _load(case, streams, which)
        streams.synchronize()
        returned, ms = streams.timed(lambda: case.call(host))
        streams.synchronize()
        bits = _collect(case, returned)
        wants.append(Want(bits, case.status(host) if case.status else None, ms))
    want_A, want_B = wants
    assert differing(want_A.bits, want_B.bits), \
        f"{case.name}: degenerate case: input sets A and B give the same bits in {list(want_A.bits)}"
    stale = {f"out {k}": v.detach().clone() for k, v in case.outs.items()}
    stale.update({f"scratch {k}": displaced(v) for k, v in case.scratch.items()})
    return Serial(want_A, want_B, stale)


def displaced(t: torch.Tensor, words: int = 257) -> torch.Tensor:
    """What a call left in a scratch buffer, moved on by ``words`` 4-byte words (cyclically): the same finite values at other
    places, as a call of another shape leaves them.  The bytes a call left itself are zero exactly where its own memsets cleared
    them -- padding rows and columns that nothing writes afterwards -- so putting THOSE back would hide a memset that ran early.
    A workspace may hold anything on entry (tests/test_gpu_scratch_state.py)."""
    flat = t.detach().contiguous().reshape(-1)
    b = flat.view(torch.uint8)
    if b.numel() == 0:
        return flat.clone().view(t.shape)
    return torch.roll(b, 4 * words).view(flat.dtype).view(t.shape)


class Gated(NamedTuple):
    bits: "OrderedDict[str, torch.Tensor]"
    status: Optional[tuple]
    busy_after_call: bool       # the side stream had not finished when the call returned (the gate was still closed)
    host_ms: float


def run_gated(case: Case, serial: Serial, streams) -> Gated:
    """Step 3 on ``streams`` (``TorchStreams`` or the CPU test's queue): everything of input set A is queued BEHIND the gate."""
    with streams.side():
        streams.gate()
        _load(case, streams, "A")
        for k, v in case.outs.items():
            streams.copy(v, serial.stale[f"out {k}"])
        for k, v in case.scratch.items():
            streams.copy(v, serial.stale[f"scratch {k}"])
        t0 = time.perf_counter()
        returned = case.call(case.host_A)
        host_ms = (time.perf_counter() - t0) * 1e3
        busy = not streams.query()
    streams.synchronize()
    bits = _collect(case, returned)
    return Gated(bits, case.status(case.host_A) if case.status else None, busy, host_ms)


def warm_up(case: Case, streams) -> None:
    """The run of B once more, on the side stream with no gate: whatever a wrapper allocates (outputs, temporaries) then comes
    from that stream's pool of cached blocks during the gated call, so its host time is the wrapper's, not a device allocation's.
    The buffers are left as the serial run of B left them; the status words the run raised are cleared."""
    with streams.side():
        _load(case, streams, "B")
        case.call(case.host_B)
    streams.synchronize()
    if case.status:
        case.status(case.host_B)


def verdict(case: Case, serial: Serial, got: Gated, gate_ms: float) -> List[str]:
    """Steps 4 and 5: the lines that say what is wrong (an empty list: the call kept the contract)."""
    bad = []
    if not case.waits:
        if not got.busy_after_call:
            bad.append(f"{case.name}: the stream was idle when the call returned: the call waited for its stream (or the gate "
                       f"of {gate_ms:.0f} ms ran out during a call of {got.host_ms:.1f} ms)")
        if got.host_ms >= 0.5 * gate_ms:
            bad.append(f"{case.name}: the call took {got.host_ms:.1f} ms on the host, not less than half the gate ({gate_ms:.0f} ms): "
                       "it blocks")
    for k, want in serial.want_A.bits.items():
        if k not in got.bits:
            bad.append(f"{case.name}: {k} missing from the gated run")
            continue
        line = ss.diff(k, got.bits[k], want)
        if line:
            stale = k in serial.want_B.bits and ss.same_bits(got.bits[k], serial.want_B.bits[k])
            bad.append(f"{case.name}: {line}" + (" -- these are input set B's bits: the work ran before the gate opened"
                                                 if stale else " -- neither A's nor B's bits: part of the work left the stream"))
    if got.status != serial.want_A.status:
        bad.append(f"{case.name}: status words {got.status} behind the gate, {serial.want_A.status} serially")
    return bad


def run_ordered(case: Case, streams, gate_for: Callable[[float], float], record: Optional[dict] = None) -> List[str]:
    """The whole protocol for one case; ``gate_for(serial GPU ms) -> gate ms`` arms ``streams`` (``Calibration.arm``)."""
    serial = run_serial(case)
    # the run of B: the first run (A) carries what happens once per process (code objects loaded, autograd's thread started)
    gate_ms = gate_for(serial.want_B.gpu_ms)
    warm_up(case, streams)
    got = run_gated(case, serial, streams)
    if record is not None:
        record[case.name] = {"entry": case.entry, "serial_gpu_ms": round(serial.want_B.gpu_ms, 4), "first_run_gpu_ms": round(serial.want_A.gpu_ms, 4),
                             "host_call_ms": round(got.host_ms, 4), "gate_ms": round(gate_ms, 1)}
    return verdict(case, serial, got, gate_ms)


# -------------------------------------------------------------------------------------------------- the gate, on the device
class TorchStreams:
    """One side stream, ordered behind torch's current stream at every ``side()``; the gate is ``torch.cuda._sleep``."""

    def __init__(self):
        self.cycles = 0
        self._side = None
        self._ctx = None

    def side(self):
        if self._side is None:           # one side stream for the session: torch's allocator keeps a pool of blocks per stream,
            self._side = torch.cuda.Stream()     # and ``warm_up`` fills this one's before a call is timed behind the gate
        self._side.wait_stream(torch.cuda.current_stream())
        self._ctx = torch.cuda.stream(self._side)
        return self._ctx

    def gate(self):
        torch.cuda._sleep(int(self.cycles))

    def copy(self, dst, src):
        dst.copy_(src, non_blocking=True)

    def query(self) -> bool:
        return self._side.query()

    def synchronize(self):
        self._side.synchronize()
        torch.cuda.current_stream().synchronize()


class Calibration:
    """``torch.cuda._sleep`` counts device clock ticks: time a fixed count with events once, scale from that."""
    PROBE_CYCLES = 20_000_000

    def __init__(self):
        torch.cuda._sleep(1000)                      # load the kernel
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(self.PROBE_CYCLES)
        e1.record()
        e1.synchronize()
        ms = float(e0.elapsed_time(e1))
        assert ms > 0.0, "torch.cuda._sleep took no time: the gate cannot be calibrated"
        self.cycles_per_ms = self.PROBE_CYCLES / ms
        self.slowest_ms = 0.0
        self.cases: Dict[str, dict] = {}

    def gate_ms(self, serial_gpu_ms: float) -> float:
        """The larger of the floor and GATE_FACTOR times the slowest serial GPU time seen SO FAR in this session (a case's own time
        included): the cases run in one pass, each right after its serial runs."""
        self.slowest_ms = max(self.slowest_ms, float(serial_gpu_ms))
        return max(GATE_FLOOR_MS, GATE_FACTOR * self.slowest_ms)

    def arm(self, streams: TorchStreams) -> Callable[[float], float]:
        def gate_for(serial_gpu_ms: float) -> float:
            ms = self.gate_ms(serial_gpu_ms)
            streams.cycles = int(ms * self.cycles_per_ms)
            return ms
        return gate_for

    def write_profile(self, repo_root: str) -> Optional[str]:
        """profiles/stream_contract.json, when NSR_RECORD_PROFILES is set (the project's convention)."""
        if not os.environ.get("NSR_RECORD_PROFILES"):
            return None
        path = os.path.join(repo_root, "profiles", "stream_contract.json")
        doc = {"what": "tests/test_gpu_stream_order.py: calibration of the torch.cuda._sleep gate, and per case the serial GPU time "
                       "(events; the run of input set B, the second in the process), the host time of the gated call and the gate it ran behind",
               "device": torch.cuda.get_device_name(0), "sleep_cycles_per_ms": round(self.cycles_per_ms, 1),
               "gate_floor_ms": GATE_FLOOR_MS, "gate_factor": GATE_FACTOR, "slowest_serial_gpu_ms": round(self.slowest_ms, 4),
               "cases": self.cases}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        return path


class Control(NamedTuple):
    ok: bool
    message: str


def positive_control(streams: TorchStreams, gate_ms: float = GATE_FLOOR_MS, n: int = 1 << 16) -> Control:
    """Work on the null stream really overtakes the gated side stream on this machine: with the gate closed and the late copy
    of A queued behind it, a copy enqueued on the DEFAULT stream reads B, and the side stream is still busy afterwards.  Were
    the two streams serialised (one hardware queue), every ordering test would pass vacuously."""
    buf = torch.full((n,), 2.0, device="cuda")        # B
    a = torch.full((n,), 1.0, device="cuda")          # A
    probe = torch.zeros(n, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with streams.side():
        streams.gate()
        streams.copy(buf, a)
    probe.copy_(buf)                                   # default stream: not ordered behind the side stream
    torch.cuda.current_stream().synchronize()          # the default stream only
    host_ms = (time.perf_counter() - t0) * 1e3
    busy = not streams.query()
    early = bool((probe == 2.0).all().item())
    streams.synchronize()
    late = bool((buf == 1.0).all().item())
    if not early:
        return Control(False, f"positive control: a copy on the default stream did not overtake the gated side stream (it read A "
                              f"after {host_ms:.1f} ms, gate {gate_ms:.0f} ms): the two streams are serialised on this machine and "
                              "no ordering test can show anything")
    if not busy:
        return Control(False, f"positive control: the side stream was idle {host_ms:.1f} ms after a gate of {gate_ms:.0f} ms was "
                              "enqueued: the gate does not hold")
    if not late:
        return Control(False, "positive control: the copy queued behind the gate did not land")
    return Control(True, f"positive control: default-stream copy read B after {host_ms:.1f} ms, side stream still gated")
