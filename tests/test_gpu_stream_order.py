"""Every entry point that takes a stream keeps the stream contract of include/nsr.h: its work is ordered on that stream and, unless
the headers say that it waits, it returns without waiting for it.

The protocol, the gate and the table of entry points are tests/stream_gate.py; the cases -- buffers, the two input sets, the
call -- tests/stream_cases.py.  The positive control runs first: it shows that work on the default stream really overtakes a
gated side stream on this machine.  Should it fail, every ordering test fails with its message (none skips): they could only
pass vacuously.

NSR_RECORD_PROFILES=1 writes the calibration and the per-case times to profiles/stream_contract.json."""
import os
import time

import pytest
import torch

from tests import stream_cases, stream_gate as sg

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = stream_cases.all_cases()


@pytest.fixture(scope="module")
def gate():
    """The calibration (once per module), the streams, and the shared inputs of the cases."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import _lib
    _lib.load()
    t0 = time.time()
    cal, streams = sg.Calibration(), sg.TorchStreams()
    yield cal, streams
    path = cal.write_profile(REPO)
    print(f"\ntests/test_gpu_stream_order.py: {time.time() - t0:.1f} s wall, {cal.cycles_per_ms:.0f} sleep cycles per ms, slowest case "
          f"{cal.slowest_ms:.2f} ms" + (f"; wrote {path}" if path else ""))


@pytest.fixture(scope="module")
def ctx():
    return stream_cases.Ctx()


@pytest.fixture(scope="module")
def control(gate):
    cal, streams = gate
    ms = cal.arm(streams)(0.0)
    return sg.positive_control(streams, ms)


def test_default_stream_overtakes_the_gated_stream(control):
    """With the gate closed on the side stream and the copy of A queued behind it, a copy on the default stream reads B, and the
    side stream is still busy once the default stream has drained."""
    assert control.ok, control.message


@pytest.mark.parametrize("name,entry,build", ALL, ids=[c[0] for c in ALL])
def test_ordered_on_its_stream(gate, ctx, control, name, entry, build):
    """Steps 1-5 of tests/stream_gate.py for one case.  ENQUEUE_ONLY rows must leave the gate closed and return in less than half
    the gate; WAITS rows (the wait is documented in the header the table names) and the wrapper cases whose own wait
    INTEGRATION.md documents must still hand back the verdict of the gated work."""
    assert control.ok, control.message
    cal, streams = gate
    case = build(ctx)
    assert case.entry == entry, (case.name, case.entry)
    if case.documented is None:
        assert case.waits == (sg.TABLE[entry].kind == sg.WAITS), (case.name, case.waits)
    else:                                    # a wait of the Python wrapper itself, documented in INTEGRATION.md
        assert case.waits and case.documented in stream_cases.WRAPPER_WAITS, (case.name, case.documented)
    case.name = name                         # one record and one message prefix per parametrised case
    bad = sg.run_ordered(case, streams, cal.arm(streams), cal.cases)
    assert not bad, "\n".join(bad)
