"""The enqueue-only entry points a caller would capture replay bit for bit from a graph (include/nsr.h: "can be captured in a graph";
include/nsr_metrics.h, include/nsr_losses.h: "no host synchronisation").

For every case of tests/stream_cases.py whose row of stream_gate.TABLE is marked ``capture``: the eager results of input sets A
and B (the serial runs of the ordering protocol), then, with B in the static buffers, a warm-up on a side stream, ONE call
captured into a ``torch.cuda.CUDAGraph``, A copied into the static buffers, the stale outputs and the displaced workspace bytes of the ordering protocol put back, a replay -- and the outputs, the state updated in
place and the status words must be the eager ones of A.  One stream, no parallel branches."""
import pytest
import torch

from tests import stream_cases, stream_gate as sg

pytestmark = pytest.mark.gpu
CAPTURED = [c for c in stream_cases.all_cases() if sg.TABLE[c[1]].capture and "wrapper" not in c[0]]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import _lib
    _lib.load()
    return stream_cases.Ctx()


def test_every_capture_row_has_a_case():
    rows = {k for k, r in sg.TABLE.items() if r.capture}
    assert rows == {c[1] for c in CAPTURED}, sorted(rows ^ {c[1] for c in CAPTURED})
    assert all(sg.TABLE[k].kind == sg.ENQUEUE_ONLY for k in rows)


@pytest.mark.parametrize("name,entry,build", CAPTURED, ids=[c[0] for c in CAPTURED])
def test_replay_has_the_eager_bits(ctx, name, entry, build):
    case = build(ctx)
    case.name = name
    serial = sg.run_serial(case)                       # the buffers now hold what B left
    streams = sg.SerialStreams()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture
        case.call(case.host_B)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if case.status:
        case.status(case.host_B)                       # clears the words the warm-up raised
    sg._load(case, streams, "B")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        returned = case.call(case.host_A)              # host arguments are frozen into the graph: A's
    sg._load(case, streams, "A")                       # the static inputs and the pristine in-place state
    for k, v in case.outs.items():
        v.copy_(serial.stale[f"out {k}"])
    for k, v in case.scratch.items():                  # the displaced bytes of the ordering protocol: a replay reads no leftovers
        v.copy_(serial.stale[f"scratch {k}"])
    graph.replay()
    torch.cuda.synchronize()
    got = sg._collect(case, returned)
    bad = []
    for k, want in serial.want_A.bits.items():
        line = sg.ss.diff(k, got[k], want)
        if line:
            bad.append(f"{case.name}: replay: {line}")
    status = case.status(case.host_A) if case.status else None
    if status != serial.want_A.status:
        bad.append(f"{case.name}: status words {status} after the replay, {serial.want_A.status} eagerly")
    assert not bad, "\n".join(bad)
