"""The table of tests/stream_gate.py is complete, and the protocol's bookkeeping works -- on CPU tensors, without a GPU.

  * the rows of ``TABLE`` are exactly the prototypes of include/*.h that take a ``void* stream`` (comments stripped): a new entry
    point cannot land without a row, a removed one cannot leave a dead row;
  * a ``WAITS`` row names the header and words of the sentence that document the wait, and they stand there;
  * every row has a case in tests/stream_cases.py, and the waits of the Python layer that the wrapper cases name are documented
    in INTEGRATION.md;
  * ``run_serial`` / ``run_gated`` / ``verdict`` on a deferred queue of CPU tensors: a call that reads early, a call that waits,
    a memset that runs early, a lost status word and a degenerate case are each reported; a well-behaved call is not."""
import glob
import os
import re
from collections import OrderedDict

import pytest
import torch

from tests import stream_cases, stream_gate as sg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stripped(path):
    s = open(path).read()
    s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
    return re.sub(r"//[^\n]*", " ", s)


def stream_prototypes(include_dir=os.path.join(REPO, "include")):
    """name -> header of every prototype with a ``void* stream`` parameter."""
    found = OrderedDict()
    for path in sorted(glob.glob(os.path.join(include_dir, "*.h"))):
        for m in re.finditer(r"\b(?:int|size_t|int64_t)\s+(nsr_\w+)\s*\(([^;{}]*?)\)\s*;", _stripped(path), flags=re.S):
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
                assert m.group(1) not in found, f"{m.group(1)} declared twice"
                found[m.group(1)] = os.path.basename(path)
    return found


def test_the_table_is_exactly_the_stream_prototypes():
    protos = stream_prototypes()
    assert len(protos) >= 77, len(protos)
    missing, dead = sorted(set(protos) - set(sg.TABLE)), sorted(set(sg.TABLE) - set(protos))
    assert not missing, f"entry points with a `void* stream` and no row in tests/stream_gate.py TABLE: {missing}"
    assert not dead, f"rows of tests/stream_gate.py TABLE without a prototype in include/*.h: {dead}"


def test_a_deleted_row_is_noticed(monkeypatch):
    """The completeness test fails when a row goes."""
    table = OrderedDict(sg.TABLE)
    del table["nsr_sr_mean"]
    monkeypatch.setattr(sg, "TABLE", table)
    with pytest.raises(AssertionError, match="nsr_sr_mean"):
        test_the_table_is_exactly_the_stream_prototypes()


def _comment_text(path):
    """The header's text with the comment frames' line starts removed and whitespace collapsed."""
    s = re.sub(r"\n\s*\*\s?", " ", open(path).read())
    return re.sub(r"\s+", " ", s)


def test_waits_rows_quote_their_header():
    protos = stream_prototypes()
    for name, row in sg.TABLE.items():
        assert row.kind in (sg.ENQUEUE_ONLY, sg.WAITS), name
        if row.kind == sg.ENQUEUE_ONLY:
            assert row.header is None and row.sentence is None, name
            continue
        assert row.header and row.sentence and not row.capture, name
        text = _comment_text(os.path.join(REPO, "include", row.header))
        assert re.sub(r"\s+", " ", row.sentence) in text, f"{name}: include/{row.header} does not say {row.sentence!r}"
        assert protos[name] == row.header, name


def test_the_waits_set_is_the_headers():
    """Every place the headers say a call waits for its stream belongs to a WAITS row: the sentences of the rows cover every
    occurrence of 'waits for' / 'WAITS for' in include/*.h."""
    sentences = {(r.header, re.sub(r"\s+", " ", r.sentence)) for r in sg.TABLE.values() if r.kind == sg.WAITS}
    for path in sorted(glob.glob(os.path.join(REPO, "include", "*.h"))):
        text = _comment_text(path)
        for m in re.finditer(r"(?i)\bwaits\s+for\b", text):
            near = text[max(0, m.start() - 120): m.end() + 60]
            assert any(h == os.path.basename(path) and (s in near) for h, s in sentences), \
                f"{os.path.basename(path)}: '...{text[max(0, m.start() - 60): m.end() + 30]}...' is documented but no WAITS row quotes it"
    waits = {k for k, r in sg.TABLE.items() if r.kind == sg.WAITS}
    assert {"nsr_pack_weights", "nsr_weights_status", "nsr_train_status", "nsr_train_backward", "nsr_refine_train_backward"} <= waits


def test_every_row_has_a_case():
    have = set(stream_cases.CASES)
    assert have == set(sg.TABLE), sorted(have ^ set(sg.TABLE))
    names = [c[0] for c in stream_cases.all_cases()]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    captured = {c[1] for c in stream_cases.all_cases() if sg.TABLE[c[1]].capture}
    assert captured == {k for k, r in sg.TABLE.items() if r.capture}


def test_wrapper_waits_are_documented():
    text = re.sub(r"\s+", " ", open(os.path.join(REPO, "INTEGRATION.md")).read())
    for key, words in stream_cases.WRAPPER_WAITS.items():
        assert words in text, f"INTEGRATION.md does not document the wrapper wait {key!r}: {words!r}"


# ------------------------------------------------------------------------------------------- the protocol on CPU tensors
class QueueStreams:
    """A side 'stream' that runs nothing until it is synchronised: what a closed gate looks like from the host."""

    def __init__(self):
        self.queue, self.gated = [], False

    class _Ctx:
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    def side(self):
        return self._Ctx()

    def gate(self):
        self.gated = True

    def enqueue(self, fn):
        if self.gated:
            self.queue.append(fn)
        else:
            fn()

    def copy(self, dst, src):
        src = src.clone()
        self.enqueue(lambda: dst.copy_(src))

    def query(self):
        return not self.queue

    def synchronize(self):
        for fn in self.queue:
            fn()
        self.queue, self.gated = [], False


def _toy(streams, behaviour="good", same_inputs=False):
    """out = 2 x + acc, acc += 1 (in place), scratch zeroed by a 'memset' first; the status word is x[0] > 5."""
    x = torch.zeros(4)
    acc = torch.zeros(4)
    out = torch.zeros(4)
    scratch = torch.full((4,), 7.0)
    word = []

    def work():
        out.copy_(2 * x + acc + scratch)
        acc.add_(1)
        word.append(int(x[0] > 5))
        scratch.fill_(7.0)                              # a workspace comes back dirty

    def call(_host):
        if behaviour == "reads early":                  # the launch left the stream
            work()
            return
        if behaviour == "memset early":
            scratch.zero_()
        else:
            streams.enqueue(lambda: scratch.zero_())
        streams.enqueue(work)
        if behaviour == "waits":
            streams.synchronize()
    A = {"x": torch.tensor([9.0, 1, 2, 3])}
    B = {"x": A["x"].clone() if same_inputs else torch.tensor([1.0, 5, 6, 7])}
    status = (lambda h: (0,)) if behaviour == "loses status" else (lambda h: (word[-1],))
    return sg.Case(f"toy[{behaviour}]", "nsr_sr_mean", call, bufs={"x": x}, A=A, B=B, state={"acc": acc}, outs={"out": out},
                   scratch={"scratch": scratch}, status=status)


def _run(behaviour, waits=False):
    streams = QueueStreams()
    case = _toy(streams, behaviour)
    case.waits = waits
    serial = sg.run_serial(case, sg.SerialStreams())
    got = sg.run_gated(case, serial, streams)
    return sg.verdict(case, serial, got, gate_ms=1e6)


def test_a_well_behaved_call_passes():
    assert _run("good") == []


def test_an_early_read_carries_the_stale_bits():
    bad = _run("reads early")
    assert any("out out" in line and "input set B's bits" in line for line in bad), bad
    assert any("status words" in line for line in bad), bad


def test_an_early_memset_is_overwritten_by_the_stale_scratch():
    bad = _run("memset early")
    assert any("out out" in line and "neither A's nor B's" in line for line in bad), bad


def test_a_hidden_wait_is_reported_unless_the_row_waits():
    bad = _run("waits")
    assert any("waited for its stream" in line for line in bad), bad
    assert _run("waits", waits=True) == []


def test_a_slow_call_is_reported():
    streams = QueueStreams()
    case = _toy(streams)
    serial = sg.run_serial(case, sg.SerialStreams())
    got = sg.run_gated(case, serial, streams)._replace(host_ms=60.0)
    assert any("it blocks" in line for line in sg.verdict(case, serial, got, gate_ms=100.0))
    assert sg.verdict(case, serial, got._replace(host_ms=49.0), gate_ms=100.0) == []


def test_a_lost_status_word_is_reported():
    streams = QueueStreams()
    case = _toy(streams, "loses status")
    serial = sg.run_serial(case, sg.SerialStreams())
    serial = serial._replace(want_A=serial.want_A._replace(status=(1,)))
    assert any("status words" in line for line in sg.verdict(case, serial, sg.run_gated(case, serial, streams), gate_ms=1e6))


def test_degenerate_inputs_are_refused():
    with pytest.raises(AssertionError, match="degenerate"):
        sg.run_serial(_toy(QueueStreams(), same_inputs=True), sg.SerialStreams())


def test_a_case_checks_its_shapes():
    with pytest.raises(ValueError, match="same keys"):
        sg.Case("x", "nsr_sr_mean", lambda h: None, bufs={"x": torch.zeros(2)}, A={"x": torch.zeros(2)}, B={})
    with pytest.raises(ValueError, match="the buffer"):
        sg.Case("x", "nsr_sr_mean", lambda h: None, bufs={"x": torch.zeros(2)}, A={"x": torch.zeros(3)}, B={"x": torch.zeros(2)})


def test_gate_length_rule():
    cal = sg.Calibration.__new__(sg.Calibration)
    cal.cycles_per_ms, cal.slowest_ms, cal.cases = 1000.0, 0.0, {}
    assert cal.gate_ms(0.5) == sg.GATE_FLOOR_MS
    assert cal.gate_ms(12.0) == 240.0
    assert cal.gate_ms(1.0) == 240.0            # the slowest case of the session so far decides
    streams = sg.TorchStreams()
    assert cal.arm(streams)(1.0) == 240.0 and streams.cycles == 240000
