"""The input contract's table and protocol, checked without a GPU (tests/input_contract.py, tests/input_contract_rows.py):

  * the table is complete: the union of the rows' entry points is exactly the set of ``nsr_*`` names the sources of
    nerf_sr_amd/*.py call (an AST scan) that stand in ``stream_gate.TABLE``;
  * every declared exception's sentence stands where the row says;
  * the protocol itself, on CPU tensors with fake wrappers over a fake library: one forgets ``.contiguous()``, one passes a
    float64 buffer through, one writes into its input, one returns a view of a buffer it reuses, one is correct; each bad one is
    caught by the phase and check meant for it, the correct one passes, a degenerate argument is rejected."""
import ast
import ctypes
import os
import re
from collections import OrderedDict
from types import SimpleNamespace

import pytest
import torch

from tests import input_contract as ic
from tests import input_contract_rows as rows        # fills ic.ROWS
from tests.stream_gate import TABLE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "nerf_sr_amd")


# ------------------------------------------------------------------------------------------------------------ completeness
def called_entry_points():
    """``nsr_*`` names the package's sources call: attribute accesses ``lib.nsr_x`` anywhere, and -- train._TrainRun picks its
    pair by name -- the string values of dict displays and of ``.update(...)`` keywords, with the ``_e`` forms it derives."""
    found = set()
    for fname in sorted(os.listdir(PKG)):
        if not fname.endswith(".py") or fname in ("_lib.py", "build.py"):
            continue
        tree = ast.parse(open(os.path.join(PKG, fname)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and node.attr.startswith("nsr_"):
                found.add(node.attr)
            strings = []
            if isinstance(node, ast.Dict):
                strings = node.values
            elif isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "update":
                strings = [k.value for k in node.keywords]
            for v in strings:
                if isinstance(v, ast.Constant) and isinstance(v.value, str) and re.fullmatch(r"nsr_[a-z0-9_]+", v.value):
                    found.update((v.value, v.value + "_e"))
    return found & set(TABLE)


def test_the_scan_finds_the_calls():
    names = called_entry_points()
    assert {"nsr_posenc_e", "nsr_train_backward_r", "nsr_train_arch_forward_e", "nsr_refine_stitch", "nsr_adam_step_n"} <= names
    assert "nsr_forward_rays" not in names and "nsr_train_forward_e" not in names     # a label / no such entry point


def test_table_is_complete():
    covered = set()
    for name, r in list(ic.ROWS.items()) + list(rows.BINDINGS.items()):
        assert r.entries and r.entries <= set(TABLE), f"{name}: {sorted(r.entries - set(TABLE))} are no streamed entry points"
        covered |= r.entries
    called = called_entry_points()
    assert not called - covered, f"called by nerf_sr_amd but in no row: {sorted(called - covered)}"
    assert not covered - called, f"named by a row but not called by nerf_sr_amd: {sorted(covered - called)}"


def _squash(s):
    return " ".join(s.split())


def test_declared_exceptions_are_documented():
    n = 0
    for name, r in ic.ROWS.items():
        for kind, (path, sentence) in r.declared.items():
            assert kind in ic.DECLARATIONS, f"{name}: {kind}"
            text = _squash(open(os.path.join(REPO, path)).read())
            assert _squash(sentence) in text, f"{name}: {kind} is declared with words that do not stand in {path}: {sentence!r}"
            n += 1
    assert n > 0


def test_both16_values_convert_exactly():
    x = ic.both16(torch.randn(1000, generator=torch.Generator().manual_seed(0)) * 3)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        assert torch.equal(x.to(dt).to(torch.float32), x)


# ------------------------------------------------------------------------------------------ the protocol on a fake library
class FakeError(RuntimeError):
    pass


class FakeLib:
    """``nsr_fake(x, n, out, stream)``: out[i] = 2 x[i] + i over n dense fp32 values.  ``nsr_fake_bytes`` has no stream."""

    def __init__(self):
        self.launched = 0

    def nsr_fake(self, x, n, out, stream):
        self.launched += 1
        src = (ctypes.c_float * n).from_address(x.value)
        dst = (ctypes.c_float * n).from_address(out.value)
        for i in range(n):
            dst[i] = 2.0 * src[i] + i
        return 0

    def nsr_fake_bytes(self, n):
        return 4 * n


LIB = FakeLib()
FAKE = SimpleNamespace(load=lambda: LIB, NsrError=FakeError)
COLS = 4


def _launch(x, out):
    lib = FAKE.load()
    assert lib.nsr_fake_bytes(x.numel()) == 4 * x.numel()
    rc = lib.nsr_fake(ctypes.c_void_p(x.data_ptr()), x.numel(), ctypes.c_void_p(out.data_ptr()), None)
    assert rc == 0
    return out


def _checked(x, convert=False):
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a tensor")
    if x.dtype != torch.float32 and not convert:
        raise TypeError("x must be float32")
    if x.ndim != 2 or x.shape[1] != COLS:
        raise ValueError("x must be (n, 4)")
    return x.detach()


def correct(x, y=None):
    x = _checked(x, convert=True).to(torch.float32).contiguous()
    return _launch(x, torch.empty_like(x))


def forgets_contiguous(x, y=None):
    x = _checked(x)
    return _launch(x, torch.empty(x.shape, dtype=torch.float32))


def passes_float64(x, y=None):
    x = _checked(x, convert=True).contiguous()         # "converts", it says -- and hands the float64 buffer on
    return _launch(x, torch.empty(x.shape, dtype=torch.float32))


def writes_input(x, y=None):
    x = _checked(x).contiguous()
    out = _launch(x, torch.empty_like(x))
    x[0, 0] += 1.0                                      # "scratch": but a contiguous input is the caller's own memory
    return out


_REUSED = torch.zeros(64, COLS)


def returns_reused_view(x, y=None):
    x = _checked(x).contiguous()
    return _launch(x, _REUSED[: x.shape[0]])


def _call(wrapper, policy=ic.RAISES, with_y=False):
    g = torch.Generator().manual_seed(7)
    mk = lambda: ic.both16(torch.rand(6, COLS, generator=g) + 0.5)
    args = OrderedDict([("x", ic.Arg(mk(), mk(), ic.FLOAT, policy, ties=(1,)))])
    if with_y:
        args["y"] = ic.Arg(mk(), mk(), ic.FLOAT, policy, ties=(1,))
    return ic.Call(wrapper.__name__, lambda t: {"out": wrapper(t["x"], t.get("y"))}, args)


def _protocol():
    return ic.Protocol(lib_module=FAKE, streamed={"nsr_fake"}, loud=(FakeError,), skip=("cpu",), synchronize=lambda: None)


def test_phase_1_launches_nothing():
    call = _call(correct, ic.CONVERTS)
    before = LIB.launched
    v = ic.variants(call.args["x"], skip=("cpu",))
    assert {"rows", "cols", "transposed", "offset", "dtype float64", "dtype float16", "dtype bfloat16", "grad", "shape dim 1 one fewer",
            "shape extra leading dimension"} == {x.name for x in v}
    for x in v:
        verdict, line = ic.phase1(_protocol(), call, "x", x)
        assert verdict is not None, line
    assert LIB.launched == before
    assert FAKE.load() is LIB                          # the proxy is gone again


def test_the_correct_wrapper_passes():
    res = ic.run_call(_protocol(), _call(correct, ic.CONVERTS))
    assert res.lines == []
    assert res.counts[ic.RAISED] == 2 and res.counts[ic.ACCEPTED] == 8
    strict = ic.run_call(_protocol(), _call(lambda x, y=None: correct(_checked(x)), ic.RAISES))
    assert strict.lines == [] and strict.counts[ic.RAISED] == 5


def _only(lines, *needles):
    assert lines, "the bad wrapper was not caught"
    for line in lines:
        assert any(n in line for n in needles), f"caught by another check than the one meant for it: {line}"


def test_forgetting_contiguous_is_caught_in_phase_1():
    res = ic.run_call(_protocol(), _call(forgets_contiguous))
    _only(res.lines, "phase 1:")
    assert all("did not normalise" in l for l in res.lines)
    assert {"[rows]", "[cols]", "[transposed]"} == {re.search(r"\[[a-z ()_]+\]", l).group(0) for l in res.lines}


def test_a_float64_buffer_passed_through_is_caught_in_phase_1():
    res = ic.run_call(_protocol(), _call(passes_float64, ic.CONVERTS))
    _only(res.lines, "phase 1:")
    assert {"[dtype float64]", "[dtype float16]", "[dtype bfloat16]"} == {re.search(r"\[[a-z0-9 ]+\]", l).group(0) for l in res.lines}


def test_writing_into_the_input_is_caught():
    res = ic.run_call(_protocol(), _call(writes_input))
    assert any("the plain call changed the allocation of its input x" in l for l in res.lines)
    assert any("phase 2:" in l and "[offset]" in l and "changed its input's allocation" in l for l in res.lines)


def test_a_view_of_a_reused_buffer_is_caught_by_the_ownership_check():
    res = ic.run_call(_protocol(), _call(returns_reused_view))
    _only(res.lines, "does not own its memory")


def test_a_degenerate_argument_is_rejected():
    res = ic.run_call(_protocol(), _call(correct, ic.CONVERTS, with_y=True))
    degenerate = [l for l in res.lines if "degenerate argument" in l]
    assert len(degenerate) == 1 and ": y:" in degenerate[0]


def test_a_late_refusal_is_a_failure():
    def late(x, y=None):
        out = correct(x[0] if x.ndim == 3 else x)          # launches first ...
        if x.ndim != 2:
            raise ValueError("x must be (n, 4)")           # ... and looks at the shape afterwards
        return out
    res = ic.run_call(_protocol(), _call(late, ic.CONVERTS))
    _only(res.lines, "was not refused before the first library call")


def test_another_exception_type_is_a_failure():
    def sloppy(x, y=None):
        if x.shape[1] != COLS:
            raise RuntimeError("bad shape")
        return correct(x)
    res = ic.run_call(_protocol(), _call(sloppy, ic.CONVERTS))
    assert any("raised RuntimeError" in l and "not TypeError / ValueError" in l for l in res.lines)


def test_pointers_flattens_arrays_and_structs():
    class D(ctypes.Structure):
        _fields_ = [("p", ctypes.c_void_p), ("n", ctypes.c_int), ("f", ctypes.c_double)]
    arr = (ctypes.c_void_p * 2)(ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000))
    got = ic.pointers((ctypes.c_void_p(0x10), arr, ctypes.byref(D(0x3000, 5, 1.5)), 7, 2.5, None, ctypes.c_void_p(0)))
    assert {0x10, 0x1000, 0x2000, 0x3000, 5, 7} <= set(got)
