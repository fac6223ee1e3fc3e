"""The input contract of the Python layer, made testable (tests/test_gpu_input_contract.py; the protocol itself is checked on CPU
tensors with fake wrappers over a fake library in tests/test_input_contract_cpu.py).

Every wrapper of nerf_sr_amd hands ``tensor.data_ptr()`` to libnsr.so, which reads dense memory of one dtype and shape.  The
contract ("Inputs"):

    For every public callable that reaches the library with a device pointer, and for every tensor argument: an input with the
    same logical values in another memory form or dtype either gives the bits of the plain call or raises TypeError / ValueError
    before anything is enqueued.  A shape that does not fit the other arguments raises before anything is enqueued.  No call
    changes its inputs, and a result owns its memory.

``ROWS`` (tests/input_contract_rows.py fills it) has one row per public callable: the ``nsr_*`` entry points it reaches and a
builder of one small valid call -- per tensor argument an ``Arg``: two valid values A and B, its kind, its dtype policy and the
shape relations that tie it to the other arguments.

The protocol (``run_call``):

  variants   each is applied to ONE argument, the others plain, and is cut from a backing allocation made of A and B
             interleaved, so that whatever a wrapper reads by mistake is still a valid value:
             ``rows`` (every other row), ``cols`` (the leading columns of a wider backing), ``transposed`` (``.t()`` of the
             transposed data; ``permute`` for 3-D / 5-D, channels_last for 4-D), ``offset`` (``backing[1:]``), ``expanded``
             (stride 0 along a dimension in which the values repeat), ``dtype`` (float64 / float16 / bfloat16; int32 <-> int64;
             float32 for uint8 images; uint8 <-> bool for masks), ``grad`` (requires_grad on an argument the wrapper does not
             differentiate), ``cpu``, ``shape`` (one fewer along each tied dimension, one extra leading dimension).
  phase 1    behind a recording proxy in place of ``nerf_sr_amd._lib.load``: entry points without a stream parameter (sizes,
             host tables) are forwarded, every other one is RECORDED -- its name and every pointer argument, pointer arrays and
             descriptor structs flattened -- and returns NSR_OK without being called.  ``cpu`` / ``shape``, and ``dtype`` under
             the policy ``raises``: TypeError / ValueError with nothing recorded.  Forms that are not dense memory of the stated
             dtype as they stand: nothing recorded may point into the variant's backing (a wrapper that normalises passes a
             copy), or the call raised.  An exception after the first recorded call is ignored: the buffers hold nothing.
  phase 2    the real library, only for what phase 1 saw accepted: every returned tensor has the bits of the plain call, the
             whole backing is unchanged, results are contiguous (unless the row declares ``returns_views``), on the device, and
             do not overlap the backing; under ``grad`` no result has a ``grad_fn``.  A loud library error is an accepted outcome
             for ``offset`` alone (an alignment the launcher checks).
  sensitivity  per argument: the call on a contiguous clone of what a wrapper that forgot to normalise would have read (numel
             elements taken densely at the ``rows`` view's pointer) must differ in bits from the plain call -- else the argument
             does not influence the outputs at this shape and the row shows nothing.
  ownership  call with A, keep the result; call with B; A's result still holds A's bits (unless the row declares
             ``reuses_output`` / ``returns_input`` with the sentence that documents it)."""
import ctypes
import time
from collections import OrderedDict
from typing import Callable, Dict, List, NamedTuple, Optional

import torch

from tests import scratch_state as ss

RAISES, CONVERTS = "raises", "converts"
FLOAT, INDEX, U8, MASK = "float values", "integer indices", "uint8 image", "bool / uint8 mask"
RAISED, ACCEPTED, NOT_APPLICABLE = "raised", "accepted", "not applicable"
DECLARATIONS = ("reuses_output", "returns_input", "returns_views")


class Arg:
    """One tensor argument of a call.

    A, B        two valid values of the same shape and dtype (B only ever fills what a wrong read would reach)
    kind        FLOAT, INDEX, U8 or MASK
    policy      what the wrapper's docstring says about another dtype: RAISES or CONVERTS
    ties        the dimensions whose extent is tied to another argument or to the kernel (``shape``: one fewer along each)
    ndim_tied   an extra leading dimension must raise (False where the wrapper documents that it flattens leading dimensions)
    repeat      a dimension along which the values of A and of B repeat (``expanded``), or None
    differentiable   the wrapper back-propagates to this argument: no ``grad`` variant
    host_ok     the argument may live on the host (the wrapper moves it, as the reference's does): ``cpu`` is not applicable
    as_is       further dtypes the wrapper reads as they stand (a uint8 mask where bool is stated)
    follows     outputs take this argument's dtype (the metrics): a ``dtype`` variant is compared in that dtype
    per_item    the wrapper takes the argument item by item (a stack of images): a form whose items ``t[i]`` are dense is read in
                place, as a list of dense images would be"""

    def __init__(self, A, B, kind=FLOAT, policy=RAISES, ties=(), ndim_tied=True, repeat=None, differentiable=False, host_ok=False,
                 as_is=(), follows=False, per_item=False):
        self.per_item = bool(per_item)
        assert A.shape == B.shape and A.dtype == B.dtype, "A and B must have one shape and dtype"
        self.A, self.B, self.kind, self.policy = A, B, kind, policy
        self.ties, self.ndim_tied, self.repeat = tuple(ties), bool(ndim_tied), repeat
        self.differentiable, self.host_ok, self.as_is, self.follows = bool(differentiable), bool(host_ok), tuple(as_is), bool(follows)


class Call:
    """One small valid call: ``fn(name -> tensor) -> name -> returned tensor`` over ``args`` (name -> Arg).  ``fn`` restores
    whatever state the callable updates in place, so that equal inputs give equal bits.  ``declared``: kind (DECLARATIONS) ->
    (file, words of the sentence that documents it)."""

    def __init__(self, name: str, fn: Callable, args: "OrderedDict[str, Arg]", declared: Optional[dict] = None):
        self.name, self.fn, self.args, self.declared = name, fn, OrderedDict(args), dict(declared or {})
        assert set(self.declared) <= set(DECLARATIONS), self.declared


class Row(NamedTuple):
    entries: frozenset              # the nsr_* entry points (of stream_gate.TABLE) the callable reaches
    build: Callable                 # build(ctx) -> Call
    declared: dict                  # kind -> (file relative to the repository, sentence), checked on the CPU


ROWS: "OrderedDict[str, Row]" = OrderedDict()


def row(name: str, entries, declared: Optional[dict] = None):
    def deco(fn):
        assert name not in ROWS, name
        ROWS[name] = Row(frozenset(entries), fn, dict(declared or {}))
        return fn
    return deco


# ----------------------------------------------------------------------------------------------------------------- variants
class Variant(NamedTuple):
    name: str
    tensor: torch.Tensor
    backing: torch.Tensor           # the allocation the tensor is cut from (the tensor itself where it owns its memory)
    expect: str                     # "raise" | "copy" (no recorded pointer in the backing, or raised) | "any"


def _span(t: torch.Tensor):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


def storage_bytes(t: torch.Tensor) -> torch.Tensor:
    """A copy of every byte of the allocation behind ``t``."""
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).clone()


def _interleave(A, B, dim=0):
    return torch.stack([A, B], dim + 1).reshape(*A.shape[:dim], 2 * A.shape[dim], *A.shape[dim + 1:]).contiguous()


def other_dtypes(arg: Arg):
    if arg.kind == FLOAT:       # stated float32 (float64 for the warp's locations): the three others
        return tuple(d for d in (torch.float64, torch.float32, torch.float16, torch.bfloat16) if d != arg.A.dtype)[:3]
    if arg.kind == U8:
        return (torch.float32,)
    if arg.kind == INDEX:
        return (torch.int32,) if arg.A.dtype == torch.int64 else (torch.int64,)
    return (torch.uint8,) if arg.A.dtype == torch.bool else (torch.bool,)


def variants(arg: Arg, skip=()) -> List[Variant]:
    """Every variant of one argument, each with the logical values of ``arg.A``."""
    A, B, out = arg.A.detach(), arg.B.detach(), []

    def add(name, t, backing, expect):
        if name.split(" ")[0] in skip:
            return
        if expect == "copy" and arg.per_item and t.dtype == A.dtype and all(x.is_contiguous() for x in t):
            expect = "any"
        if expect == "copy":
            assert not (t.is_contiguous() and t.dtype == A.dtype) or name.startswith("expanded"), f"{name}: the variant is dense"
        assert t.shape == A.shape or name.startswith("shape"), name
        out.append(Variant(name, t, backing, expect))

    if A.ndim >= 1 and A.shape[0] >= 1:
        b = _interleave(A, B, 0)
        if A.shape[0] > 1 or A.ndim > 1:
            v = b[::2]
            if not v.is_contiguous():
                add("rows", v, b, "copy")
        b = torch.cat([B[:1], A], 0).contiguous()
        add("offset", b[1:], b, "any")
    if A.ndim >= 2:
        b = torch.cat([A, B], -1).contiguous()
        v = b[..., :A.shape[-1]]
        if not v.is_contiguous():
            add("cols", v, b, "copy")
        if A.ndim == 2:
            b = torch.stack([A.t().contiguous(), B.t().contiguous()])
            v, how = b[0].t(), "transposed"
        elif A.ndim == 4:
            b = torch.cat([A, B], 0).contiguous(memory_format=torch.channels_last)
            v, how = b[:A.shape[0]], "transposed (channels_last)"
        else:
            b = torch.stack([A.movedim(-1, 0).contiguous(), B.movedim(-1, 0).contiguous()])
            v, how = b[0].movedim(0, -1), "transposed (permute)"
        if not v.is_contiguous():
            add(how, v, b, "copy")
    if arg.repeat is not None:
        d = arg.repeat
        assert torch.equal(A, A.narrow(d, 0, 1).expand_as(A)), "repeat: the values of A do not repeat along that dimension"
        b = torch.cat([A, B], 0).contiguous()
        strides = list(A.contiguous().stride())
        strides[d] = 0
        add("expanded", b.as_strided(A.shape, strides, 0), b, "copy")
    for dt in other_dtypes(arg):
        t = A.to(dt)
        expect = "any" if dt in arg.as_is else ("copy" if arg.policy == CONVERTS else "raise")
        if expect != "raise":       # a variant that may be accepted must hold the same logical values
            assert torch.equal(t.to(A.dtype), A), f"dtype {dt}: the values of A are not representable (see ``both16``)"
        add(f"dtype {str(dt).replace('torch.', '')}", t, t, expect)
    if A.dtype.is_floating_point and not arg.differentiable:
        t = A.clone().requires_grad_(True)
        add("grad", t, t, "any")
    if A.is_cuda and not arg.host_ok:
        t = A.cpu()
        add("cpu", t, t, "raise")
    for d in arg.ties:
        if A.shape[d] > 1:
            t = A.narrow(d, 0, A.shape[d] - 1).contiguous()
            add(f"shape dim {d} one fewer", t, t, "raise")
    if arg.ndim_tied:
        t = A.unsqueeze(0).contiguous()
        add("shape extra leading dimension", t, t, "raise")
    return out


def forgotten(v: Variant) -> torch.Tensor:
    """What a wrapper that forgot to normalise would have read: numel elements taken densely at the view's pointer."""
    lo, _ = _span(v.backing)
    flat = torch.empty(0, dtype=v.tensor.dtype, device=v.tensor.device).set_(v.backing.untyped_storage())
    first = (v.tensor.data_ptr() - lo) // v.tensor.element_size()
    return flat[first:first + v.tensor.numel()].reshape(v.tensor.shape).clone()


# ------------------------------------------------------------------------------------------------------- the recording proxy
def pointers(args) -> List[int]:
    """Every integer a recorded call was handed, pointer arrays and descriptor structs flattened (a count or an option word is no
    device address, so it never lies inside a backing allocation)."""
    out = []

    def walk(a, depth=0):
        if a is None or isinstance(a, (float, bytes, str)) or depth > 4:
            return
        if isinstance(a, bool):
            return
        if isinstance(a, int):
            out.append(a)
        elif isinstance(a, ctypes.Array):
            for x in a:
                walk(x, depth + 1)
        elif isinstance(a, ctypes.Structure):
            for f in a._fields_:
                walk(getattr(a, f[0]), depth + 1)
        elif isinstance(a, ctypes._SimpleCData):
            walk(a.value, depth + 1)
        elif hasattr(a, "_obj"):                 # ctypes.byref(...)
            walk(a._obj, depth + 1)
    for a in args:
        walk(a)
    return out


class Recorder:
    """Stands in for the loaded library: names in ``streamed`` are recorded and answer NSR_OK, the rest is forwarded."""

    def __init__(self, real, streamed):
        self._real, self._streamed, self.calls = real, streamed, []

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._streamed:
            return getattr(self._real, name)

        def stub(*args):
            self.calls.append((name, pointers(args)))
            return 0
        return stub


class Protocol:
    """Where the library is loaded from (``lib_module.load``), which of its names take a stream, what a loud library error is."""

    def __init__(self, lib_module=None, streamed=None, loud=None, skip=(), synchronize=None):
        if lib_module is None:
            from nerf_sr_amd import _lib as lib_module
        if streamed is None:
            from tests.stream_gate import TABLE
            streamed = frozenset(TABLE)
        if loud is None:
            loud = (lib_module.NsrError,)
        self.lib_module, self.streamed, self.loud, self.skip = lib_module, frozenset(streamed), tuple(loud), tuple(skip)
        self.synchronize = synchronize or (lambda: torch.cuda.synchronize() if torch.cuda.is_available() else None)

    def record(self, fn, tensors):
        """(recorded calls, exception or None) of ``fn(tensors)`` behind the proxy; nothing of ``streamed`` runs."""
        mod = self.lib_module
        real_load = mod.load
        rec = Recorder(real_load(), self.streamed)
        mod.load = lambda: rec
        try:
            try:
                fn(tensors)
            except Exception as e:      # noqa: BLE001 -- the verdict decides what the exception means
                return rec.calls, e
            return rec.calls, None
        finally:
            mod.load = real_load
            self.synchronize()


def phase1(p: Protocol, call: Call, name: str, v: Variant):
    """(RAISED | ACCEPTED | None, line): None with a line is a failure."""
    tensors = OrderedDict((k, a.A) for k, a in call.args.items())
    tensors[name] = v.tensor
    calls, exc = p.record(call.fn, tensors)
    who = f"{call.name}: {name} [{v.name}] {tuple(v.tensor.shape)} {v.tensor.dtype} strides {tuple(v.tensor.stride())}"
    raised = exc is not None and not calls
    if raised and not isinstance(exc, (TypeError, ValueError)):
        return None, f"{who}: raised {type(exc).__name__} ({exc}) before anything was enqueued, not TypeError / ValueError"
    if v.expect == "raise":
        if raised:
            return RAISED, None
        return None, (f"{who}: was not refused before the first library call"
                      + (f" ({calls[0][0]} was reached)" if calls else " (the call returned without reaching the library)"))
    if raised:
        return RAISED, None
    if v.expect == "copy":
        lo, hi = _span(v.backing)
        for entry, ptrs in calls:
            for q in ptrs:
                if lo <= q < hi:
                    return None, (f"{who}: {entry} was handed a pointer {q - lo} bytes into the variant's own allocation "
                                  f"({hi - lo} bytes): the wrapper did not normalise it")
    return ACCEPTED, None


def _bits(res) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, t.detach().clone()) for k, t in res.items() if isinstance(t, torch.Tensor))


def phase2(p: Protocol, call: Call, name: str, v: Variant, want) -> List[str]:
    arg = call.args[name]
    tensors = OrderedDict((k, a.A) for k, a in call.args.items())
    tensors[name] = v.tensor
    who = f"{call.name}: {name} [{v.name}]"
    before = storage_bytes(v.backing)
    try:
        res = call.fn(tensors)
        p.synchronize()
    except p.loud as e:
        if v.name == "offset":
            return []
        return [f"{who}: the library refused it ({e}): only an `offset` view may end in a loud error"]
    lines = []
    got = _bits(res)
    if v.name.startswith("dtype") and arg.follows:
        want = OrderedDict((k, t.to(v.tensor.dtype) if t.dtype.is_floating_point and got.get(k) is not None
                            and got[k].dtype == v.tensor.dtype else t) for k, t in want.items())
    lines += [f"{who}: not the bits of the plain call: {line}" for line in ss.diff_all("", got, want)]
    if not ss.same_bits(storage_bytes(v.backing), before):
        lines.append(f"{who}: the call changed its input's allocation")
    lines += [f"{who}: {line}" for line in check_results(call, res, [v.backing], device=arg.A.device)]
    if v.name == "grad":
        for k, t in res.items():
            if isinstance(t, torch.Tensor) and (t.grad_fn is not None or t.requires_grad):
                lines.append(f"{who}: result {k} carries a grad_fn for an argument the wrapper does not differentiate")
    return lines


def check_results(call: Call, res, backings, device) -> List[str]:
    lines = []
    for k, t in res.items():
        if not isinstance(t, torch.Tensor):
            continue
        if not t.is_contiguous() and "returns_views" not in call.declared:
            lines.append(f"result {k} {tuple(t.shape)} is not contiguous (strides {tuple(t.stride())})")
        if t.device.type != torch.device(device).type:
            lines.append(f"result {k} lives on {t.device}")
        if "returns_input" in call.declared:
            continue
        lo, hi = _span(t)
        for b in backings:
            blo, bhi = _span(b)
            if lo < bhi and blo < hi and t.numel() > 0:
                lines.append(f"result {k} overlaps an input's allocation")
    return lines


class Result(NamedTuple):
    lines: List[str]
    counts: Dict[str, int]
    wall_s: float


def run_call(p: Protocol, call: Call) -> Result:
    """The whole protocol for one call."""
    t0 = time.perf_counter()
    lines, counts = [], {RAISED: 0, ACCEPTED: 0, NOT_APPLICABLE: 0}
    A = OrderedDict((k, a.A) for k, a in call.args.items())
    B = OrderedDict((k, a.B) for k, a in call.args.items())
    before = [storage_bytes(t) for t in A.values()]
    kept = call.fn(A)
    p.synchronize()
    want = _bits(kept)
    lines += [f"{call.name}: the plain call changed the allocation of its input {k}"
              for (k, t), b in zip(A.items(), before) if not ss.same_bits(storage_bytes(t), b)]
    assert want, f"{call.name}: the call returns no tensor"
    lines += [f"{call.name}: plain call: {line}" for line in check_results(call, kept, list(A.values()), next(iter(A.values())).device)]
    res_b = call.fn(B)
    p.synchronize()
    if not [k for k in want if not ss.same_bits(want[k], res_b[k].detach())]:
        lines.append(f"{call.name}: degenerate call: input sets A and B give the same bits")
    if "reuses_output" not in call.declared and "returns_input" not in call.declared:
        lines += [f"{call.name}: a result does not own its memory: after a call with other inputs, {line}"
                  for line in ss.diff_all("", _bits(kept), want)]
    del kept, res_b
    again = _bits(call.fn(A))
    p.synchronize()
    lines += [f"{call.name}: the plain call is not reproducible (state left behind?): {line}" for line in ss.diff_all("", again, want)]
    for name, arg in call.args.items():
        vs = variants(arg, p.skip)
        if arg.host_ok:
            counts[NOT_APPLICABLE] += 1
        dense = next((v for v in vs if v.name == "rows"), None) or next((v for v in vs if v.name == "offset"), None)
        if dense is not None:
            tensors = OrderedDict(A)
            tensors[name] = forgotten(dense)
            got = _bits(call.fn(tensors))
            p.synchronize()
            if not ss.diff_all("", got, want):
                lines.append(f"{call.name}: {name}: degenerate argument: what a wrapper that forgot to normalise the `{dense.name}` view "
                             "would have read gives the bits of the plain call")
        for v in vs:
            verdict, line = phase1(p, call, name, v)
            if verdict is None:
                lines.append("phase 1: " + line)
                continue
            counts[verdict] += 1
            if verdict == ACCEPTED:
                lines += ["phase 2: " + l for l in phase2(p, call, name, v, want)]
    return Result(lines, counts, time.perf_counter() - t0)


# ------------------------------------------------------------------------------------------------ values both 16-bit formats hold
def both16(t: torch.Tensor) -> torch.Tensor:
    """``t`` rounded to values that float16 AND bfloat16 hold exactly (8 significant bits, nothing below 2^-14): the inputs of a
    ``converts`` argument, so that its float16 / bfloat16 variants have the same logical values."""
    r = t.to(torch.bfloat16).to(torch.float32)
    return torch.where(r.abs() < 2.0 ** -14, torch.zeros_like(r), r).clamp(-60000.0, 60000.0)
