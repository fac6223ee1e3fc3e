"""Every public callable of nerf_sr_amd that reaches libnsr.so with a tensor pointer keeps the input contract (INTEGRATION.md,
"Inputs"): another memory form or dtype of the same values gives the bits of the plain call or raises TypeError / ValueError
before anything is enqueued; a shape that does not fit raises before anything is enqueued; no call changes its inputs; a result
owns its memory.  The autograd bindings give the same gradients however the upstream gradient is delivered.

The protocol and the variants are tests/input_contract.py, the rows and the bindings tests/input_contract_rows.py.  Phase 1 runs
behind a recording proxy and launches nothing; only what it saw accepted reaches a kernel (phase 2), always inside its backing
allocation and made of valid values.  A failure names the row, the argument, the variant and the tensor.

NSR_RECORD_PROFILES=1 writes the per-row counts (variants raised / accepted / not applicable) and wall times to
profiles/input_contract.json."""
import json
import os
import time
from collections import OrderedDict

import pytest
import torch

from tests import input_contract as ic
from tests import input_contract_rows as rows
from tests import stream_cases

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import _lib
    _lib.load()
    return stream_cases.Ctx()


@pytest.fixture(scope="module")
def profile():
    doc, t0 = OrderedDict(), time.time()
    yield doc
    if os.environ.get("NSR_RECORD_PROFILES") and doc:
        out = {"what": "tests/test_gpu_input_contract.py: per row the (argument, variant) pairs that were refused before the first library "
                       "call (raised), ran on the real library with the bits of the plain call (accepted), the arguments that may live on "
                       "the host (not applicable: no `cpu` variant), and the wall time of the whole row, builder included",
               "device": torch.cuda.get_device_name(0), "wall_s": round(time.time() - t0, 2), "rows": doc}
        with open(os.path.join(REPO, "profiles", "input_contract.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


def _stop_on_fault(exc: BaseException):
    """Nothing more is started on a device that reported a fault."""
    text = str(exc).lower()
    if "illegal memory access" in text or "hip error" in text or "hiperror" in text:
        pytest.exit(f"the device reported a fault, nothing more is run: {exc}", returncode=3)


@pytest.mark.parametrize("name", list(ic.ROWS))
def test_input_contract(ctx, profile, name):
    try:
        _row(ctx, profile, name)
    except Exception as e:      # noqa: BLE001
        _stop_on_fault(e)
        raise


def _row(ctx, profile, name):
    r = ic.ROWS[name]
    t0 = time.perf_counter()
    call = r.build(ctx)
    assert call.declared == r.declared, (name, call.declared, r.declared)
    p = ic.Protocol()
    # the row names the entry points the call reaches (the table's completeness rests on it): the plain call behind the proxy
    calls, exc = p.record(call.fn, OrderedDict((k, a.A) for k, a in call.args.items()))
    reached = {entry for entry, _ in calls}
    assert reached <= r.entries, f"{name}: reaches {sorted(reached - r.entries)}, which its row does not name"
    assert exc is not None or reached == r.entries, f"{name}: its row names {sorted(r.entries - reached)}, which the call does not reach"
    call = r.build(ctx)       # afresh: what the recorded call allocated (a workspace, its status block) was never initialised
    res = ic.run_call(p, call)
    wall = time.perf_counter() - t0
    profile[name] = {"raised": res.counts[ic.RAISED], "accepted": res.counts[ic.ACCEPTED], "not_applicable": res.counts[ic.NOT_APPLICABLE],
                     "arguments": len(call.args), "wall_s": round(wall, 3)}
    print(f"\n{name}: {res.counts}, {wall:.2f} s")
    assert not res.lines, "\n".join(res.lines)
    assert res.counts[ic.ACCEPTED] > 0 and res.counts[ic.RAISED] > 0, f"{name}: {res.counts}: the row shows nothing"


@pytest.mark.parametrize("name", list(rows.BINDINGS))
def test_autograd_binding(ctx, name):
    try:
        lines = rows.BINDINGS[name].run(ctx)
    except Exception as e:      # noqa: BLE001
        _stop_on_fault(e)
        raise
    assert not lines, "\n".join(lines)
