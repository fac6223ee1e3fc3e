"""tests/test_gpu_scratch_state.py for precision 'f16x3_gemm_bwd' (NSR_F16X3_GEMM_BWD): its workspace -- 'f16x3_gemm''s layout plus
a tail of transposed split weight copies and range words -- is pure scratch behind the status block and its stated size
suffices.  The machinery is that file's: runs whose workspaces were filled with zeros, with 0xFF bytes and with the bytes
another call left behind give identical outputs and gradients, every output is fully overwritten, and the guard bands behind
the stated sizes stay intact."""
import pytest
import torch

from . import scratch_state as ss
from .test_gpu_scratch_state import ZERO, _arch_pair, _assert_live, _default_pair, _four_runs, _fused_run, _snap
from .test_gpu_scratch_state import arch_batch, batch, lib  # noqa: F401  -- that module's fixtures

pytestmark = pytest.mark.gpu
PREC = "f16x3_gemm_bwd"


@pytest.mark.parametrize("embed,chunk", [(e, c) for e in (0, 1) for c in ss.ARCH_CHUNKS])
def test_arch_training_workspace_is_scratch(arch_batch, embed, chunk):      # noqa: F811
    """nsr_train_arch_forward / _backward[_e] on the case of that file (D = 3, W = 48 -> Wp = 64, a skip at layer 1, 7 rays: 3.5
    tiles of 128 coarse points; chunks of 3 rays).  LEFTOVER: what 'f16x3_gemm' left at 4 rays under the other embedding word."""
    def donor():
        _, _, ws, after_forward, _ = _arch_pair(arch_batch, "f16x3_gemm", 1 - embed, 0, ZERO, None, R=4)
        return torch.cat([after_forward, _snap(ws)])
    case = f"arch train {PREC} embed={embed} ray_chunk={chunk}"
    _assert_live(case, _four_runs(case, lambda f, l: _arch_pair(arch_batch, PREC, embed, chunk, f, l)[:2], donor))


@pytest.mark.parametrize("entry,chunk", [("fused", 0), ("fused", 40), ("pair", 40)])
def test_default_training_workspace_is_scratch(batch, entry, chunk):      # noqa: F811
    """nsr_train_loss_and_grads and the nsr_train_forward / nsr_train_backward pair on the default network (the batch of
    tests/golden/train_llff_rand.npz; 40-ray chunks leave a ragged 16-ray pass).  LEFTOVER: the chain pair's bytes at 32 rays."""
    def donor():
        _, _, ws, after_forward, _ = _default_pair(batch, "f16x3", 0, ZERO, None, R=32)
        return torch.cat([after_forward, _snap(ws)])
    if entry == "fused":
        run = lambda f, l: _fused_run(batch, PREC, chunk, f, l)[:2]
    else:
        run = lambda f, l: _default_pair(batch, PREC, chunk, f, l)[:2]
    case = f"train {entry} {PREC} ray_chunk={chunk}"
    _assert_live(case, _four_runs(case, run, donor))
