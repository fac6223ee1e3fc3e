"""Every documented build variant (nerf_sr_amd/build.py VARIANTS: the timeline stamps and the ablation switches of the
measurement ladders) still COMPILES for gfx950 and still honours the inline-asm ISA contract -- on the CPU box, so that the
instruments inside the product translation units cannot rot between the rounds that use them (VERDICT r4 'next' #6).  hipcc -S
of the touched units only; listings are cached by source hash."""
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from nerf_sr_amd import build as nsr_build


def test_every_documented_variant_compiles_and_keeps_the_isa_contract():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    names = sorted(nsr_build.VARIANTS)
    with ThreadPoolExecutor(min(len(names), os.cpu_count() or 1)) as ex:
        results = list(ex.map(nsr_build.check_variant, names))
    for name, bad in zip(names, results):
        assert not bad, (name, bad[:4])


def test_every_switch_in_the_sources_belongs_to_a_documented_variant():
    """A preprocessor switch in csrc/ that no VARIANTS entry defines is one nobody compiles: list it or delete it."""
    import re
    known = {d.split("=")[0][2:] for defs, _, _ in nsr_build.VARIANTS.values() for d in defs}
    tunables = {"NSR_MAX_SPLITS", "NSR_H1_WAVES", "NSR_HALO_SPREAD", "NSR_F16X3_KPF", "NSR_SLICE_INLINE"}  # #ifndef X / #define X default
    seen = set()
    for fn in os.listdir(nsr_build.CSRC):
        if fn.endswith((".hip", ".h")):
            for m in re.finditer(r"^\s*#\s*if(?:n?def)?\s+(?:!?defined\()?(NSR_\w+)", open(os.path.join(nsr_build.CSRC, fn)).read(), re.M):
                seen.add(m.group(1))
    stray = seen - known - tunables - {"NSR_TRAIN_H_"}
    assert not stray, f"undocumented switches: {sorted(stray)}"
