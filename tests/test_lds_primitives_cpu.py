"""The inline-asm VMEM statements and the LDS address space have ONE home in the sources, csrc/nsr_lds_dma.h (DESIGN "One home
for the inline-asm VMEM rule"): the hazard rule build.isa_contract checks on the compiled listings is then changed in one place.
Text scans of csrc/ only; nothing is compiled."""
import os
import re

from nerf_sr_amd import build as nsr_build

HOME = "nsr_lds_dma.h"
ASM_VMEM = re.compile(r'"[^"\n]*global_(load_lds|store)')


def _sources():
    return {fn: open(os.path.join(nsr_build.CSRC, fn)).read() for fn in sorted(os.listdir(nsr_build.CSRC)) if fn.endswith((".hip", ".h"))}


def scan(sources):
    """Violations of the one-home rule in {file name: text}."""
    bad = []
    for fn, text in sources.items():
        if fn != HOME:
            bad += [f"{fn}: asm VMEM string {m.group(0)!r}" for m in ASM_VMEM.finditer(text)]
            bad += [f"{fn}: address_space(3)"] * text.count("address_space(3)")
        bad += [f"{fn}: declares {m.group(1)}" for m in re.finditer(r"\btypedef\b[^;]*\b(lds_ptr_t|glb_ptr_t)\s*;", text)]
    return bad


def test_asm_vmem_and_lds_address_space_only_in_the_primitives_header():
    src = _sources()
    assert HOME in src and ASM_VMEM.search(src[HOME]) and "address_space(3)" in src[HOME]
    assert "nsr_mlp_stream.h" not in src
    assert not scan(src), scan(src)


def test_the_scan_catches_violations():
    """The scan itself: a second asm string, a second address-space cast and the unused pointer typedefs are all reported."""
    fake = {HOME: 'asm volatile("global_load_lds_dwordx4 %1, %0 offset:%4");\n(const __attribute__((address_space(3))) char*)p;\n',
            "nsr_other.hip": 'asm volatile("s_mov_b64 %0, %2\\n\\t"\n "global_load_lds_dwordx4 %1, %0" : "=&s"(tmp));\n'
                             'asm volatile("global_store_dword %1, %2, %0");\n'
                             "return *(const __attribute__((address_space(3))) unsigned*)(size_t)a;\n"
                             "typedef __attribute__((address_space(3))) void* lds_ptr_t;\n// global_load_lds in a comment is fine\n"}
    bad = scan(fake)
    assert len(bad) == 5 and all(b.startswith("nsr_other.hip") for b in bad), bad
    assert sum("asm VMEM" in b for b in bad) == 2 and sum("address_space" in b for b in bad) == 2 and sum("lds_ptr_t" in b for b in bad) == 1


def test_isa_units_are_the_units_that_reach_the_header():
    def reaches(fn, seen):
        if fn == HOME:
            return True
        path = os.path.join(nsr_build.CSRC, fn)
        if fn in seen or not os.path.exists(path):
            return False
        seen.add(fn)
        incs = re.findall(r'^\s*#\s*include\s+"([^"/]+)"', open(path).read(), re.M)       # csrc/ headers: no directory part
        return any(reaches(i, seen) for i in incs)

    want = {u for u, _ in nsr_build.UNITS if reaches(u, set())}
    assert set(nsr_build.ISA_UNITS) == want and len(nsr_build.ISA_UNITS) == len(want)
    assert {"nsr_mlp_f16.hip", "nsr_train_chain.hip", "nsr_gemm_f16.hip", "nsr_wgrad_f16.hip", "nsr_mlp.hip", "nsr_mlp_h1.hip",
            "nsr_mlp_arch_f16.hip", "nsr_refine_wgrad_f16.hip"} == want
