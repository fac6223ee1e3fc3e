"""The library-internal functions (NSR_INTERNAL: hidden visibility, called across translation units) are declared ONCE, in a
header that the defining unit includes as well (DESIGN "One home for the inference units' internal interface").  Most of them
have C linkage, where the signature is not part of the symbol: a hand-copied prototype that has drifted from the definition
links cleanly and passes garbage to a kernel launch.  With one declaration that the definition sees, the drift is a compile
error.  Text scans of csrc/ and tests/csrc/ only; nothing is compiled."""
import glob
import os
import re

from nerf_sr_amd import build as nsr_build

HOOKS = os.path.join(os.path.dirname(nsr_build.HERE), "tests", "csrc")
PROTO = re.compile(r"\bNSR_INTERNAL\b[^;{}()]*?(\w+)\s*\(")


def _strip_comments(text):
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def internals(text):
    """[(function name, 'decl' | 'def')] of the NSR_INTERNAL prototypes of one file, in order."""
    text = re.sub(r"^\s*#\s*define\s+NSR_INTERNAL\b[^\n]*", "", _strip_comments(text), flags=re.M)
    found = []
    for m in PROTO.finditer(text):
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        tail = text[i:].lstrip()
        found.append((m.group(1), "decl" if tail.startswith(";") else "def"))
    return found


def scan(sources, closure):
    """Violations in {file name: text}; closure(file name) = names of the files it reaches through #include "..." lines."""
    bad = []
    declared = {}
    for fn, text in sources.items():
        for name, kind in internals(text):
            if kind == "decl" and fn.endswith(".hip"):
                bad.append(f"{fn}: declares {name} (prototypes belong in a header)")
            elif kind == "decl":
                declared.setdefault(name, []).append(fn)
    for fn, text in sources.items():
        if not fn.endswith(".hip"):
            continue
        for name, kind in internals(text):
            if kind != "def":
                continue
            homes = declared.get(name, [])
            if len(homes) != 1:
                bad.append(f"{fn}: defines {name}, declared in {len(homes)} headers {homes}")
            elif homes[0] not in closure(fn):
                bad.append(f"{fn}: defines {name} without including its declaration ({homes[0]})")
    return bad


def _sources():
    paths = sorted(glob.glob(os.path.join(nsr_build.CSRC, "*.hip")) + glob.glob(os.path.join(nsr_build.CSRC, "*.h")) +
                   glob.glob(os.path.join(HOOKS, "*.hip")))
    return {os.path.basename(p): open(p).read() for p in paths}, {os.path.basename(p): p for p in paths}


def _closure(path):
    return {os.path.basename(p) for p in nsr_build.include_closure(path)}


def test_internal_functions_are_declared_once_and_seen_by_their_definitions():
    src, paths = _sources()
    names = {n for text in src.values() for n, _ in internals(text)}
    assert {"nsr_f16x3_render_composite", "nsr_h1_pack", "nsr_fp32_render_composite", "nsr_check_weights_range2", "nsr_payload_bytes",
            "nsr_chain_bwd", "gemm_f16x3"} <= names
    bad = scan(src, lambda fn: _closure(paths[fn]))
    assert not bad, bad


def test_the_inference_units_share_one_header():
    src, paths = _sources()
    home = "nsr_mlp_units.h"
    for unit in ("nsr_mlp.hip", "nsr_mlp_f16.hip", "nsr_mlp_h1.hip", "nsr_api.hip", "nsr_train.hip"):
        assert home in _closure(paths[unit]), unit
    assert all(kind == "decl" for _, kind in internals(src[home]))
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src[home], re.M) == ["nsr_common.h", "nsr_composite.h"]
    # the host-only units stay out of the ISA contract's unit list (build.ISA_UNITS)
    assert nsr_build.ISA_HEADER not in _closure(paths[home]) and nsr_build.ISA_HEADER not in _closure(paths["nsr_api.hip"])
    assert "nsr_api.hip" not in nsr_build.ISA_UNITS


def test_the_scan_catches_violations():
    """The scan itself: a prototype in a unit, a second declaration, a missing one, and a definition that does not see its
    declaration are all reported; comments, the macro's own definition and a correct pair are not."""
    fake = {
        "nsr_common.h": '#define NSR_INTERNAL __attribute__((visibility("hidden")))\n',
        "a.h": '#include "nsr_common.h"\n// NSR_INTERNAL int in_a_comment(int);\n'
               'extern "C" NSR_INTERNAL int good(const float* const* w,\n    void* stream);\n'
               "NSR_INTERNAL int twice(int a = f(1));\nNSR_INTERNAL int unseen(void);\n",
        "b.h": "NSR_INTERNAL int twice(int a);\n",
        "good.hip": '#include "a.h"\nextern "C" NSR_INTERNAL int good(const float* const* w, void* stream) {\n  return 0;\n}\n'
                    "/* NSR_INTERNAL int also_a_comment(int); */\n",
        "bad.hip": '#include "b.h"\nextern "C" NSR_INTERNAL size_t copied(void);\n'
                   "NSR_INTERNAL int twice(int a) { return a; }\nNSR_INTERNAL int nowhere(int (*f)(int)) { return f(0); }\n"
                   "NSR_INTERNAL int unseen(void) { return 1; }\n",
    }
    reach = {"good.hip": {"good.hip", "a.h", "nsr_common.h"}, "bad.hip": {"bad.hip", "b.h"}}
    assert internals(fake["a.h"]) == [("good", "decl"), ("twice", "decl"), ("unseen", "decl")]
    assert internals(fake["bad.hip"]) == [("copied", "decl"), ("twice", "def"), ("nowhere", "def"), ("unseen", "def")]
    bad = scan(fake, lambda fn: reach[fn])
    assert len(bad) == 4 and all(b.startswith("bad.hip") for b in bad), bad
    assert sum("declares copied" in b for b in bad) == 1 and sum("twice, declared in 2" in b for b in bad) == 1
    assert sum("nowhere, declared in 0" in b for b in bad) == 1 and sum("unseen without including" in b for b in bad) == 1
