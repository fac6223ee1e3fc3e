"""Device-code identity of two source trees: ``python scripts/isa_diff.py OTHER_TREE [--variant NAME]... [--hooks]``.

Compiles every unit of ``build.UNITS`` (with ``--variant``: that ``build.VARIANTS`` entry's units with its defines; with
``--hooks``: tests/csrc/nsr_test_hooks*.hip too) in this tree and in OTHER_TREE (a ``git worktree`` / ``git archive`` of the
commit to compare against) with ``hipcc -S --cuda-device-only`` and the unit's own product flags, normalises the listings and
prints per unit ``identical`` or the first differing lines.  ``--json PATH`` writes the record (``--commit`` names OTHER_TREE
in it); ``--work DIR`` keeps the listings, and OTHER_TREE's are reused from there on the next run.  Exit status 1 on a difference.
"""
import argparse
import difflib
import glob
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_sr_amd import build as B  # noqa: E402

COMMON = [f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-S", "--cuda-device-only"]


def normalise(text):
    """The two differences that carry no information: the per-compile __hip_cuid_ symbol, and a printed zero offset on an
    inline-asm instruction (same encoding as no offset operand; compiler-written instructions never print one)."""
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    return re.sub(r";;#ASMSTART.*?;;#ASMEND", lambda m: re.sub(r" offset:0[ \t]*$", "", m.group(0), flags=re.M), text, flags=re.S)


def listing(tree, rel, flags, out, reuse):
    if not (reuse and os.path.exists(out)):
        csrc = os.path.join(tree, "nerf_sr_amd", "csrc")
        src = os.path.join(tree, rel)
        if not os.path.exists(src):
            return None
        subprocess.check_call([B._hipcc(), *COMMON, "-I" + csrc, *flags, src, "-o", out + ".tmp"], stderr=subprocess.DEVNULL)
        os.replace(out + ".tmp", out)
    with open(out) as f:
        return normalise(f.read())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("other")
    ap.add_argument("--variant", action="append", default=[], choices=sorted(B.VARIANTS))
    ap.add_argument("--hooks", action="store_true")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--work", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="nsr_isa_diff_")
    for side in ("other", "this"):
        os.makedirs(os.path.join(work, side), exist_ok=True)
    flags = dict(B.UNITS)
    jobs = [("product", os.path.join("nerf_sr_amd", "csrc", u), f) for u, f in B.UNITS]
    for v in a.variant:
        jobs += [(v, os.path.join("nerf_sr_amd", "csrc", u), flags[u] + B.VARIANTS[v][0]) for u in B.VARIANTS[v][1]]
    if a.hooks:
        jobs += [("product", os.path.relpath(s, ROOT), ["-ffp-contract=off"]) for s in sorted(glob.glob(os.path.join(ROOT, "tests", "csrc", "nsr_test_hooks*.hip")))]

    def one(job):
        name, rel, fl = job
        out = f"{name}__{os.path.basename(rel)}.s"
        old = listing(os.path.abspath(a.other), rel, fl, os.path.join(work, "other", out), True)
        new = listing(ROOT, rel, fl, os.path.join(work, "this", out), False)
        return old, new

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        results = list(ex.map(one, jobs))
    record, n_diff = [], 0
    for (name, rel, fl), (old, new) in zip(jobs, results):
        same = old is not None and old == new
        n_diff += not same
        print(f"{name:20s} {rel:50s} {'identical' if same else 'DIFFERENT'}")
        if not same:
            d = difflib.unified_diff((old or "").split("\n"), (new or "").split("\n"), "other", "this", n=1, lineterm="")
            print("\n".join(list(d)[:24]))
        record.append({"defines": name, "unit": rel.replace(os.sep, "/"), "flags": COMMON + fl, "identical": same,
                       "sha256_before": old and hashlib.sha256(old.encode()).hexdigest(),
                       "sha256_after": new and hashlib.sha256(new.encode()).hexdigest()})
    if a.json:
        hipcc = [ln for ln in subprocess.check_output([B._hipcc(), "--version"], text=True).split("\n") if "HIP version" in ln or "clang version" in ln]
        with open(a.json, "w") as f:
            json.dump({"parent": a.commit, "hipcc": hipcc, "normalisations": ["__hip_cuid_[0-9a-f]+ -> __hip_cuid_X", "trailing ' offset:0' removed inside ;;#ASMSTART ... ;;#ASMEND"],
                       "all_identical": n_diff == 0, "listings": record}, f, indent=1)
            f.write("\n")
    print(f"{len(jobs) - n_diff} of {len(jobs)} listings identical")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
