#!/usr/bin/env python3
"""Per-kernel device-code diff of one csrc/ source between two trees, for refactors that must
not change what runs:  python scripts/isa_diff.py csrc/conv_wino4.hip OLD NEW [-DFLAG ...]

OLD / NEW: a tree's root directory, or a git revision of this repository (exported to a
temporary directory).  Each side is compiled with az_build.FLAGS (minus -shared) plus
--cuda-device-only -S and the extra flags.  Per kernel symbol, without comments and the
__hip_cuid_* symbol: instruction count, sha256 of the code, sha256 of the kernel descriptor
(.amdhsa_*) + metadata entry, and whether the sides agree.  Exit status 1 on any difference.
A differ, not a scanner: it knows no instruction."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "alphazero-othello_amd"
sys.path.insert(0, os.path.join(ROOT, PKG))
import az_build  # noqa: E402


def tree_of(arg, tmp):
    """A directory as it is; anything else as a git revision exported under tmp."""
    if os.path.isdir(arg):
        return os.path.abspath(arg)
    out = os.path.join(tmp, re.sub(r"\W", "_", arg))
    os.makedirs(out)
    tar = subprocess.run(["git", "-C", ROOT, "archive", arg], check=True, capture_output=True)
    subprocess.run(["tar", "-x", "-C", out], input=tar.stdout, check=True)
    return out


def assembly(tree, src, extra, out):
    flags = [f for f in az_build.FLAGS if f != "-shared"] + ["--cuda-device-only", "-S"] + extra
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + flags + [src, "-o", out], cwd=os.path.join(tree, PKG), check=True)
    with open(out) as fh:
        return fh.read()


def kernels(text):
    """{kernel symbol: (instruction count, code sha256, descriptor + metadata sha256)}"""
    lines = [ln.split(";")[0].rstrip() for ln in text.splitlines()]
    lines = [ln for ln in lines if ln.strip() and "__hip_cuid_" not in ln]
    digest = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()[:16]  # noqa: E731
    # the metadata note: one "  - .agpr_count ..." entry per kernel, named by its .symbol
    meta = {}
    for blk in re.split(r"\n(?=  - \.)", "\n".join(lines).split("amdhsa.kernels:")[-1]):
        m = re.search(r"^\s+\.symbol:\s+(\S+)\.kd", blk, re.M)
        if m:
            meta[m.group(1)] = blk.splitlines()
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
        if m:
            name, end = m.group(1), lines.index("\t.end_amdhsa_kernel", i)
            body = lines[lines.index(name + ":") + 1:i]  # the label up to its descriptor
            code = [b for b in body if b.startswith("\t") and not b.startswith("\t.")]
            out[name] = (len(code), digest(body), digest(lines[i:end + 1] + meta.get(name, [])))
    return out


def main():
    src, old, new, extra = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:]
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(tree_of(t, tmp), os.path.join(tmp, f"side{i}.s")) for i, t in enumerate((old, new))]
        with ThreadPoolExecutor(2) as ex:
            a, b = ex.map(lambda j: kernels(assembly(j[0], src, extra, j[1])), jobs)
    print(f"# {src}: {old} vs {new}; flags {' '.join(extra) or '(default)'}")
    print("# kernel | instructions | code sha256 | descriptor+metadata sha256 | verdict")
    bad = 0
    for name in sorted(set(a) | set(b)):
        same = a.get(name) == b.get(name)
        bad += not same
        for side in ([a[name]] if same else [a.get(name), b.get(name)]):
            print(name, *(side or ("missing",)), "equal" if same else "DIFFERENT")
    print(f"# {len(a)} / {len(b)} kernels, {bad} different")
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(main())
