#!/usr/bin/env python
"""Which kernel instantiations does the device code hold, and which of them ran?  (CPU only; reads symbol tables, nothing else.)

    python tools/kernel_census.py                                  # every csrc/*.hip
    python tools/kernel_census.py rgcn_kernels rgcn_bwd rgcn_gemm  # some of them
    python tools/kernel_census.py rgcn_bwd --trace kernel_trace.csv

A kernel is a symbol of the gfx950 code object that has a kernel descriptor (`<name>.kd`).  The code object of a translation unit comes
from its host object under csrc/build/ when that is newer than the source (the `.hip_fatbin` section, unbundled), else from a device-only
compile with the Makefile's flags.  Output: one demangled name per line, without the anonymous-namespace prefix and without the parameter
list -- `wgrad_tiled_d16_kernel<8, 2>`.  With --trace FILE (the kernel-trace CSV of `rocprofv3 --kernel-trace`, or its --stats summary):
every census name of the chosen files followed by `ran` or `not seen`; exit status 1 when a name is `not seen` that --expect-missing
FILE (one name per line) does not list."""
import argparse
import csv
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-rgcn_amd", "csrc")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


class ToolMissing(RuntimeError):
    pass


def _tool(*names):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for n in names:
        for d in (None, os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "bin")):
            p = shutil.which(n) if d is None else (os.path.join(d, n) if os.access(os.path.join(d, n), os.X_OK) else None)
            if p:
                return p
    raise ToolMissing(f"none of {names} found")


def sources():
    """stems of csrc/*.hip plus the second compile of rgcn_fbasis_tile.hip (the Makefile's SRC, without the host file)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=\s*(.*)$", text, re.M).group(1).split()
    return [os.path.splitext(s)[0] for s in src if s.endswith(".hip")]


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    return flags + re.search(r"^INC\s*:=\s*(.*)$", text, re.M).group(1).split()


def _source_of(stem):
    p = os.path.join(CSRC, stem + ".hip")
    if not os.path.exists(p):
        raise FileNotFoundError(p)
    return p, []


def code_object(stem, tmp):
    """-> path of the gfx950 code object of csrc/<stem>.hip"""
    src, extra = _source_of(stem)
    obj = os.path.join(CSRC, "build", stem + ".o")
    deps = [src] + [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")]
    co = os.path.join(tmp, stem + ".co")
    bundler = _tool("clang-offload-bundler")
    if os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(d) for d in deps):
        fb = os.path.join(tmp, stem + ".fatbin")
        subprocess.check_call([_tool("llvm-objcopy", "objcopy"), f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(tmp, stem + ".copy.o")])
        subprocess.check_call([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fb}", f"--output={co}"])
        return co
    dev = os.path.join(tmp, stem + ".dev.o")
    hipcc = os.environ.get("HIPCC") or _tool("hipcc")
    subprocess.check_call([hipcc] + _makefile_flags() + extra + ["--cuda-device-only", "-c", "-o", dev, src], cwd=CSRC, stderr=subprocess.DEVNULL)
    head = open(dev, "rb").read(24)
    if head.startswith(b"__CLANG_OFFLOAD_BUNDLE__"):
        subprocess.check_call([bundler, "--unbundle", "--type=o", f"--targets={TARGET.replace('hipv4', 'hip')}", f"--input={dev}", f"--output={co}"])
        return co
    return dev


def short_name(demangled):
    """`void (anonymous namespace)::k<4, true>(float const*, int) [clone .kd]` -> `k<4, true>`"""
    s = re.sub(r"\s*\[clone [^\]]*\]", "", demangled.strip())
    s = re.sub(r"\.kd$", "", s)
    s = s.replace("(anonymous namespace)::", "")
    depth, cut = 0, len(s)
    for i, c in enumerate(s):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            cut = i
            break
    s = s[:cut].strip()
    return s[5:] if s.startswith("void ") else s


def census(stem, tmp=None):
    """-> sorted kernel names of csrc/<stem>.hip"""
    with tempfile.TemporaryDirectory() as own:
        co = code_object(stem, tmp or own)
        out = subprocess.check_output([_tool("nm", "llvm-nm"), "--defined-only", co], text=True)
        kd = [ln.split()[-1][:-3] for ln in out.splitlines() if ln.split() and ln.split()[-1].endswith(".kd")]
        dem = subprocess.run([_tool("c++filt", "llvm-cxxfilt")], input="\n".join(kd), capture_output=True, text=True, check=True).stdout
    return sorted({short_name(ln) for ln in dem.splitlines() if ln.strip()})


def trace_names(path):
    """kernel names of a rocprofv3 kernel-trace CSV (column Kernel_Name) or of its stats summary (column Name), shortened as the census"""
    seen = set()
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        col = next((c for c in ("Kernel_Name", "Name", "KernelName") if c in (rd.fieldnames or [])), None)
        if col is None:
            raise SystemExit(f"{path}: no kernel-name column in {rd.fieldnames}")
        for row in rd:
            seen.add(short_name(row[col]))
    return seen


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="*", help="stems or names of csrc/*.hip (default: all)")
    ap.add_argument("--trace", action="append", default=[], help="kernel-trace CSV; may be given more than once")
    ap.add_argument("--expect-missing", help="file of names that may read `not seen`")
    a = ap.parse_args(argv)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in a.files] or sources()
    ran = set()
    for t in a.trace:
        ran |= trace_names(t)
    allowed = set()
    if a.expect_missing:
        allowed = {ln.strip() for ln in open(a.expect_missing) if ln.strip() and not ln.startswith("#")}
    bad = 0
    for stem in stems:
        names = census(stem)
        if a.trace:
            print(f"# {stem}.hip: {len(names)} kernels, {sum(n in ran for n in names)} ran")
        for n in names:
            if not a.trace:
                print(n)
                continue
            ok = n in ran
            print(f"{n}\t{'ran' if ok else 'not seen'}")
            bad += (not ok) and n not in allowed
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
