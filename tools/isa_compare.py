"""Compare the kernels of two device-assembly files (hipcc -S --cuda-device-only, flags of csrc/Makefile), e.g. a translation unit before
and after a change:

    python tools/isa_compare.py before.s after.s [--rename 'REGEX=>REPLACEMENT' ...]

Bodies are compared with comments stripped, basic-block / temporary label numbers normalised and lines naming symbols dropped, so a
kernel that only moved in the file (or got a defaulted template parameter: map its old mangled name with --rename) compares equal.
Prints one line per file pair; exit status 1 when a kernel of the first file differs or is missing from the second."""
import argparse
import re
import sys


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r'^(_Z\S+):\s*(;.*)?$', line)
        if m and name is None:
            name, cur = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = cur
            name = None
            continue
        line = re.sub(r'\.LBB\d+_', '.LBB_', line)
        line = re.sub(r'\.Ltmp\d+', '.Ltmp', line)
        line = re.sub(r'\s*;.*$', '', line).rstrip()
        if line and '_Z' not in line:
            cur.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=>REPLACEMENT applied to the first file's kernel names")
    a = ap.parse_args()
    rules = [r.split("=>", 1) for r in a.rename]

    def rename(k):
        for pat, rep in rules:
            k = re.sub(pat, rep, k)
        return k
    b0, b1 = kernels(a.before), kernels(a.after)
    same = [k for k in b0 if b1.get(rename(k)) == b0[k]]
    diff = [k for k in b0 if rename(k) in b1 and b1[rename(k)] != b0[k]]
    gone = [k for k in b0 if rename(k) not in b1]
    print(f"{a.before}: {len(b0)} kernels, {len(same)} identical in {a.after}, differ: {diff}, missing: {gone}")
    sys.exit(1 if diff or gone else 0)


if __name__ == "__main__":
    main()
