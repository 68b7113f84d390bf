#!/usr/bin/env python3
"""One hash per kernel of a libhip_ad_rgb.so over its gfx950 disassembly (instructions only: no addresses, no encodings, no symbol names), to show that a
change left every other kernel's code object alone.  No GPU needed.
Usage: python tools/kernel_hashes.py <a.so> [<b.so>]      one library: the table; two: the kernels whose code differs or that exist in one only"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def hashes(so):
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin"); co = os.path.join(d, "gfx950.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so])
        targets = subprocess.check_output([os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o", "--input=" + fat]).decode().split()
        tgt = next(t for t in targets if "gfx950" in t)
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + tgt, "--input=" + fat, "--output=" + co])
        dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co]).decode()
    out = {}; name = None; h = None; n = 0
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line.strip())
        if m:
            if name:
                out[name] = (h.hexdigest()[:16], n)
            name = m.group(1); h = hashlib.sha256(); n = 0
            continue
        s = line.strip()
        if name and s and not s.startswith("<"):
            s = re.sub(r"\s*//.*$", "", s)                    # the trailing address / encoding comment
            h.update(s.encode() + b"\n"); n += 1
    if name:
        out[name] = (h.hexdigest()[:16], n)
    demangled = subprocess.check_output(["c++filt"], input="\n".join(out).encode()).decode().splitlines()
    return {re.sub(r"\(.*$", "", dn).replace("void ", ""): v for dn, v in zip(demangled, out.values())}


def main():
    a = hashes(sys.argv[1])
    if len(sys.argv) < 3:
        for k in sorted(a):
            print("%-100s %s %7d" % (k, a[k][0], a[k][1]))
        return
    b = hashes(sys.argv[2])
    same = [k for k in a if k in b and a[k] == b[k]]
    print("%d kernels / device functions of %s, %d of %s; identical instruction streams: %d" % (len(a), sys.argv[1], len(b), sys.argv[2], len(same)))
    only_a = {k: v for k, v in a.items() if k not in b}; only_b = {k: v for k, v in b.items() if k not in a}
    for k in sorted(only_a):                                   # a kernel that gained a template argument keeps its code under a longer name
        twin = [kb for kb in sorted(only_b) if only_b[kb] == only_a[k] and kb.startswith(k.rstrip(">"))]
        if twin:
            print("same code, renamed: %-80s -> %s  %s %7d instructions" % (k, twin[0], a[k][0], a[k][1])); del only_b[twin[0]]
        else:
            print("only in the first:  %-80s %s %7d instructions" % (k, a[k][0], a[k][1]))
    for k in sorted(only_b):
        print("only in the second: %-80s %s %7d instructions" % (k, b[k][0], b[k][1]))
    for k in sorted(set(a) & set(b)):
        if a[k] != b[k]:
            print("differs:            %-80s %s %7d -> %s %7d" % (k, a[k][0], a[k][1], b[k][0], b[k][1]))

if __name__ == "__main__":
    main()
