#!/usr/bin/env python3
"""Compare the register / scratch / LDS / occupancy figures of every kernel of two source trees.

    tools/resource_usage_diff.py --dump <tree> > a.json        compile the tree's kernel sources (device only) with
                                                               -Rpass-analysis=kernel-resource-usage and print {kernel: figures}
    tools/resource_usage_diff.py a.json b.json                 kernels in both: every figure must be equal (exit 1 otherwise);
                                                               kernels only in b are listed with their figures

A kernel is named by its demangled signature.  Kernels that became templates keep their place in the comparison: the
template arguments `<false>` of k_api_bsdf_eval_pdf / k_api_bsdf_sample and the trailing `, false` of k_aov_fill are the
instantiations that other scenes launch, and are compared with the parent's plain kernels.
"""
import json
import os
import re
import subprocess
import sys

SOURCES = ("har_kernels.hip", "har_aov.hip", "har_refit.hip")
FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -munsafe-fp-atomics -fPIC -Wno-unused-function".split()
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def dump(tree):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(tree, "mitsuba3_amd", "csrc")
    procs = [(f, subprocess.Popen([hipcc] + FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, f],
                                  cwd=src, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True)) for f in SOURCES]
    out = {}
    for f, p in procs:
        err = p.communicate()[1]
        if p.returncode:
            sys.exit("%s: hipcc failed\n%s" % (f, err[-2000:]))
        name = None
        for line in err.splitlines():
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                name = m.group(1); out[name] = {}
                continue
            m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
            if m and name and m.group(1).strip() in FIELDS:
                out[name][m.group(1).strip()] = m.group(2)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d: out[n] for n, d in zip(names, dem)}


def canonical(name):
    """the name a kernel had before it became a template (see the module text)"""
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"k_api_bsdf_(eval_pdf|sample)<false>", r"k_api_bsdf_\1", name)
    name = re.sub(r"k_aov_fill<(true|false), false>", r"k_aov_fill<\1>", name)
    return name


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        json.dump(dump(sys.argv[2]), sys.stdout, indent=1, sort_keys=True)
        return 0
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a = {canonical(k): v for k, v in json.load(open(sys.argv[1])).items()}
    b = {canonical(k): v for k, v in json.load(open(sys.argv[2])).items()}
    bad = 0
    for k in sorted(a):
        if k not in b:
            print("GONE   ", k[:160]); bad += 1
        elif a[k] != b[k]:
            print("DIFFERS", k[:160])
            for f in FIELDS:
                if a[k].get(f) != b[k].get(f):
                    print("          %s: %s -> %s" % (f, a[k].get(f), b[k].get(f)))
            bad += 1
    new = sorted(k for k in b if k not in a)
    print("%d kernels in both, %d differ or are gone, %d new" % (len(set(a) & set(b)), bad, len(new)))
    for k in new:
        v = b[k]
        print("NEW     VGPRs %s AGPRs %s SGPRs %s scratch %s B/lane LDS %s B occupancy %s  %s" % (
            v.get("VGPRs"), v.get("AGPRs"), v.get("TotalSGPRs"), v.get("ScratchSize [bytes/lane]"), v.get("LDS Size [bytes/block]"), v.get("Occupancy [waves/SIMD]"), k[:150]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
