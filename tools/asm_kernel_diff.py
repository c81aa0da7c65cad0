#!/usr/bin/env python
"""Compare two device assembly files kernel by kernel: the instruction stream (comments, labels and directives stripped, labels in
operands renamed by order of first use) and .vgpr_count / .sgpr_count / .private_segment_fixed_size of the metadata.
  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -I include temporalstereo_amd/csrc/X.hip -o new.s   (and old.s)
  python tools/asm_kernel_diff.py old.s new.s"""
import re
import sys


def kernels(path):
    text = open(path).read()
    streams, cur = {}, None
    for line in text.split(".amdgpu_metadata")[0].splitlines():
        line = re.sub(r"\s*(;|//).*", "", line).strip()
        m = re.match(r"^(_Z\w+|\w+_kernel\w*):$", line)
        if m:
            cur, names = m.group(1), {}
            streams[cur] = []
        elif line.startswith(".end_amdhsa_kernel") or line.startswith(".section"):
            cur = None
        elif cur and line and not line.startswith(".") and not line.endswith(":"):
            streams[cur].append(re.sub(r"\.LBB\w+", lambda g: names.setdefault(g.group(0), "L%d" % len(names)), line))
    res = {}
    for blk in re.split(r"\n  - \.agpr_count", text.split(".amdgpu_metadata")[1])[1:]:
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        res[re.search(r"\.name:\s+(\S+)", blk).group(1)] = (get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"))
    return streams, res


(s0, r0), (s1, r1) = kernels(sys.argv[1]), kernels(sys.argv[2])
assert sorted(r0) == sorted(r1), "kernel symbols differ: %s" % sorted(set(r0) ^ set(r1))
print("%-10s %-22s %-22s %s" % ("stream", "old vgpr/sgpr/scratch", "new vgpr/sgpr/scratch", "kernel"))
for k in sorted(r0):
    same = s0[k] == s1[k]
    print("%-10s %-22s %-22s %s" % ("same" if same else "DIFFERS (%d -> %d)" % (len(s0[k]), len(s1[k])), "%d / %d / %d" % r0[k], "%d / %d / %d" % r1[k], k))
