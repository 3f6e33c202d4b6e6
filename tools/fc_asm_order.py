#!/usr/bin/env python3
"""Order of the vector-memory requests, workgroup barriers, vmcnt waits and branches of one
fc_decim_kernel<Z, DT, FLIP> instantiation, read from `hipcc -S` output: where each prefetch
group of fc_prefetch_plan.h landed between the barriers, whether pass C still loads the table,
and which waits lie on the carried path.  Consecutive equal events are counted.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I pypanadapter_amd/csrc -I include \\
        --cuda-device-only -S pypanadapter_amd/csrc/fc_kernels.hip -o fc.s
  tools/fc_asm_order.py fc.s 8 0 0        (Z, DT as InDtype numbers it, FLIP)"""
import re
import sys


def order(path, z, dt, flip):
    key = f"fc_decim_kernelILi{z}ELi{dt}ELi{flip}E"
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_Z\S*" + key + r"\S*:", l))
    out = []

    def push(tag, ln):  # a run of equal events no more than 40 lines apart is one entry
        if out and out[-1][0] == tag and ln - out[-1][3] <= 40:
            out[-1][1] += 1
            out[-1][3] = ln
        else:
            out.append([tag, 1, ln, ln])

    for i in range(start + 1, len(lines)):
        l = lines[i].strip()
        if l.startswith("s_endpgm"):
            break
        m = re.match(r"(\.LBB\S+):", l)
        if m:
            push("label " + m.group(1), i)
            continue
        op = l.split()[0] if l else ""
        if re.match(r"(buffer|global|scratch)_(load|store)", op):
            push(op + (" nt" if l.endswith(" nt") else ""), i)
        elif op == "s_barrier":
            push(op, i)
        elif op == "s_waitcnt" and "vmcnt" in l:
            push(l, i)
        elif op.startswith("s_cbranch") or op == "s_branch":
            push(l, i)
    return out


if __name__ == "__main__":
    for tag, n, ln, _ in order(sys.argv[1], *sys.argv[2:5]):
        print(f"{ln + 1:6d}  {tag}" + (f"  x{n}" if n > 1 else ""))
