#!/usr/bin/env python3
"""Instruction mix of one welch_dif_kernel instantiation's segment loop, from a gfx950 assembly
listing of zfft_kernels.hip (hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S).

The segment loop is the kernel's only loop; with the two prefetch arrays (ZFFT_DIF_PP) it holds
two segment bodies, otherwise one.  Printed: per segment body the VALU instructions by class,
vector-memory loads, LDS operations by opcode, waits and barriers; then the order of the
vector-memory requests, the vmcnt waits and the barriers in the first body, with the number of
VALU instructions since the body's start (where the prefetch is requested, where it is waited for).

usage: tools/welch_asm_mix.py FILE.s [N PRUNE HALF SEG LINES]   (default 4096 1 1 0 0: cfg2)
"""
import re
import sys
from collections import Counter


def kernel_lines(path, N, P, H, S, L):
    tag = f"_ZN4zfft16welch_dif_kernelILi{N}ELb{P}ELb{H}ELb{S}ELb{L}E"
    out, on = [], False
    for line in open(path):
        if not on and line.startswith(tag) and ":" in line:
            on = True
        if on:
            out.append(line.rstrip("\n"))
            if line.strip().startswith("s_endpgm"):
                break
    assert out, f"{tag} not in {path}"
    return out


def valu_class(op, line):
    if op.startswith(("v_pk_fma", "v_pk_mul", "v_pk_add")):
        return "packed f32"
    if "_dpp" in op or "row_" in line or "quad_perm" in line:
        return "dpp"
    if op.startswith("v_permlane"):
        return "permlane"
    if re.match(r"v_(fma|fmac|mul|add|sub|subrev|mac)_f32", op):
        return "scalar f32"
    if op.startswith("v_mov") or op.startswith("v_accvgpr"):
        return "mov"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "readlane"
    if op.startswith(("v_cmp", "v_cndmask")):
        return "cmp/select"
    return "int/addr"


def main():
    path = sys.argv[1]
    args = sys.argv[2:7] if len(sys.argv) >= 7 else ["4096", "1", "1", "0", "0"]
    lines = kernel_lines(path, *args)
    hdr = next(i for i, l in enumerate(lines) if "Loop Header: Depth=1" in l)
    label = lines[hdr].split(":")[0]
    backs = [i for i, l in enumerate(lines) if re.search(r"s_c?branch\w*\s+" + re.escape(label) + r"\b", l) and i > hdr]
    if backs:
        back = max(backs)
    else:  # the latch is placed elsewhere: take the loop's last block by the compiler's comments
        last = max(i for i, l in enumerate(lines) if f"Header={label[2:]} " in l)
        back = next((i - 1 for i in range(last + 1, len(lines)) if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", lines[i])),
                    len(lines) - 1)
    body = lines[hdr:back + 1]
    ops = [(l.split()[0], l) for l in (b.strip() for b in body) if l and not l.startswith((";", "."))]
    # two segment bodies with the two prefetch arrays (ZFFT_DIF_PP, every N but 16384), else one
    nbar = sum(1 for op, _ in ops if op == "s_barrier")
    bodies = 1 if args[0] == "16384" else 2
    valu, lds, other = Counter(), Counter(), Counter()
    for op, l in ops:
        if op.startswith("v_"):
            valu[valu_class(op, l)] += 1
        elif op.startswith("ds_"):
            lds[op] += 1
        elif op.startswith(("buffer_load", "global_load", "flat_load")):
            other["vector-memory loads"] += 1
        elif op.startswith(("buffer_store", "global_store", "scratch_")):
            other[op] += 1
        elif op == "s_waitcnt" and "vmcnt" in l:
            other["s_waitcnt vmcnt"] += 1
        elif op in ("s_barrier", "s_nop"):
            other[op] += 1
    print(f"welch_dif_kernel<{', '.join(args)}>: loop of {len(ops)} instructions, {bodies} segment bodies")
    print(f"per segment body: VALU {sum(valu.values()) / bodies:g}")
    for k, v in sorted(valu.items(), key=lambda kv: -kv[1]):
        print(f"  {k:12s} {v / bodies:g}")
    print("LDS: " + ", ".join(f"{k} {v / bodies:g}" for k, v in sorted(lds.items())))
    print("other: " + ", ".join(f"{k} {v / bodies:g}" for k, v in sorted(other.items())))
    print("order in the first body (VALU instructions since the loop head):")
    nv, run, last = 0, 0, None
    if bodies == 1:
        first = ops
    elif nbar < bodies:  # a frame is one wave (no s_barrier): the loop's first half
        first = ops[:len(ops) // 2]
    else:
        first = ops[:next(i for i, (op, _) in enumerate(ops) if op == "s_barrier" and
                          sum(1 for o, _ in ops[:i + 1] if o == "s_barrier") == nbar // bodies) + 1]

    def flush():
        nonlocal run, last
        if run:
            print(f"  {last[0]:5d}  {last[1]} x{run}")
        run, last = 0, None
    for op, l in first:
        if op.startswith("v_"):
            nv += 1
        ev = None
        if op.startswith(("buffer_load", "global_load")):
            ev = op
        elif op == "s_waitcnt" and "vmcnt" in l:
            ev = "s_waitcnt " + re.search(r"vmcnt\(\d+\)", l).group(0)
        elif op == "s_barrier" or op.startswith(("ds_bpermute", "v_permlane")):
            ev = op
        if ev is None:
            continue
        if last and last[1] == ev and ev.startswith(("buffer_load", "global_load", "ds_bpermute", "v_permlane")):
            run += 1
        else:
            flush()
            last, run = (nv, ev), 1
    flush()


if __name__ == "__main__":
    main()
