#!/usr/bin/env python3
"""Instructions k_pack issues per 16-base span on upper-case ACGT data, counted in its gfx950 assembly (no GPU needed):

    hipcc --offload-arch=gfx950 --cuda-device-only -O3 -std=c++17 -S -Iinclude -Iquicked_amd/csrc t.hip -o t.s
    python tools/pack_span_count.py t.s          (t.hip: the four lines tools/kernel_resources.sh compiles)

The walk starts at every inner-loop header of the kernel that is followed by 16-byte loads and follows the path such data
takes until the loop's back edge: a uniform branch on `vccz` (no lane has a candidate for a flag) is taken, a branch around a
block that is skipped when no lane is active (`execz`) is taken unless the block loads 16 bytes or stores -- the flag code
is skipped, the guarded load and the store are not -- and every other conditional branch falls through.  Printed per loop:
the loads of 16 bytes on the path (= the spans of one trip) and the VALU, scalar and memory instructions per span."""
import re
import sys


def kernel_lines(path, name="_ZN2qe6k_packENS_8PackArgsE"):
    out, on = [], False
    for line in open(path):
        if line.startswith(name + ":"):
            on = True
        if on:
            out.append(line.rstrip("\n"))
            if ".amdhsa_kernel" in line:
                break
    return out


def walk(lines, head):
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    m = re.match(r"(\.LBB\d+_\d+):", lines[head]) or re.match(r"(\.LBB\d+_\d+):", lines[head - 1])      # (a nested loop's header comment takes two lines)
    name = m.group(1)
    i, count, steps = head + 1, {"valu": 0, "salu": 0, "load16": 0, "store": 0, "dot4": 0, "lds": 0}, 0
    while i < len(lines) and steps < 100000:
        steps += 1
        if i == head or i == head - 1 and steps > 1:
            return count                                          # back at the header by falling through
        t = lines[i].strip()
        op = t.split()[0] if t and not t.startswith((";", ".")) else ""
        if op.startswith("v_"):
            count["valu"] += 1
            count["dot4"] += op.startswith("v_dot4")
        elif op.startswith("ds_"):
            count["lds"] += 1
        elif op == "global_load_dwordx4":
            count["load16"] += 1
        elif op.startswith("global_store") or op.startswith("global_atomic"):
            count["store"] += 1
        elif op.startswith("s_"):
            count["salu"] += 1
            m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
            if m:
                to = m.group(1)
                if to == name:
                    return count                                  # the back edge
                if op == "s_branch":
                    i = labels[to]; continue
                if op == "s_cbranch_vccz":
                    i = labels[to]; continue
                block = "\n".join(lines[i + 1:labels[to]]) if labels[to] > i else ""
                if op == "s_cbranch_execz" and block and "global_load_dwordx4" not in block and "global_store" not in block:
                    i = labels[to]; continue
                if op == "s_cbranch_vccnz" and "global_load_dwordx4" in block and "v_perm_b32" in block:
                    i = labels[to]; continue                      # around the load of the reversed string
        i += 1
    return None


def main():
    lines = kernel_lines(sys.argv[1])
    total = {"valu": sum(1 for l in lines if l.strip().startswith("v_")), "salu": sum(1 for l in lines if l.strip().startswith("s_"))}
    print(f"k_pack: {total['valu']} VALU and {total['salu']} scalar instructions in all")
    for i, l in enumerate(lines):
        if "Loop Header" in l:
            c = walk(lines, i)
            if c and c["load16"]:
                n = c["load16"]
                print(f"loop at line {i + 1}: {n} spans per trip; per span {c['valu'] / n:.1f} VALU ({c['dot4'] / n:.0f} v_dot4), "
                      f"{c['salu'] / n:.1f} scalar, {c['lds'] / n:.1f} LDS-crossbar, {c['store'] / n:.1f} stores")


if __name__ == "__main__":
    main()
