#!/usr/bin/env python3
"""Instruction counts of the scans (irbx.hip: expand_pool_kernel, expand_stats_kernel) in a listing made with
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S irbx.hip -o irbx.s
Per kernel: the static counts of the whole kernel, and the dynamic counts of one pass through the innermost loop (one 32-pixel
block times the wave's NBW channel blocks) on the path an interior block takes: every `s_cbranch_vccnz` inside the loop is the
skip of a group's border work and is followed.  `after MFMA` lists, per channel block, the VALU instructions between its last MFMA
and the first such branch.  A kernel without those branches (the parent's, expand_stats) is simply walked to the loop's back edge.
usage: isa_scan_counts.py irbx.s"""
import re
import sys


def readable(m):
    return f"{m.group(1)}<{'_Float16' if m.group(2) == 'DF16_' else '__bf16'}, {m.group(3)}, {m.group(4)}>"


def main():
    lines = open(sys.argv[1]).read().split("\n")
    pat = re.compile(r"^_ZN4llie\d+(expand_(?:pool|stats)_kernel)I(DF16_|DF16b)Li(\d)ELi(\d)EE\w*:")
    for si, l0 in enumerate(lines):
        m = pat.match(l0)
        if not m:
            continue
        end = next(i for i in range(si, len(lines)) if lines[i].strip() == "s_endpgm")
        ops = [l.split()[0] for l in (x.strip() for x in lines[si + 1:end]) if l and not l.startswith((";", ".")) and not l.endswith(":")]
        valu = [o for o in ops if o.startswith("v_") and not o.startswith("v_mfma")]
        static = (f"static: VALU {len(valu):4d}  v_cndmask {sum(o.startswith('v_cndmask') for o in valu):3d}  "
                  f"v_dot2 {sum(o.startswith('v_dot2') for o in valu):3d}  v_mov {sum(o.startswith('v_mov') for o in valu):3d}  "
                  f"branches {sum(o.startswith('s_cbranch') for o in ops):2d}")
        labels = {mm.group(1): i for i in range(si, end) for mm in [re.match(r"^(\.LBB\d+_\d+):", lines[i])] if mm}
        first_mfma = next(i for i in range(si, end) if "v_mfma" in lines[i])
        pc = max(i for i in labels.values() if i < first_mfma)  # header of the innermost loop
        n_valu = n_mfma = n_salu = skipped = 0
        seg, segs, nops = None, [], []
        for _ in range(5000):
            l = lines[pc].strip()
            pc += 1
            if not l or l.startswith((";", ".")):
                continue
            op = l.split()[0]
            if op.startswith("v_mfma"):
                n_mfma += 1
                seg = 0
            elif op.startswith("v_"):
                n_valu += 1
                if seg is not None:
                    seg += 1
            elif op == "s_nop":
                nops.append(int(l.split()[1]))
            elif op == "s_cbranch_vccnz":
                skipped += 1
                if seg is not None:
                    segs.append(seg)
                    seg = None
                pc = labels[l.split()[1]]
            elif op == "s_branch":
                pc = labels[l.split()[1]]
            elif op in ("s_cbranch_scc0", "s_cbranch_scc1"):
                break  # the loop's back edge
            elif op.startswith("s_") and op != "s_waitcnt":
                n_salu += 1
        print(f"{readable(m):38s} {static} | interior block: VALU {n_valu:3d}  MFMA {n_mfma:2d}  SALU {n_salu:2d}  "
              f"border branches skipped {skipped}  after MFMA {segs}  s_nop {nops}")


if __name__ == "__main__":
    main()
