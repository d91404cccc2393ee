#!/usr/bin/env python3
"""Kernel time per step from a `rocprofv3 --kernel-trace` database (*_results.db): the top kernels by mangled name, the share of
the ragged instantiations (image sizes off the multiples of 64) and of launches under 15 us; with a second
database, time per kernel family side by side.
usage: rocpd_kernel_summary.py <results.db> <steps in the trace> [top N] [second results.db]"""
import collections, re, sqlite3, sys
c = sqlite3.connect(sys.argv[1])
steps = int(sys.argv[2])
sym = dict(c.execute("select id, kernel_name from kernel_symbols").fetchall())
rows = c.execute("select kernel_id, duration from kernels").fetchall()
tot = collections.defaultdict(lambda: [0, 0])
for kid, d in rows:
    n = sym.get(kid, str(kid)).removesuffix(".kd")
    tot[n][0] += d; tot[n][1] += 1
RAGGED = [r"bwd_mask_reduce_kernelI\w+Lb1E", r"dw_wgrad_kernelI\w+Lb1E", r"linattn_bwd_(q|kv)_kernelI\w+Lb1E", r"wgrad_kernelI\w+Lb1E",
          r"ragged", r"pw_gemm_kernelI\w+ELb0ELb1ELb[01]E", r"conv3x3_kernelI\w+ELb1ELb0E"]
def ragged(n):
    return any(re.search(p, n) for p in RAGGED)
allt = sum(v[0] for v in tot.values())
rt = sum(v[0] for n, v in tot.items() if ragged(n))
small = sum(v[0] for n, v in tot.items() if v[0] / v[1] < 15e3)
print(f"{len(rows)} dispatches, {allt/1e6:.2f} ms of kernel time over {steps} steps (warm-up included): {allt/1e6/steps:.2f} ms per step")
print(f"ragged variants (R): {rt/1e6/steps:.2f} ms per step = {100*rt/allt:.1f} % of kernel time")
print(f"kernels averaging < 15 us per launch: {small/1e6/steps:.2f} ms per step = {100*small/allt:.1f} %")
print(f"{'ms/step':>8} {'calls/step':>10} {'us/call':>8}")
for n, v in sorted(tot.items(), key=lambda kv: -kv[1][0])[:int(sys.argv[3]) if len(sys.argv) > 3 else 45]:
    print(f"{v[0]/1e6/steps:8.3f} {v[1]/steps:10.1f} {v[0]/v[1]/1e3:8.1f} {'R' if ragged(n) else ' '} {n[:140]}")
print("ragged instantiations:")
for n, v in sorted(tot.items(), key=lambda kv: -kv[1][0]):
    if ragged(n):
        print(f"{v[0]/1e6/steps:8.3f} {v[1]/steps:10.1f} {v[0]/v[1]/1e3:8.1f} R {n[:140]}")

if len(sys.argv) > 4:  # per kernel family, this trace vs a second one (same step count)
    def families(path):
        c2 = sqlite3.connect(path)
        sy = dict(c2.execute("select id, kernel_name from kernel_symbols").fetchall())
        fam = collections.defaultdict(float)
        for kid, d in c2.execute("select kernel_id, duration from kernels"):
            name = sy.get(kid, "?")
            m = re.match(r"_ZN4llie(\d+)", name)  # mangled: the length-prefixed identifier; else up to the first '('
            key = name[m.end():m.end() + int(m.group(1))] if m else re.split(r"[(<]", name.removeprefix("_Z"))[0]
            fam[key] += d / 1e6 / steps
        return fam
    a, b = families(sys.argv[1]), families(sys.argv[4])
    print(f"{'kernel family':40s} {'this':>8s} {'other':>8s} ratio  (ms per step)")
    for k in sorted(set(a) | set(b), key=lambda k: -max(a.get(k, 0), b.get(k, 0))):
        if max(a.get(k, 0), b.get(k, 0)) >= 0.1:
            r = f"{a.get(k, 0) / b[k]:5.2f}" if b.get(k) else "    -"
            print(f"{k:40s} {a.get(k, 0):8.3f} {b.get(k, 0):8.3f} {r}")
    print(f"{'total':40s} {sum(a.values()):8.3f} {sum(b.values()):8.3f} {sum(a.values()) / sum(b.values()):5.2f}")
