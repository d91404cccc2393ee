#!/usr/bin/env python3
"""Per-function sha256 of the gfx950 assembly of every csrc/*.hip, to prove that a host-side change left device code alone.

  tools/kernel_asm_hashes.py hash [csrc dir [a.hip ...]] > hashes.txt   one line per function: file, sha256, symbol
  tools/kernel_asm_hashes.py compare parent.txt change.txt      one row per file, a line per differing function; exit status 1 on any difference

The recipe is the one of profiles/r26/README.md section 1: hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S,
cut per function symbol (its label to .Lfunc_end), comments and __hip_cuid_ lines dropped, the local labels
.LBB<function index>_<k> written .LBB_<k> (the index is the function's position in its file, which any reordering of the
instantiations changes).  The assembly is hashed, never searched.  Needs no GPU.
"""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LOCAL = re.compile(r"\.L(BB|JTI|CPI)\d+_")


def functions(asm):
    """{symbol: normalised body} of one assembly file"""
    out, name, body = {}, None, []
    types = set(re.findall(r"^\s*\.type\s+([^,\s]+),@function", asm, re.M))
    for line in asm.splitlines():
        line = line.split(";", 1)[0].rstrip()
        if not line.strip() or "__hip_cuid_" in line:
            continue
        if name is None:
            if line.endswith(":") and line[:-1] in types:
                name, body = line[:-1], []
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = "\n".join(body), None
            continue
        body.append(LOCAL.sub(lambda m: ".L%s_" % m.group(1), line.strip()))
    return out


def hash_file(path):
    asm = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", path, "-o", "-"],
                         check=True, capture_output=True, text=True, cwd=os.path.dirname(path)).stdout
    return [(os.path.basename(path), hashlib.sha256(b.encode()).hexdigest(), s) for s, b in sorted(functions(asm).items())]


def read(path):
    t = {}
    for line in open(path):
        f, h, s = line.split()
        t[(f, s)] = h
    return t


def main():
    if len(sys.argv) >= 2 and sys.argv[1] == "hash":
        d = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(__file__), "..", "cv-diffusion-model_amd", "csrc")
        d = os.path.abspath(d)
        files = sorted(os.path.join(d, f) for f in (sys.argv[3:] or os.listdir(d)) if f.endswith(".hip"))
        with ThreadPoolExecutor(int(os.environ.get("JOBS", "8"))) as ex:
            for rows in ex.map(hash_file, files):
                for r in rows:
                    print(*r)
        return 0
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        a, b = read(sys.argv[2]), read(sys.argv[3])
        bad, per = 0, {}
        for k in sorted(set(a) | set(b)):  # a function that differs or is missing on one side gets a line of its own
            ha, hb = a.get(k, "-" * 64), b.get(k, "-" * 64)
            bad += ha != hb
            n = per.setdefault(k[0], [0, 0, hashlib.sha256(), hashlib.sha256()])
            n[0] += 1
            n[1] += ha == hb
            n[2].update((k[1] + " " + ha + "\n").encode())
            n[3].update((k[1] + " " + hb + "\n").encode())
            if ha != hb:
                print("DIFFERENT", k[0], k[1], ha, hb)
        print("# file  functions  identical  sha256[:16] over the sorted (symbol, sha256) lines: parent, change")
        for f, (n, same, da, db) in sorted(per.items()):
            print("%-14s %4d %4d  %s %s" % (f, n, same, da.hexdigest()[:16], db.hexdigest()[:16]))
        print("# total %d functions, %d missing or different" % (len(set(a) | set(b)), bad))
        return 1 if bad else 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
