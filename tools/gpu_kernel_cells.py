#!/usr/bin/env python3
"""Every device result the kernel-level GPU tests read back, as one line per read: test id, sha256 of the bytes, and
llie_last_kernel() at that moment.  Two builds of the library that compute the same bits and launch the same kernels give
the same file, so a host-side change is checked with

  cp ab/libA.so cv-diffusion-model_amd/libllie_hip.so && python tools/gpu_kernel_cells.py cells_A.txt
  cp ab/libB.so cv-diffusion-model_amd/libllie_hip.so && python tools/gpu_kernel_cells.py cells_B.txt
  cmp cells_A.txt cells_B.txt
  python tools/gpu_kernel_cells.py summary cells_A.txt cells_B.txt     one row per test function instead of one per read

(each run in a fresh process).  The cells are those of the kernel-level test modules (MODULES): every launch path, dtype, tile width,
ragged and whole map of the launchers behind the C ABI, on the tests' seeded inputs.  The tests' own assertions run as usual; the
exit status is pytest's.
"""
import hashlib
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODULES = ["forward_kernels", "backward_kernels", "boundary_kernels", "softattn_kernels", "expand_dw_paths", "irbx_prologue", "input_grad_kernel",
           "upconv_fold", "upconv_maps", "upconv_maps_items", "expand_dw_project", "expand_dw_project_skip", "expand_dw_project_tail", "expand_scan",
           "expand_pool_border", "wide_project", "wide_gram", "weight_loading", "stamps", "irb_paths", "round2", "round3", "round4",
           "expand_gram_kernels"]


class Recorder:
    def __init__(self, out):
        self.out, self.test, self.k = out, "-", 0
        self.lib = importlib.import_module("cv-diffusion-model_amd._native").lib()
        cpu = torch.Tensor.cpu
        rec = self

        def recording_cpu(t, *a, **kw):
            r = cpu(t, *a, **kw)
            if t.is_cuda:
                b = r.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
                rec.out.write(f"{rec.test}#{rec.k} {tuple(r.shape)} {str(r.dtype)[6:]} {hashlib.sha256(b).hexdigest()[:16]} "
                              f"{(rec.lib.llie_last_kernel() or b'-').decode()}\n")
                rec.k += 1
            return r
        torch.Tensor.cpu = recording_cpu

    def pytest_runtest_setup(self, item):
        self.test, self.k = item.nodeid.split("/")[-1], 0


def summary(pa, pb):
    """per test function: cases, reads, sha256[:16] over its lines in either file; then the kernel names by kernel"""
    rows, names = {}, [set(), set()]
    for i, p in enumerate((pa, pb)):
        for line in open(p):
            tid, name = line.split("#", 1)[0], line.rstrip("\n").split(" ", 1)[1].split(") ", 1)[1].split(" ", 2)[2]
            r = rows.setdefault(tid.split("[", 1)[0], [set(), 0, hashlib.sha256(), hashlib.sha256()])
            r[0].add(tid)
            r[1] += i == 0
            r[2 + i].update(line.encode())
            names[i].add(name)
    print("# test function  cases  reads  sha256[:16] over its reads (id, shape, dtype, sha256 of the bytes, llie_last_kernel): A, B")
    bad = 0
    for f, (cases, reads, da, db) in rows.items():
        bad += da.digest() != db.digest()
        print(f, len(cases), reads, da.hexdigest()[:16], db.hexdigest()[:16], "" if da.digest() == db.digest() else "DIFFERENT")
    print("# kernel  distinct names recorded: A, B")
    for k in sorted({n.split("<")[0] for n in names[0] | names[1]}):
        print(k, *(sum(n.split("<")[0] == k for n in ns) for ns in names))
    print(f"# {len(rows)} test functions, {bad} differ; names {'equal' if names[0] == names[1] else 'DIFFERENT'}")
    return 1 if bad or names[0] != names[1] else 0


def main():
    if sys.argv[1] == "summary":
        return summary(sys.argv[2], sys.argv[3])
    with open(sys.argv[1], "w") as out:
        files = [os.path.join(ROOT, "tests", f"test_gpu_{m}.py") for m in MODULES]
        return int(pytest.main(["-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", *files], plugins=[Recorder(out)]))


if __name__ == "__main__":
    sys.exit(main())
