"""The cycle-stamped diagnostic builds (knobs "gemm_stamp", "pwx_stamp", "conv_stamp", "irbx_stamp") and what reads them back
(llie_debug_*_stamps).  One case per stamped build, through the kernel-level entry point, at the smallest shape that reaches the
stamped instantiation (fp16 only: the stamped builds exist for fp16):

  * the call returns 0 and leaves the output bytes of the same call with the knob at 0
  * llie_debug_*_stamps returns 0 and its last value is the launch's wave count, workgroups x 4, with the grid from
    llie_expand_dw_plan or from the launcher's grid formula restated here
  * every slot the build uses is finite and >= 0, and some slot is > 0
  * the knob is 0 again afterwards

and, in a fresh process: a family that has not been stamped answers LLIE_ERR_ARG.
"""
import ctypes as C
import importlib
import math
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

F16 = 1
WAVES_PER_WG = 4  # every stamped build runs 256-thread workgroups at these shapes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _stamped(knob, value, run, fetch, nslots, used, waves):
    """run() -> tensors, with the knob at 0 and then at `value`; the checks of the module docstring"""
    L = N.lib()
    name = knob.encode()
    assert L.llie_tune(name, 0) == 0
    plain = [t.cpu() for t in run()]
    out = (C.c_double * (nslots + 1))(*([float("nan")] * (nslots + 1)))
    try:
        assert L.llie_tune(name, value) == 0
        got = [t.cpu() for t in run()]
        assert fetch(out) == 0, N.last_error()
    finally:
        assert L.llie_tune(name, 0) == 0
    for a, b in zip(plain, got):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    vals = list(out)
    print(f"{knob}={value}: {vals}")
    assert vals[nslots] == waves, (vals[nslots], waves)
    assert all(math.isfinite(vals[i]) and vals[i] >= 0 for i in range(used)), vals
    assert any(vals[i] > 0 for i in range(used)), vals


def _segs(x, sc, bi, act=3):
    arr = (N.GemmSeg * 1)()
    arr[0] = N.GemmSeg(x.data_ptr(), x.shape[1], sc.data_ptr(), bi.data_ptr(), x.shape[1], act)
    return arr


def _gemm_operands(dev, P, K, nout, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(P, K, generator=g) * 1.5).half().to(dev)
    w32 = (torch.randn(nout, K, generator=g) / math.sqrt(K)).to(dev)
    sc = ((torch.rand(1, K, generator=g) + 0.5) / 6).to(dev)  # tables of ACT_RELU6_S6: scale / 6, shift / 6
    bi = ((torch.randn(1, K, generator=g) * 0.5 + 0.4) / 6).to(dev)
    return x, w32, sc, bi


def test_unstamped_family_is_an_argument_error(dev):
    """In a process that has stamped nothing, each llie_debug_*_stamps answers LLIE_ERR_ARG (the buffer is valid, so it is the
    'nothing was stamped' refusal).  A child process: the other cases of this module stamp every family in this one."""
    code = ("import ctypes, sys\n"
            "L = ctypes.CDLL(sys.argv[1])\n"
            "out = (ctypes.c_double * 16)()\n"
            "print(*[getattr(L, 'llie_debug_%s_stamps' % f)(out) for f in ('gemm', 'pwx', 'conv', 'irbx')])\n")
    r = subprocess.run([sys.executable, "-c", code, N.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(v) for v in r.stdout.split()] == [N.ERR_ARG] * 4, r.stdout


def test_gemm_stamp(dev):
    """llie_pw_gemm at B = 1, P = 128, N = 32, K = 64: pw_gemm_kernel<_Float16, 128, 32, 4, 1, 64>, one workgroup
    (grid = images x ceil(P / 128) x N / 32)."""
    L = N.lib()
    P, K, nout = 128, 64, 32
    x, w32, sc, bi = _gemm_operands(dev, P, K, nout, 1)
    w = w32.half()
    arr = _segs(x, sc, bi)

    def run():
        out = torch.full((P, nout), float("nan"), dtype=torch.float16, device=dev)
        stats = torch.full((1, 1, 2, nout), float("nan"), device=dev)
        N.check(L.llie_pw_gemm(F16, arr, 1, w.data_ptr(), None, None, out.data_ptr(), stats.data_ptr(), P, nout, P, _st()), "pw_gemm")
        torch.cuda.synchronize()
        return out, stats

    grid = 1 * ((P + 127) // 128) * (nout // 32)
    _stamped("gemm_stamp", 1, run, L.llie_debug_gemm_stamps, 2, 2, grid * WAVES_PER_WG)


def test_pwx_stamp(dev):
    """llie_pw_expand at B = 1, P = 128, K = 192, N = 64: pw_expand_kernel<_Float16, 12, 1>; grid = M / 128 x nsplit."""
    L = N.lib()
    P, K, nout = 128, 192, 64
    x, w32, sc, bi = _gemm_operands(dev, P, K, nout, 2)
    arr = _segs(x, sc, bi)
    wpack = torch.empty(nout * K, dtype=torch.float16, device=dev)

    def run():
        out = torch.full((P, nout), float("nan"), dtype=torch.float16, device=dev)
        stats = torch.full((1, P // 128, 2, nout), float("nan"), device=dev)
        N.check(L.llie_pw_expand(F16, arr, 1, w32.data_ptr(), wpack.data_ptr(), out.data_ptr(), stats.data_ptr(), P, nout, P, _st()), "pw_expand")
        torch.cuda.synchronize()
        return out, stats

    # pwx.hip, nsplit_for (32-channel blocks per buffer: 1): the channels of a pixel tile are split while the launch has fewer than
    # 512 workgroups and each part keeps an even number of blocks, at least two of them, in 64-channel pairs
    ns = 1
    while (P // 128) * ns < 512 and (nout // 32) % (2 * ns) == 0 and nout // (64 * ns) >= 2 and (nout // (2 * ns)) % 64 == 0:
        ns *= 2
    assert ns == 1
    _stamped("pwx_stamp", 1, run, L.llie_debug_pwx_stamps, 3, 3, (P // 128) * ns * WAVES_PER_WG)


def test_conv_stamp(dev):
    """llie_conv3x3 mode 1 (bilinear x2, then 3x3) at 8 x 8 -> 16 x 16, C = 32: conv3x3_kernel<_Float16, 1, 16, 32, 4, 1>;
    grid = images x Ho / 8 x Wo / 16 x Cout / 32."""
    L = N.lib()
    Hi, Cc = 8, 32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, Hi, Hi, Cc, generator=g).half().to(dev)
    w = (torch.randn(9, Cc, Cc, generator=g) / math.sqrt(9 * Cc)).half().to(dev)
    bias = (0.1 * torch.randn(Cc, generator=g)).to(dev)
    Ho = 2 * Hi
    nt = int(L.llie_conv3x3_tiles(Ho, Ho))

    def run():
        out = torch.full((1, Ho, Ho, Cc), float("nan"), dtype=torch.float16, device=dev)
        stats = torch.full((1, nt, 2, Cc), float("nan"), device=dev)
        N.check(L.llie_conv3x3(F16, 1, x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), stats.data_ptr(), 1, Hi, Hi, Cc, Cc, _st()), "conv3x3")
        torch.cuda.synchronize()
        return out, stats

    grid = 1 * (Ho // 8) * (Ho // 16) * (Cc // 32)
    _stamped("conv_stamp", 1, run, L.llie_debug_conv_stamps, 7, 7, grid * WAVES_PER_WG)


def _block_operands(dev, cin, H, W, seed):
    """operands of the recompute kernels as the engine hands them over: norm1's tables / 6, norm2's undivided"""
    g = torch.Generator().manual_seed(seed)
    chid = 4 * cin
    t = {"x": torch.randn(1, H, W, cin, generator=g).half(), "s1": 0.15 + 0.1 * torch.rand(1, cin, generator=g),
         "b1": 0.3 + 0.2 * torch.rand(1, cin, generator=g), "w1": (torch.randn(chid, cin, generator=g) / math.sqrt(cin)).half(),
         "s2": 0.5 + torch.rand(1, chid, generator=g), "b2": 1.0 + 2.0 * torch.rand(1, chid, generator=g),
         "wd": 0.3 * torch.randn(9, chid, generator=g), "gate": torch.rand(1, chid, generator=g),
         "wp": (torch.randn(cin, chid, generator=g) / math.sqrt(chid)).half()}
    return {k: v.to(dev) for k, v in t.items()}


def _plan_workgroups(cin, B, H, W, project):
    plan = (C.c_int * 4)()
    N.check(N.lib().llie_expand_dw_plan(cin, B, H, W, project, plan), "expand_dw_plan")
    return plan[2] * plan[3] * B


@pytest.mark.parametrize("stamp", [1, 2, 3])
def test_irbx_stamp(dev, stamp):
    """c0 = 32, H = 8, W = 16, B = 1: expand_dw ("irbx_stamp" = 1, nine slots), expand_pool (2, five slots; one workgroup per
    llie_irbx_stats_rows(H W) pixels of an image) and expand_dw_project (3, nine slots)."""
    L = N.lib()
    cin, H, W = 32, 8, 16
    chid = 4 * cin
    d = _block_operands(dev, cin, H, W, 4)
    front = (F16, d["x"].data_ptr(), cin, None, 0, d["s1"].data_ptr(), d["b1"].data_ptr(), d["w1"].data_ptr(), d["s2"].data_ptr(),
             d["b2"].data_ptr(), d["wd"].data_ptr())

    def run_dw():
        h2 = torch.full((1, H, W, chid), float("nan"), dtype=torch.float16, device=dev)
        tot = torch.zeros(1, chid, dtype=torch.int64, device=dev)
        N.check(L.llie_expand_dw(*front, h2.data_ptr(), tot.data_ptr(), 1, H, W, _st()), "expand_dw")
        torch.cuda.synchronize()
        return h2, tot

    def run_pool():
        tot = torch.zeros(1, chid, dtype=torch.int64, device=dev)
        N.check(L.llie_expand_pool(*front, tot.data_ptr(), 1, H, W, _st()), "expand_pool")
        torch.cuda.synchronize()
        return (tot,)

    def run_project():
        y = torch.full((1, H, W, cin), float("nan"), dtype=torch.float16, device=dev)
        stats = torch.full((1, int(L.llie_irbx_project_tiles(H, W)), 2, cin), float("nan"), device=dev)
        N.check(L.llie_expand_dw_project(F16, d["x"].data_ptr(), cin, d["s1"].data_ptr(), d["b1"].data_ptr(), d["w1"].data_ptr(), d["s2"].data_ptr(),
                                         d["b2"].data_ptr(), d["wd"].data_ptr(), d["gate"].data_ptr(), d["wp"].data_ptr(), y.data_ptr(),
                                         stats.data_ptr(), 1, H, W, _st()), "expand_dw_project")
        torch.cuda.synchronize()
        return y, stats

    run, used, wgs = {1: (run_dw, 9, _plan_workgroups(cin, 1, H, W, 0)),
                      2: (run_pool, 5, H * W // int(L.llie_irbx_stats_rows(H * W))),
                      3: (run_project, 9, _plan_workgroups(cin, 1, H, W, 1))}[stamp]
    _stamped("irbx_stamp", stamp, run, L.llie_debug_irbx_stamps, 9, used, wgs * WAVES_PER_WG)
