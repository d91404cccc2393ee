"""Float64 reference of the input conv's data gradient (llie_init_conv_dgrad, bwd.hip: init_conv_dgrad_kernel), its bar, and the
cases tests/test_gpu_input_grad_kernel.py and tests/test_input_grad_host.py share.  Method and helpers: tests/kernel_refs.py.

    dx[b][ci][y][x] = sum_{ky, kx in 0..2} sum_{co < C0} g[b][y + 1 - ky][x + 1 - kx][co] * w[co][ci][ky][kx]    (outside the map: 0)

the transpose of init_conv (out[y][x] = sum x[y - 1 + ky][x - 1 + kx] w[ky][kx], zero padding).
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_refs import _rt, _ulp, seeded  # noqa: E402

# (H, W): one 16 x 16 tile of the kernel; partial tiles on the right and bottom edges; three and four tiles along the axes, so that
# tiles with neighbours on all four sides exist; 40 x 24: higher than wide, so non-square maps come both ways round.
DGRAD_MAPS = [(16, 16), (24, 40), (48, 56), (40, 24)]
DGRAD_SPLITS = [(3, 3), (4, 4), (1, 2), (3, 0)]
DGRAD_COUT = [32, 64]


def dgrad_inputs(dtype, B, H, W, split, C0, seed0):
    """-> (g fp32 draws [B][H][W][C0] -- the kernel is given _rt(g, dtype) --, w fp32 OIHW [C0][c0 + c1][3][3])"""
    gn = seeded(seed0, "init_dgrad", dtype, H, W, split, C0)
    g = torch.randn(B, H, W, C0, generator=gn)
    w = torch.randn(C0, split[0] + split[1], 3, 3, generator=gn) / math.sqrt(9 * C0)
    return g, w


def dgrad_sum(gd, wd, flip=True, swap=False, replicate=False):
    """sum over the nine taps of the window of `gd` [B][H][W][C0] (float64) times wd[:, :, ky, kx] ([C0][Cin]); -> (sum, absolute
    sum), NCHW [B][Cin][H][W].  The defaults are the definition; the switches build the wrong kernels tests/test_input_grad_host.py
    holds the bar against: flip=False reads g[y - 1 + ky][x - 1 + kx] (correlation, not the transpose), swap exchanges ky and kx in
    the weight, replicate pads g with its edge values instead of zeros."""
    B, H, W, _ = gd.shape
    if replicate:
        gp = torch.nn.functional.pad(gd.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
    else:
        gp = torch.nn.functional.pad(gd, (0, 0, 1, 1, 1, 1))
    ref, ab = 0.0, 0.0
    for ky in range(3):
        for kx in range(3):
            oy, ox = (2 - ky, 2 - kx) if flip else (ky, kx)  # padded row of g[y + 1 - ky] is y + 2 - ky
            win = gp[:, oy:oy + H, ox:ox + W, :]
            wt = wd[:, :, kx, ky] if swap else wd[:, :, ky, kx]
            ref, ab = ref + win @ wt, ab + win.abs() @ wt.abs()
    return ref.permute(0, 3, 1, 2).contiguous(), ab.permute(0, 3, 1, 2).contiguous()


def init_conv_dgrad_ref(dtype, g, w):
    """llie_init_conv_dgrad: g [B][H][W][C0] (any float type; the values the kernel reads are _rt(g, dtype), taken exactly as stored),
    w fp32 OIHW [C0][Cin][3][3] (used as given: the kernel reads the fp32 table).  Roundings mirrored: none -- products and sums are
    fp32 in the kernel, float64 here; the output is fp32.  -> (ref, abssum, slack), float64 NCHW [B][Cin][H][W]; abssum the sum of
    |term| per entry, slack one fp32 ulp of ref.  Channels [0, c0) are d_x0, the rest d_x1."""
    ref, ab = dgrad_sum(_rt(g, dtype).double(), w.float().double())
    return ref, ab, _ulp(ref, 0)


# BAR x 2^-24 x abssum per entry (kernel_refs.py: "bars").  worst = the worst ratio |out - ref| / (2^-24 abssum) after the slack, measured
# on the MI355X over every case of tests/test_gpu_input_grad_kernel.py::test_init_conv_dgrad_vs_float64 and LLIE_FWD_TEST_SEED 0, 1, 2,
# as fp32 / fp16 / bf16; the bar is about 10x that (and far below 1e-4 of the absolute sum, which would be 1678).
BAR_INIT_DGRAD = 31.0  # worst 3.04 / 3.00 / 3.15 (an entry is the sum of two chains of 9 C0 / 2 fused multiply-adds, 144 or 288 long)
