"""The float64 reference of the input conv's data gradient (tests/input_grad_refs.py) against torch's own operators, and the teeth
of its bar: every subtly wrong kernel listed below must fail BAR_INIT_DGRAD on the smallest case of
tests/test_gpu_input_grad_kernel.py.  Runs on the CPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_grad_refs as G  # noqa: E402
from kernel_refs import U, _rt  # noqa: E402

SMALLEST = G.DGRAD_MAPS[0]


def _ratio_of(out, ref, ab, sl):
    err = ((out - ref).abs() - sl).clamp_min(0.0)
    return (err / (U * ab).clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("split", G.DGRAD_SPLITS, ids=[f"c{a}_{b}" for a, b in G.DGRAD_SPLITS])
def test_reference_is_autograd_of_conv2d_and_conv_transpose2d(dtype, split):
    """d(x0), d(x1) of sum(conv2d(cat[x0, x1], w, padding=1) * g) by torch.autograd.grad in float64, and conv_transpose2d(g, w,
    padding=1): both equal the reference to float64 rounding, on a map with partial tiles, at C0 = 64."""
    B, (H, W), C0 = 2, G.DGRAD_MAPS[1], 64
    c0, c1 = split
    g, w = G.dgrad_inputs(dtype, B, H, W, split, C0, 0)
    ref, ab, sl = G.init_conv_dgrad_ref(dtype, g, w)
    assert ref.shape == (B, c0 + c1, H, W) and ref.dtype == torch.float64 and (sl > 0).all() and (ab >= ref.abs() - 1e-12).all()
    gd = _rt(g, dtype).double().permute(0, 3, 1, 2).contiguous()  # NCHW cotangent, exactly as stored
    x0 = torch.zeros(B, c0, H, W, dtype=torch.float64, requires_grad=True)
    xs = [x0] + ([torch.zeros(B, c1, H, W, dtype=torch.float64, requires_grad=True)] if c1 else [])
    y = F.conv2d(torch.cat(xs, 1), w.double(), padding=1)
    grads = torch.autograd.grad(y, xs, gd)
    tol = 1e-12 * ab.max().item()
    assert (torch.cat(grads, 1) - ref).abs().max().item() < tol
    assert (grads[0] - ref[:, :c0]).abs().max().item() < tol
    assert (F.conv_transpose2d(gd, w.double(), padding=1) - ref).abs().max().item() < tol


def _smallest(split, C0, dtype=0):
    g, w = G.dgrad_inputs(dtype, 2, SMALLEST[0], SMALLEST[1], split, C0, 0)
    return _rt(g, dtype).double(), w.double(), G.init_conv_dgrad_ref(dtype, g, w)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_slack_is_the_fp32_store(dtype):
    """the reference rounded to fp32 lies inside the slack: a kernel that is exact up to its fp32 store has ratio 0"""
    gd, wd, (ref, ab, sl) = _smallest((3, 3), 64, dtype)
    assert _ratio_of(ref.float().double(), ref, ab, sl) == 0.0


@pytest.mark.parametrize("variant", ["no_flip", "swap_kykx", "replicate"])
def test_bar_rejects_wrong_taps_and_padding(variant):
    """taps not flipped (correlation instead of the transpose), ky and kx exchanged, zero padding replaced by edge replication"""
    gd, wd, (ref, ab, sl) = _smallest((3, 3), 32)
    kw = {"no_flip": dict(flip=False), "swap_kykx": dict(swap=True), "replicate": dict(replicate=True)}[variant]
    wrong, _ = G.dgrad_sum(gd, wd, **kw)
    assert _ratio_of(wrong, ref, ab, sl) > 100 * G.BAR_INIT_DGRAD


@pytest.mark.parametrize("split", [(1, 2), (4, 4)], ids=["c1_2", "c4_4"])
@pytest.mark.parametrize("shift", [-1, 1])
def test_bar_rejects_a_seam_off_by_one(split, shift):
    """d_x1 starting one channel early (its first plane is x0's last) or one late (its last plane is whatever lay beyond: zeros)"""
    gd, wd, (ref, ab, sl) = _smallest(split, 32)
    c0, c1 = split
    full = torch.cat([ref, torch.zeros_like(ref[:, :1])], 1)
    wrong = torch.cat([ref[:, :c0], full[:, c0 + shift:c0 + shift + c1]], 1)
    assert wrong.shape == ref.shape
    assert _ratio_of(wrong, ref, ab, sl) > 100 * G.BAR_INIT_DGRAD


def test_bar_rejects_a_dropped_second_channel_block():
    """C0 = 64 with output channels 32..63 of g never read"""
    gd, wd, (ref, ab, sl) = _smallest((3, 3), 64)
    w_half = wd.clone()
    w_half[32:] = 0.0
    wrong, _ = G.dgrad_sum(gd, w_half)
    assert _ratio_of(wrong, ref, ab, sl) > 100 * G.BAR_INIT_DGRAD
