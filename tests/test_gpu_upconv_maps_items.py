"""The item loop of the up-sampling conv from nine tap maps (csrc/upconv.hip: conv3x3_upmaps_kernel), and the rest of its contract.

The kernel's grid is sized to the chip: min(items, compute units) workgroups, each working through items blockIdx.x, + gridDim.x,
...; one LDS region serves the operand buffers, then the maps, then the statistics scratch; the next item's first loads are issued
before this item's blend.  On a chip with more compute units than a test has items no workgroup ever takes a second item, so
llie_conv3x3_upmaps_grid launches an explicit number of workgroups: the same small shapes then run the loop with one workgroup
taking every item, with uneven tails and with the last round partly empty.  Which workgroup computes an item changes no bit, so
the yardstick is the launch with one workgroup per item, which test_gpu_upconv_maps.py holds to float64.  Output and statistics
are pre-filled with NaN before every launch.  TH x TW = 8 x 16 is the kernel's tile; an item is (image, tile, 32 output channels).

To add a case: a row in GRID_CASES = (C, B, Hi, Wi, grids); nitems = B (Hi / 8) (Wi / 16) (C / 32), the item order is the XCD
order where B (Hi / 8) (Wi / 16) is a multiple of 8 and the plain one otherwise, and every grid below nitems loops."""
import functools
import importlib
import math

import pytest
import torch

import test_gpu_upconv_maps as T
from test_upconv_fold_host import upconv_ref_f64

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

TH, TW = T.TH, T.TW
DTYPES = T.DTYPES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nitems(B, H, W, C):
    return B * (H // TH) * (W // TW) * (C // 32)


def _launch(dev, dtype, tdt, xd, wd, bd, B, H, W, C, grid, with_stats=True):
    """llie_conv3x3_upmaps_grid on `grid` workgroups (None: llie_conv3x3_upmaps, the rule) -> (out, stats or None), NaN-filled first."""
    L = N.lib()
    out = torch.full((B, 4 * H * W, C), float("nan"), dtype=tdt, device=dev)
    stats = torch.full((B, 4 * (H // TH) * (W // TW), 2, C), float("nan"), device=dev) if with_stats else None
    args = (dtype, xd.data_ptr(), wd.data_ptr(), None if bd is None else bd.data_ptr(), out.data_ptr(), None if stats is None else stats.data_ptr(),
            B, H, W, C)
    if grid is None:
        N.check(L.llie_conv3x3_upmaps(*args, T._stream()), "conv3x3_upmaps")
    else:
        N.check(L.llie_conv3x3_upmaps_grid(*args, grid, T._stream()), "conv3x3_upmaps_grid")
    torch.cuda.synchronize()
    return out, stats


@functools.lru_cache(maxsize=None)
def _inputs(C, H, W, tdt, B):
    """Different random data in every image and tile -> x NHWC [B][H * W][C] tdt, w [9][C][C] tdt (tap-major), bias fp32, on the CPU."""
    g = torch.Generator().manual_seed(7 * C + 10 * H + W + 1000 * B)
    x = torch.randn(B, H * W, C, generator=g).to(tdt)
    w = (torch.randn(9, C, C, generator=g) / math.sqrt(9 * C)).to(tdt)
    return x, w, torch.randn(C, generator=g) * 0.1


_YARD = {}


def _yardstick(dev, dtype, tdt, C, B, H, W):
    """One workgroup per item on _inputs(...), once per case -> (x, w, bias on the device, out, stats); nothing left NaN."""
    key = (dtype, C, B, H, W)
    if key not in _YARD:
        xd, wd, bd = (t.to(dev) for t in _inputs(C, H, W, tdt, B))
        out, stats = _launch(dev, dtype, tdt, xd, wd, bd, B, H, W, C, _nitems(B, H, W, C))
        assert torch.isfinite(out).all() and torch.isfinite(stats).all()
        _YARD[key] = (xd, wd, bd, out, stats)
    return _YARD[key]


# ------------------------------------------------------------------ a. any grid, same bits
GRID_CASES = [
    (128, 1, TH, TW, (1, 2, 3)),                   # 4 items, plain order
    (256, 2, 2 * TH, 2 * TW, (1, 3, 8, 24, 63)),   # 64 items, 8 (image, tile) pairs: the XCD order
    (128, 3, TH, 2 * TW, (1, 5, 7, 16)),           # 24 items, 6 pairs: plain order
] + [(C, 2, TH, TW, (1,)) for C in T.NEW_C]        # one workgroup through every item at the chunk counts 1, 2, 3 and 5


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("C,B,H,W,grid", [(C, B, H, W, g) for C, B, H, W, grids in GRID_CASES for g in grids])
def test_any_grid_gives_the_bits_of_one_item_per_workgroup(dev, dtype, tdt, C, B, H, W, grid):
    """Grid 1: one workgroup takes every item in sequence; 3, 5, 7, 63: uneven tails, some workgroups run one item more than
    others and the last round is partly empty.  Three launches each, all bit-equal to the one-item-per-workgroup launch in output
    and statistics (a race need not show on the first), nothing left NaN."""
    nitems = _nitems(B, H, W, C)
    assert grid < nitems
    xd, wd, bd, out0, st0 = _yardstick(dev, dtype, tdt, C, B, H, W)
    for rep in range(3):
        out, stats = _launch(dev, dtype, tdt, xd, wd, bd, B, H, W, C, grid)
        assert not torch.isnan(out).any() and not torch.isnan(stats).any(), rep
        assert torch.equal(out, out0), (rep, (out.float() - out0.float()).abs().max().item())
        assert torch.equal(stats, st0), rep


# ------------------------------------------------------------------ b. NaN does not cross items
@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("grid", [1, 8])
@pytest.mark.parametrize("poisoned", [0, 1])
def test_nan_image_does_not_reach_the_other_image(dev, dtype, tdt, grid, poisoned):
    """The 64-item case with one image all NaN: the other image's output and statistics are the bits of its clean
    one-item-per-workgroup launch, the NaN image's output is NaN everywhere.  With grid 1 the clean image's items follow (poisoned
    0) or alternate with NaN items in one workgroup; stale maps, statistics scratch or bias would carry the NaN over."""
    C, B, H, W = 256, 2, 2 * TH, 2 * TW
    xd, wd, bd, out0, st0 = _yardstick(dev, dtype, tdt, C, B, H, W)
    xp = xd.clone()
    xp[poisoned] = float("nan")
    out, stats = _launch(dev, dtype, tdt, xp, wd, bd, B, H, W, C, grid)
    clean = 1 - poisoned
    assert torch.equal(out[clean], out0[clean]) and torch.equal(stats[clean], st0[clean])
    assert torch.isnan(out[poisoned]).all()


# ------------------------------------------------------------------ c. the rule itself loops
def _rule_workgroups():
    """The rule's workgroup count once there are more items than it launches (None where it launches one per item whatever their
    number: compute units no multiple of 8)."""
    big = 1 << 12
    w = int(N.lib().llie_conv3x3_upmaps_workgroups(big, TH, TW, 256))
    assert w > 0, w
    return None if w == 8 * big else w


def _looping_batches(w):
    """C = 256 at 8 x 16 is 8 items per image.  -> [(B, order)]: the smallest B with 8 B >= 2 w + 8 that is no multiple of 8 (plain
    order: the first workgroups take three items, the others two), the next such B but one (a longer third round), and the smallest
    multiple of 8 above the first (the XCD order)."""
    b1 = (2 * w + 8 + 7) // 8
    while b1 % 8 == 0:
        b1 += 1
    b2 = b1 + 2
    while b2 % 8 == 0:
        b2 += 1
    return [(b1, "plain"), (b2, "plain"), ((b1 // 8 + 1) * 8, "XCD")]


def test_rule_workgroups_is_the_documented_rule(dev):
    """llie_conv3x3_upmaps_workgroups = min(items, compute units), or the items where the compute units are no multiple of 8."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    L = N.lib()
    for B, H, W, C in [(1, TH, TW, 32), (1, TH, TW, 128), (2, 2 * TH, 2 * TW, 256), (64, TH, TW, 256), (67, TH, TW, 256), (3, 5 * TH, 7 * TW, 96)]:
        n = _nitems(B, H, W, C)
        assert L.llie_conv3x3_upmaps_workgroups(B, H, W, C) == (n if cus & 7 else min(n, cus)), (B, H, W, C, cus)
    print(f"compute units {cus}, rule's workgroup count with items to spare: {_rule_workgroups()}")


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_rule_launch_that_loops(dev, dtype, tdt, which):
    """llie_conv3x3_upmaps itself (no explicit grid) at batches with more than twice as many items as workgroups, so that image
    B - 1 is computed as a third item: bit-equal to the same images in launches of at most w // 8 images, which the rule gives
    one workgroup per item; images 0, B // 2 and B - 1 against float64 within 1.5 x the max-abs error of llie_conv3x3 mode 1 on the
    same three images (the bar of test_upmaps_entry_point_vs_float64)."""
    w = _rule_workgroups()
    if w is None:
        pytest.skip("the rule launches one workgroup per item on this device (compute units no multiple of 8): it cannot loop")
    C, H, W = 256, TH, TW
    B, order = _looping_batches(w)[which]
    nitems = _nitems(B, H, W, C)
    L = N.lib()
    assert L.llie_conv3x3_upmaps_workgroups(B, H, W, C) == w
    print(f"{tdt} {order} order: workgroups {w}, B = {B}, nitems {nitems} > workgroups {w}: {nitems > w}, third-round items {nitems - 2 * w}")
    assert nitems > 2 * w and (B % 8 == 0) == (order == "XCD")
    x, wq, b = _inputs(C, H, W, tdt, B)
    xd, wd, bd = x.to(dev), wq.to(dev), b.to(dev)
    out, stats = _launch(dev, dtype, tdt, xd, wd, bd, B, H, W, C, None)
    assert not torch.isnan(out).any() and not torch.isnan(stats).any()
    per = w // 8
    for k in range(0, B, per):
        n = min(per, B - k)
        assert L.llie_conv3x3_upmaps_workgroups(n, H, W, C) == 8 * n
        o, s = _launch(dev, dtype, tdt, xd[k:k + n].contiguous(), wd, bd, n, H, W, C, None)
        assert torch.equal(out[k:k + n], o) and torch.equal(stats[k:k + n], s), k
    pick = [0, B // 2, B - 1]
    xs = x[pick].contiguous()
    ref = upconv_ref_f64(xs.float().view(3, H, W, C).permute(0, 3, 1, 2), wq.float().view(3, 3, C, C).permute(2, 3, 0, 1), b)
    got = T._nchw(out[pick], 3, H, W, C)
    old = T._nchw(T._run_blend(dev, dtype, tdt, xs.to(dev), wd, bd, 3, H, W, C), 3, H, W, C)
    err, err_old = (got - ref).abs().max().item(), (old - ref).abs().max().item()
    per_image = [(got[i] - ref[i]).abs().max().item() for i in range(3)]
    print(f"  images {pick}: max-abs error maps {err:.3e} (per image {', '.join(f'{e:.3e}' for e in per_image)}), blending kernel {err_old:.3e} "
          f"(ratio {err / err_old:.3f})")
    assert err <= 1.5 * err_old, (err, err_old)


# ------------------------------------------------------------------ d. through the engine
@pytest.mark.parametrize("which", [0, 2])
def test_engine_forward_that_loops(dev, which):
    """A bare Upsample engine at fp16, C = 256, 8 x 16, at the looping batches of the plain and the XCD order: the path with the
    non-temporal stores, the engine's weights blob and the rule as forward.cpp calls it.  The profile names the tap-map kernel;
    the result equals, image by image and bit for bit, the same module on batches of at most w // 8 images (the module is the conv
    plus element-wise layout changes); images 0 and B - 1 are within 1.5 x the error of llie_conv3x3 mode 1 against float64
    interpolate + conv2d on the rounded inputs and weights."""
    w = _rule_workgroups()
    if w is None:
        pytest.skip("the rule launches one workgroup per item on this device (compute units no multiple of 8): it cannot loop")
    C, H, W = 256, TH, TW
    B, order = _looping_batches(w)[which]
    assert _nitems(B, H, W, C) > 2 * w
    whole, batched, names, x, wt, b = T._up_forward(dev, "fp16", H, W, C, B, w // 8)
    assert names and all(n.startswith("conv3x3_upmaps_kernel<") for n in names), names
    assert not torch.isnan(whole).any() and not torch.isnan(batched).any()
    for k in range(B):
        assert torch.equal(whole[k], batched[k]), k
    pick = [0, B - 1]
    tdt = torch.float16
    xq, wq = x[pick].to(tdt), wt.to(tdt)
    ref = upconv_ref_f64(xq.float(), wq.float(), b)
    xd = xq.permute(0, 2, 3, 1).reshape(2, H * W, C).contiguous().to(dev)
    wd = wq.permute(2, 3, 0, 1).reshape(9, C, C).contiguous().to(dev)
    old = T._nchw(T._run_blend(dev, 1, tdt, xd, wd, b.to(dev), 2, H, W, C), 2, H, W, C)
    err, err_old = (whole[pick].double() - ref).abs().max().item(), (old - ref).abs().max().item()
    print(f"engine fp16 {order} order: workgroups {w}, B = {B}, kernels {names}; images {pick}: max-abs error {err:.3e}, blending kernel "
          f"{err_old:.3e} (ratio {err / err_old:.3f})")
    assert err <= 1.5 * err_old, (err, err_old)


# ------------------------------------------------------------------ optional arguments
@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("grid", [1, 8])
def test_null_bias_and_null_stats(dev, dtype, tdt, grid):
    """C = 128, 8 x 16, B = 2 (8 items), one workgroup for all and one per item: bias = NULL gives the bits of a zero bias vector
    (output and statistics), stats = NULL gives the output bits of the launch with a slab."""
    C, B, H, W = 128, 2, TH, TW
    assert _nitems(B, H, W, C) == 8
    xd, wd, bd, out0, _ = _yardstick(dev, dtype, tdt, C, B, H, W)
    oz, sz = _launch(dev, dtype, tdt, xd, wd, torch.zeros(C, device=dev), B, H, W, C, grid)
    on, sn = _launch(dev, dtype, tdt, xd, wd, None, B, H, W, C, grid)
    assert not torch.isnan(on).any() and not torch.isnan(sn).any()
    assert torch.equal(on, oz) and torch.equal(sn, sz)
    assert not torch.equal(on, out0)  # the bias of the case is not zero: the comparison above is not vacuous
    o, none = _launch(dev, dtype, tdt, xd, wd, bd, B, H, W, C, grid, with_stats=False)
    assert none is None and torch.equal(o, out0)
