"""The identity behind the up-sampling conv from nine low-resolution tap maps (csrc/upconv.hip: conv3x3_upmaps_kernel), pinned in
float64 without a GPU.

    y = conv3x3(up2(x), w, pad 1),   up2 = F.interpolate(scale_factor=2, mode="bilinear", align_corners=False)

is linear in x and up2 is fixed: with Z_t = W_t x, the nine 1x1 maps of the LOW-resolution input (t = (dy, dx)),

    y(oy, ox) = bias + sum over the taps t whose position (oy + dy - 1, ox + dx - 1) lies inside the 2H x 2W image of up2(Z_t) there.

up2 is the replicate clamp of the low-resolution neighbour index with weights 1/4 and 3/4; the conv's zero padding is a term left
out.  upconv_maps_f64 applies the identity the way the kernel does (separably: columns, then rows), and with `tdt` rounds where
the kernel rounds: the inputs and weights are taken as given, the maps are rounded to the compute dtype once, the blend and the
bias are added in higher precision, the result is rounded.  The GPU tests (test_gpu_upconv_maps.py) reuse it.

The entry points' refusals (llie_conv3x3_upmaps, llie_conv3x3_upmaps_grid) are checked here too: they come before any HIP call."""
import ctypes
import importlib

import pytest
import torch

from test_upconv_fold_host import upconv_ref_f64


def _up2_axis(z, dim):
    """Bilinear x2 along `dim` as clamp + 1/4, 3/4: even sample 2m = 1/4 z[m - 1] + 3/4 z[m], odd 2m + 1 = 3/4 z[m] + 1/4 z[m + 1]."""
    n = z.shape[dim]
    idx = torch.arange(n)
    lo, hi = z.index_select(dim, (idx - 1).clamp(min=0)), z.index_select(dim, (idx + 1).clamp(max=n - 1))
    even, odd = 0.25 * lo + 0.75 * z, 0.75 * z + 0.25 * hi
    return torch.stack([even, odd], dim + 1).flatten(dim, dim + 1)


def _shift(u, d, dim):
    """v[o] = u[o + d - 1] along `dim` where that lies inside, else 0: the tap's position, out-of-image terms dropped."""
    n = u.shape[dim]
    v = torch.zeros_like(u)
    if d == 0:
        v.narrow(dim, 1, n - 1).copy_(u.narrow(dim, 0, n - 1))
    elif d == 1:
        v.copy_(u)
    else:
        v.narrow(dim, 0, n - 1).copy_(u.narrow(dim, 1, n - 1))
    return v


def upconv_maps_f64(x, w, bias, tdt=None):
    """x [B][I][H][W], w [O][I][3][3], bias [O] -> [B][O][2H][2W] float64 by the nine-map identity.  tdt: round the maps and the
    result to that dtype, as the kernel does (x and w are then expected to be rounded already)."""
    x, w = x.double(), w.double()
    y = torch.zeros(x.shape[0], w.shape[0], 2 * x.shape[2], 2 * x.shape[3], dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            z = torch.einsum("oi,bihw->bohw", w[:, :, dy, dx], x)
            if tdt is not None:
                z = z.to(tdt).double()
            y += _shift(_shift(_up2_axis(_up2_axis(z, 3), 2), dy, 2), dx, 3)
    y = y + bias.double().view(1, -1, 1, 1)
    return y if tdt is None else y.to(tdt).double()


@pytest.mark.parametrize("hw", [(8, 16), (16, 32), (8, 48), (1, 1), (3, 2)])
def test_nine_map_identity_equals_interpolate_then_conv(hw):
    """One kernel tile (every border and corner), 2 x 2 tiles (every seam), a non-square 1 x 3, and two tiny maps where every
    pixel is a border pixel, against F.interpolate + F.conv2d in float64, to 1e-12 relative."""
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randn(2, 5, *hw, generator=g, dtype=torch.float64)
    w = torch.randn(4, 5, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    ref = upconv_ref_f64(x, w, b)
    got = upconv_maps_f64(x, w, b)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 1e-12 * ref.abs().max().item()


def test_up2_axis_is_interpolate():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(1, 2, 5, 7, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False)
    assert (_up2_axis(_up2_axis(z, 3), 2) - ref).abs().max().item() < 1e-14


@pytest.mark.parametrize("tdt,ulp", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)])
def test_rounded_maps_stay_within_the_rounding_budget(tdt, ulp):
    """The emulation with the kernel's rounding points against float64 on the same rounded inputs, C = 128 at the GPU test's
    weight scale: an output is 36 map terms with coefficients summing to at most 9, each map off by at most half an ulp of its
    magnitude, plus the final rounding; |Z| <= zmax and |y| <= ymax bound both."""
    g = torch.Generator().manual_seed(128)
    C = 128
    x = torch.randn(1, C, 8, 16, generator=g).to(tdt).float()
    w = (torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(tdt).float()
    b = torch.randn(C, generator=g) * 0.1
    ref = upconv_ref_f64(x, w, b)
    got = upconv_maps_f64(x, w, b, tdt)
    zmax = torch.einsum("oiuv,bihw->bouvhw", w.double(), x.double()).abs().max().item()
    bound = 9 * ulp * zmax + ulp * ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"{tdt}: emulated max-abs error {err:.3e}, rounding budget {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------ the entry points' refusals (no HIP call is made on these paths)
_OK = dict(dtype=1, inp=True, w=True, out=True, batch=2, Hi=8, Wi=16, C=128, workgroups=0)
_REFUSED = [dict(dtype=0), dict(Hi=12), dict(Wi=24), dict(C=48), dict(batch=0), dict(inp=False), dict(w=False), dict(out=False),
            dict(workgroups=-1)]


@pytest.mark.parametrize("bad", _REFUSED, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_upmaps_entry_points_refuse_before_any_launch(bad):
    """llie_conv3x3_upmaps and llie_conv3x3_upmaps_grid answer an error for a dtype the kernel does not take, Hi % 8, Wi % 16,
    C % 32, an empty batch, a NULL input, weight or output pointer and (the _grid call) a negative workgroup count; every check
    sits in front of the first HIP call, so this runs without a GPU (the pointers are dummies that are never read), and no
    launcher has recorded a kernel name afterwards.  llie_conv3x3_upmaps_supported and llie_conv3x3_upmaps_workgroups give the
    same answer for each shape."""
    native = importlib.import_module("cv-diffusion-model_amd._native")
    L = native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    a = dict(_OK, **bad)
    ptr = lambda on: p if on else None
    before = L.llie_last_kernel()
    assert L.llie_conv3x3_upmaps_supported(_OK["dtype"], _OK["Hi"], _OK["Wi"], _OK["C"]) == 1  # the case the bad ones differ from by one argument
    rc_grid = L.llie_conv3x3_upmaps_grid(a["dtype"], ptr(a["inp"]), ptr(a["w"]), p, ptr(a["out"]), p, a["batch"], a["Hi"], a["Wi"], a["C"],
                                         a["workgroups"], None)
    assert rc_grid != 0, a
    if a["workgroups"] < 0:
        assert rc_grid == native.ERR_ARG
    else:  # the call without a count has the same contract
        assert L.llie_conv3x3_upmaps(a["dtype"], ptr(a["inp"]), ptr(a["w"]), p, ptr(a["out"]), p, a["batch"], a["Hi"], a["Wi"], a["C"], None) == rc_grid
    if not (a["inp"] and a["w"] and a["out"]) or a["dtype"] == 0:
        assert rc_grid == native.ERR_ARG
    assert L.llie_last_kernel() == before
    shape_bad = any(k in bad for k in ("dtype", "Hi", "Wi", "C"))
    assert L.llie_conv3x3_upmaps_supported(a["dtype"], a["Hi"], a["Wi"], a["C"]) == (0 if shape_bad else 1)
    if any(k in bad for k in ("Hi", "Wi", "C", "batch")):
        assert L.llie_conv3x3_upmaps_workgroups(a["batch"], a["Hi"], a["Wi"], a["C"]) == native.ERR_ARG
