"""Exact operands and references of expand_dw (irbx.hip), shared by tests/test_gpu_expand_dw_paths.py (on the device) and
tests/test_expand_dw_paths_host.py (on the CPU).

Every value on the way is a small integer, so no step rounds in fp16 or bf16 and the order of no sum matters:

    x          integers in [-3, 3]
    norm1      scale in {+1, -1}, shift in {0, 1}, per image and channel: a' = clamp01(x scale + shift) is 0 or 1
    W1         entries in {-1, 0, 1}, about 20 % non-zero: h1 / 6 = W1 a' is an integer, |.| <= Cin
    norm2      scale in {+1, -1, 2}, shift 0, per image and channel: a = clamp01(scale h1 / 6) is 0 or 1
    6 w        entries in {-1, 0, 1} (w = k / 6: the fp32 product 6 w is within 2^-23 of k and rounds to k in T)
    h2         = dw3x3(a), an integer with |h2| <= 9
    pool       each per-tile partial is an integer with |.| <= 9 * 128 < 2^24: exact in fp32 in any order; the totals are
               2^24 * sum_px h2, exact in int64

The tables differ per image and per channel, so that a kernel indexing the wrong image, chunk or channel cannot give the
reference (the seeded faults of the host file show it).
"""
import ctypes

import torch

TILE_H, TILE_W = 8, 16       # kXT_H, kXT_W: the output tile of the recompute kernels
POOL_FIX = 2 ** 24           # kPoolFixScale


def plan(L, cin, B, H, W, project=0):
    """(tpw, cpw, grid.x, grid.y) from llie_expand_dw_plan; a negative return code is raised as an AssertionError"""
    p = (ctypes.c_int * 4)()
    rc = int(L.llie_expand_dw_plan(cin, B, H, W, project, p))
    assert rc == 0, (rc, cin, B, H, W, project)
    return tuple(p)


def exact_operands(cin, B, H, W, device, seed):
    """the operands above, fp32 / float tensors on `device` (x, w1 hold integers: cast to T without loss)"""
    g = torch.Generator(device=device).manual_seed(seed)
    chid = 4 * cin

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi, shape, generator=g, device=device)

    t = {"x": ri(-3, 4, B, H, W, cin).float(),
         "s1": (ri(0, 2, B, cin) * 2 - 1).float(), "b1": ri(0, 2, B, cin).float(),
         "w1": (ri(-1, 2, chid, cin) * (torch.rand(chid, cin, generator=g, device=device) < 0.2)).float(),
         "s2": torch.tensor([1.0, -1.0, 2.0], device=device)[ri(0, 3, B, chid)], "b2": torch.zeros(B, chid, device=device),
         "k6": ri(-1, 2, 9, chid).float()}
    t["wd"] = t["k6"] / 6.0
    return t


def exact_h2(t, tdt=None, conv_dtype=torch.float32, x=None, s2=None, k6=None):
    """h2 [B][H][W][Chid] (conv_dtype) of the operands: the affine steps and the expand product in float64, the depthwise conv as nine
    shifted adds in conv_dtype.  tdt: round to T at every point where the kernel rounds (a', a, 6 w as the fp32 product, h2).
    x / s2 / k6 replace that operand (the seeded faults of the host file)."""
    x = t["x"] if x is None else x
    s2 = t["s2"] if s2 is None else s2
    rt = (lambda v: v) if tdt is None else (lambda v: v.float().to(tdt).to(v.dtype))
    B, H, W, _ = x.shape
    ap = rt((rt(x).double() * t["s1"].double()[:, None, None, :] + t["b1"].double()[:, None, None, :]).clamp(0, 1))
    acc = ap @ rt(t["w1"]).double().t()                                               # h1 / 6
    a = rt((acc * s2.double()[:, None, None, :] + t["b2"].double()[:, None, None, :] / 6).clamp(0, 1)).to(conv_dtype)
    del ap, acc
    w6 = rt(6.0 * t["wd"]) if k6 is None else k6                                      # fp32 product, as the kernel stages it
    w6 = w6.to(conv_dtype)
    pad = torch.nn.functional.pad(a, (0, 0, 1, 1, 1, 1))
    del a
    h2 = torch.zeros(B, H, W, w6.shape[1], dtype=conv_dtype, device=x.device)
    for tap in range(9):
        h2 += pad[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, :] * w6[tap]
    return rt(h2)


def tile_sums(h2):
    """[B][H][W][C] -> per 8 x 16 tile sums [B][tiles_y][tiles_x][C], float64"""
    B, H, W, C = h2.shape
    return h2.view(B, H // TILE_H, TILE_H, W // TILE_W, TILE_W, C).sum((2, 4), dtype=torch.float64)


def exact_totals(h2):
    """the fixed-point pool totals [B][Chid] int64 of an integral h2"""
    return (h2.sum((1, 2), dtype=torch.float64) * POOL_FIX).round().to(torch.int64)


def assert_exact(h2):
    """the reference is what the docstring promises before anything is compared with it"""
    assert torch.equal(h2, h2.round()) and h2.abs().max().item() <= 9 and h2.abs().max().item() >= 4
    ts = tile_sums(h2)
    assert ts.abs().max().item() < 2 ** 24 and (ts != 0).any()


def runs(tpw, gx, H, W):
    """the runs of tiles [first, last) one image's workgroups take (irbx_tiles): fixed runs of tpw, or tpw = 0: the image's tiles
    split evenly over gx workgroups"""
    n = (H // TILE_H) * (W // TILE_W)
    if tpw > 0:
        return [(f, min(f + tpw, n)) for f in range(0, n, tpw)]
    return [(i * n // gx, (i + 1) * n // gx) for i in range(gx)]
