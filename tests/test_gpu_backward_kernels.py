"""Each backward kernel of the training step (bwd.hip, wgrad.hip) through its own C ABI entry point, against a float64 reference.

Method: every input is drawn in fp32 and rounded to the storage type the kernel reads; the reference is computed in float64 from
exactly those values and mirrors each rounding the kernel does (the weight-gradient prologue rounds act(x * scale + shift) to the
compute type, the depthwise one relu6(h * scale + shift), the GroupNorm mask stores dz in the compute type) and nothing else.

Tolerance: what remains is fp32 accumulation, so the bar of an output entry is BAR * 2^-24 * (the absolute sum of that entry's
terms, as the kernel forms them, computed in the reference), plus one ulp of the storage type for outputs stored in it.  Where a
value the kernel rounds to a 2-byte type lies so close to a rounding midpoint that the kernel's fp32 arithmetic (fused multiply-add,
__expf) may round it the other way, the bar also admits that one-ulp flip (`_flip_slack`).  Each test's docstring records the worst
measured ratio |err| / (2^-24 * abs sum) on the MI355X; the bars are about 10x that, and never looser than 1e-4 of the abs sum.

Every output is filled with NaN first (entries the kernel never writes show up), strided outputs carry canary values around the
written window, and every call is made twice and must give the same bits.
"""
import ctypes
import importlib
import math
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_refs import TDT, U, _flip_slack, _r64, _ratio, _rt, _ulp  # noqa: E402  (the comparison helpers: one copy)

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

CANARY = 12345.5
DTYPES = [0, 1, 2]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _act64(z, act):
    if act == 1:
        return z.clamp(0.0, 6.0)
    if act == 2:
        return z * torch.sigmoid(z)
    return z


# =============================================================================================
# llie_wgrad: weight gradient of 1x1 and 3x3 convolutions (wgrad.hip)
# Bars in multiples of 2^-24 x the absolute sum; the worst ratios measured on the MI355X over all shapes are noted beside them.
WGRAD_BAR = 48.0  # measured worst: 5.92 fp32, 1.55 fp16, 1.84 bf16


class WgCase:
    def __init__(self, name, N, segs, B, Ho, Wo, Hi=None, Wi=None, stride=1, ntap=1, dy=0, dx=0, nstore=0, kstore=0, ms=(0,)):
        self.name, self.N, self.segs, self.B, self.Ho, self.Wo = name, N, segs, B, Ho, Wo
        self.Hi, self.Wi = Hi or Ho, Wi or Wo
        self.stride, self.ntap, self.dy, self.dx, self.nstore, self.kstore, self.ms = stride, ntap, dy, dx, nstore, kstore, ms


# segs: (channels, act, affine) with affine 0 = none, 1 = scale only (shift null), 2 = scale and shift
WG_CASES = [
    WgCase("pw32x32_p16", 32, [(32, 0, 0)], 1, 16, 16, ms=(0, 1)),
    WgCase("pw64x96_p32_b3_nseg2", 64, [(64, 1, 2), (32, 2, 1)], 3, 32, 32, ms=(0, 1, 24, 5)),
    WgCase("pw128x96_p9_b3_nseg3", 128, [(32, 2, 2), (32, 0, 1), (32, 1, 2)], 3, 9, 9, ms=(0, 1, "ragged")),
    WgCase("pw256x160_p25", 256, [(128, 1, 2), (32, 2, 2)], 1, 25, 25, ms=(0, 1, "ragged")),
    WgCase("pw96x192_p18_b3", 96, [(192, 2, 2)], 3, 18, 18, ms=(0, "ragged", 18)),
    WgCase("pw128x96_p36", 128, [(96, 1, 2)], 1, 36, 36, ms=(0, "ragged")),
    WgCase("pw256x160_p50_b3", 256, [(160, 2, 2)], 3, 50, 50, ms=(0, 1, "ragged")),
    WgCase("pw64x96_p32_b3_reduce2", 64, [(96, 0, 2)], 3, 32, 32, ms=(48, 17)),
    WgCase("c3_64_s1_p16_b3", 64, [(64, 0, 0)], 3, 16, 16, ntap=9, ms=(0, 1)),
    WgCase("c3_128_s1_p16", 128, [(128, 0, 0)], 1, 16, 16, ntap=9, ms=(0, 1)),
    WgCase("c3_64_s2_hi18_b3", 64, [(64, 0, 0)], 3, 9, 9, Hi=18, Wi=18, stride=2, ntap=9, ms=(0, "ragged")),
    WgCase("c3_128_s2_hi32", 128, [(128, 0, 0)], 2, 16, 16, Hi=32, Wi=32, stride=2, ntap=9, ms=(0,)),
    WgCase("tap_s2_dy1_dxm1", 64, [(64, 0, 0)], 3, 9, 9, Hi=18, Wi=18, stride=2, ntap=1, dy=1, dx=-1, ms=(0,)),
    WgCase("head_n32_nstore3", 32, [(64, 2, 2)], 3, 16, 16, ntap=9, nstore=3, ms=(0, 1)),
    WgCase("input_k32_kstore6", 64, [(32, 0, 0)], 3, 16, 16, ntap=9, kstore=6, ms=(0, 1)),
]


def _wg_inputs(c, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    B, P, Pi = c.B, c.Ho * c.Wo, c.Hi * c.Wi
    gr = _rt(torch.randn(B * P, c.N, generator=g), dtype)
    K = sum(s[0] for s in c.segs)
    xs, tabs = [], []
    for ch, act, aff in c.segs:
        xs.append(_rt(torch.randn(B * Pi, ch, generator=g) * 1.5, dtype))
        sc = (torch.rand(B, ch, generator=g) + 0.5) if aff else None
        sh = (torch.randn(B, ch, generator=g) * 0.7) if aff == 2 else None
        tabs.append((sc, sh))
    return gr, xs, tabs, K


def _wg_reference(c, dtype, gr, xs, tabs):
    """-> ref [ntap][N][K], abssum, slack (float64) for the kernel's operands: A' = round_T(act(fma(x, scale, shift)))."""
    B, P = c.B, c.Ho * c.Wo
    cols, slacks = [], []
    for (ch, act, aff), x, (sc, sh) in zip(c.segs, xs, tabs):
        z = x.double().view(B, -1, ch)
        if aff:
            z = z * sc.double()[:, None, :] + (sh.double()[:, None, :] if sh is not None else 0.0)
            z = z.float().double()                         # one fp32 rounding (fused multiply-add)
        v = _act64(z, act)
        if act == 2 or aff:
            a = _r64(v, dtype)
            sl = _flip_slack(v, dtype) if dtype else (v.abs() * 2.0 ** -21 if act == 2 else torch.zeros_like(v))
        else:
            a, sl = v, torch.zeros_like(v)
        cols.append(a)
        slacks.append(sl)
    A = torch.cat(cols, -1).view(B, c.Hi, c.Wi, -1)        # [B][Hi][Wi][K]
    S = torch.cat(slacks, -1).view(B, c.Hi, c.Wi, -1)
    taps = [(t // 3 - 1, t % 3 - 1) for t in range(9)] if c.ntap == 9 else [(c.dy, c.dx)]
    G = gr.double().view(B * P, c.N)
    ys = torch.arange(c.Ho) * c.stride
    xs_ = torch.arange(c.Wo) * c.stride
    ref, absr, slk = [], [], []
    for ty, tx in taps:
        yy, xx = ys + ty, xs_ + tx
        oky, okx = (yy >= 0) & (yy < c.Hi), (xx >= 0) & (xx < c.Wi)
        Ag = A[:, yy.clamp(0, c.Hi - 1)][:, :, xx.clamp(0, c.Wi - 1)]
        Sg = S[:, yy.clamp(0, c.Hi - 1)][:, :, xx.clamp(0, c.Wi - 1)]
        m = (oky[:, None] & okx[None, :]).double()[None, :, :, None]
        Ag, Sg = (Ag * m).reshape(B * P, -1), (Sg * m).reshape(B * P, -1)
        ref.append(G.t() @ Ag)
        absr.append(G.abs().t() @ Ag.abs())
        slk.append(G.abs().t() @ Sg)
    return torch.stack(ref), torch.stack(absr), torch.stack(slk)


def _wg_run(dev, c, dtype, gd, xd, tabd, K, ms):
    L = N.lib()
    nst, kst = c.nstore or c.N, c.kstore or K
    # strided destination with canaries: rows of ldn floats (a gap after each row), 3 floats before the window
    if c.ntap == 9:
        ldk, ldn = 9, kst * 9 + 7
    else:
        ldk, ldn = 1, K + 5
    off = 3
    total = off + nst * ldn + 11
    out = torch.full((total,), CANARY, device=dev)
    win = torch.zeros(total, dtype=torch.bool)
    idx = (off + torch.arange(nst)[:, None, None] * ldn + torch.arange(kst)[None, :, None] * ldk
           + torch.arange(c.ntap)[None, None, :]).flatten()
    win[idx] = True
    out[win.to(dev)] = float("nan")
    arr = (N.GemmSeg * len(c.segs))()
    for i, ((ch, act, aff), x, (sc, sh)) in enumerate(zip(c.segs, xd, tabd)):
        arr[i] = N.GemmSeg(x.data_ptr(), ch, sc.data_ptr() if sc is not None else None, sh.data_ptr() if sh is not None else None,
                           ch, act)
    msv = ms
    if ms == "ragged":
        msv = int(L.llie_wgrad_msplit(dtype, c.B, c.Ho * c.Wo, c.N, K, c.ntap, 1))
    eff = msv or int(L.llie_wgrad_msplit(dtype, c.B, c.Ho * c.Wo, c.N, K, c.ntap, int((c.Ho * c.Wo) % 64 != 0)))
    pf = int(L.llie_wgrad_partial_floats(eff, c.N, K, c.ntap))
    part = torch.full((pf,), float("nan"), device=dev)
    N.check(L.llie_wgrad(dtype, gd.data_ptr(), c.N, arr, len(c.segs), c.B, c.Ho, c.Wo, c.Hi, c.Wi, c.stride, c.dy, c.dx, c.ntap,
                         c.nstore, c.kstore, part.data_ptr(), pf, out.data_ptr(), ldn, ldk, off, msv, _st()), "wgrad")
    torch.cuda.synchronize()
    o = out.cpu()
    assert (o[~win] == CANARY).all(), "wgrad wrote outside its nstore / kstore window"
    res = o[off:off + nst * ldn].view(nst, ldn)[:, :kst * ldk].reshape(nst, kst, ldk)[:, :, :c.ntap]  # [n][k][tap]
    return res.permute(2, 0, 1).contiguous(), eff


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", WG_CASES, ids=[c.name for c in WG_CASES])
def test_wgrad_vs_float64(dev, case, dtype):
    """llie_wgrad at every tile shape (64 and, 2-byte with N >= 128 and K > 64, 128), K and N tails, ragged maps (9^2 .. 50^2),
    1-3 segments with per-image affines (some without shift) and none / ReLU6 / SiLU, 3x3 (9 taps) at stride 1 and 2 (ragged output
    from Hi = 18), one off-centre tap, the head (nstore 3) and input-conv (kstore 6) windows, and row splits: the engine's rule,
    1, the ragged rule (splits that do not divide the chunks), a non-dividing count on a 64-multiple map, and more than 16 splits
    under 32 768 outputs (the two-stage reduce).  The engine's split and a single split agree within the summation bound.
    Measured worst ratio (MI355X) over all shapes and splits: 5.92 fp32, 1.55 fp16, 1.84 bf16; bar WGRAD_BAR = 48."""
    c = case
    gr, xs, tabs, K = _wg_inputs(c, dtype, seed=zlib.crc32(c.name.encode()) % 10000 + dtype)
    ref, absr, slk = _wg_reference(c, dtype, gr, xs, tabs)
    nst, kst = c.nstore or c.N, c.kstore or K
    ref, absr, slk = ref[:, :nst, :kst], absr[:, :nst, :kst], slk[:, :nst, :kst]
    slack = slk + _ulp(ref, 0)  # stored fp32: one ulp
    gd, xd = gr.to(dev), [x.to(dev) for x in xs]
    tabd = [(sc.to(dev) if sc is not None else None, sh.to(dev) if sh is not None else None) for sc, sh in tabs]
    outs = {}
    for ms in c.ms:
        o1, eff = _wg_run(dev, c, dtype, gd, xd, tabd, K, ms)
        o2, _ = _wg_run(dev, c, dtype, gd, xd, tabd, K, ms)
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)), f"msplit {ms}: two calls differ"
        _ratio(o1, ref, absr, slack, WGRAD_BAR, f"wgrad/{c.name}/dt{dtype}/ms{ms}={eff}")
        outs[ms] = o1
    if 0 in outs and 1 in outs:
        _ratio(outs[0], outs[1].double(), absr, 2 * slack, 2 * WGRAD_BAR, f"wgrad/{c.name}/dt{dtype}/engine-vs-1")


def test_wgrad_msplit_rules_reach_the_branches():
    """The shapes above reach what they claim: the ragged rule leaves a shorter last split (18 and 21 chunks), and the forced
    counts give more than 16 splits under 32 768 outputs (the two-stage reduce)."""
    L = N.lib()
    for dtype in DTYPES:
        for B, P, n, k in ((3, 18 * 18, 96, 192), (1, 36 * 36, 128, 96)):
            chunks = B * math.ceil(P / 64)
            ms = int(L.llie_wgrad_msplit(dtype, B, P, n, k, 1, 1))
            assert ms > 1 and chunks % math.ceil(chunks / ms) != 0, (dtype, B, P, ms)
    assert 64 * 96 < 32768 and 96 * 192 < 32768


# =============================================================================================
# llie_dw_wgrad: depthwise 3x3 weight gradient (bwd.hip)
DW_BAR = 20.0  # measured worst: 1.99 fp32, 1.21 fp16, 1.18 bf16
DW_CASES = [  # (B, H, W, C); C % 64 for the 2-byte dtypes
    (1, 16, 32, 64), (3, 40, 16, 192), (3, 9, 8, 64), (3, 40, 25, 64), (1, 9, 9, 192), (3, 16, 9, 64), (3, 40, 32, 64),
    (1, 40, 8, 192),
]
DW_PARAMS = [(d, c) for d in DTYPES for c in DW_CASES] + [(0, (3, 40, 32, 32)), (0, (1, 9, 25, 32))]


@pytest.mark.parametrize("dtype,case", DW_PARAMS, ids=[f"dt{d}-{'x'.join(map(str, c))}" for d, c in DW_PARAMS])
def test_dw_wgrad_vs_float64(dev, dtype, case):
    """llie_dw_wgrad over TX = 32 / 16 / 8 and the ragged W (9, 25), partial 32-row strips (H = 9, 40), CC = 32 (fp32) / 64, and
    B * strips > 16 (the grouped partial reduce).  dh2 = g * gs + gb in fp32, a2 = relu6(h * scale + shift) rounded to T.
    Measured worst ratio (MI355X): 1.99 fp32, 1.21 fp16, 1.18 bf16; bar DW_BAR = 20."""
    B, H, W, C = case
    L = N.lib()
    g = torch.Generator().manual_seed(B * 1000 + H * 37 + W * 3 + C + dtype)
    gr = _rt(torch.randn(B, H, W, C, generator=g), dtype)
    h = _rt(torch.randn(B, H, W, C, generator=g) * 2, dtype)
    gs, gb = torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g) * 0.3
    sc, sh = torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g) + 1.0
    dh2 = (gr.double() * gs.double()[:, None, None, :] + gb.double()[:, None, None, :]).float().double()
    v = (h.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]).float().double().clamp(0, 6)
    a2 = _r64(v, dtype)
    sl = _flip_slack(v, dtype)
    a2p, slp = F.pad(a2.permute(0, 3, 1, 2), (1, 1, 1, 1)), F.pad(sl.permute(0, 3, 1, 2), (1, 1, 1, 1))
    d = dh2.permute(0, 3, 1, 2)
    ref, absr, slk = (torch.zeros(C, 9, dtype=torch.float64) for _ in range(3))
    for t in range(9):
        ky, kx = t // 3, t % 3
        win, wsl = a2p[:, :, ky:ky + H, kx:kx + W], slp[:, :, ky:ky + H, kx:kx + W]
        ref[:, t] = (d * win).sum((0, 2, 3))
        absr[:, t] = (d.abs() * win.abs()).sum((0, 2, 3))
        slk[:, t] = (d.abs() * wsl).sum((0, 2, 3))
    dd = [t.to(dev) for t in (gr, h, gs, gb, sc, sh)]
    strips = int(L.llie_dw_wgrad_strips(H, W))
    outs = []
    for _ in range(2):
        part = torch.full((B * strips * 9 * C,), float("nan"), device=dev)
        out = torch.full((C * 9 + 16,), float("nan"), device=dev)
        out[C * 9:] = CANARY
        N.check(L.llie_dw_wgrad(dtype, dd[0].data_ptr(), dd[2].data_ptr(), dd[3].data_ptr(), dd[1].data_ptr(), dd[4].data_ptr(),
                                dd[5].data_ptr(), part.data_ptr(), out.data_ptr(), B, H, W, C, _st()), "dw_wgrad")
        torch.cuda.synchronize()
        o = out.cpu()
        assert (o[C * 9:] == CANARY).all()
        outs.append(o[:C * 9].view(C, 9))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    _ratio(outs[0], ref, absr, slk + _ulp(ref, 0), DW_BAR, f"dw_wgrad/dt{dtype}/{B}x{H}x{W}x{C}")


# =============================================================================================
# llie_groupnorm_backward: one norm site (mask + reduce, coefficients, parameter gradients, apply)
GN_BAR = 20.0  # measured worst (dgamma / dbeta / ds / df / dx): 2.03 fp32, 1.85 fp16, 1.11 bf16
GN_CASES = [  # (name, c0, c1, P, B, act, film, add0, add1, alias)
    ("c32_p64_none", 32, 0, 64, 1, 0, False, False, False, False),
    ("c96cat_p81_relu6_film_add", 64, 32, 81, 3, 1, True, True, True, True),
    ("c96cat_p1296_silu_add1", 64, 32, 1296, 3, 2, False, False, True, False),
    ("c2048_p64_relu6_film", 2048, 0, 64, 3, 1, True, True, False, True),
    ("c2112_p81_silu_film_slab_reduce", 2112, 0, 81, 3, 2, True, False, True, False),
    ("c2112_p64_none_add0", 2112, 0, 64, 1, 0, False, True, False, False),
    ("c32_p1296_silu_film_b3", 32, 0, 1296, 3, 2, True, True, True, True),
    ("c96cat_p64_none_film", 64, 32, 64, 1, 0, True, False, False, False),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_groupnorm_backward_vs_float64_autograd(dev, case, dtype):
    """llie_groupnorm_backward (the engine's norm-site sequence) against float64 autograd of act((xhat * gamma + beta) * (1 + s) + f),
    32 groups, w.r.t. x, gamma, beta, s and f: C = 32, 96 as a 64 + 32 concat, 2048 (tile sums in the coefficient kernel) and 2112
    (slab_reduce), each act, FiLM on / off, add0 / add1 on / off, P in {64, 81, 1296}, B in {1, 3}.  dz (stored in T) is checked on
    its own first; the rest of the reference then takes the kernel's dz, the values every later stage reads.  Absolute sums follow
    the kernel's algebra: dG = rstd (sum dz x - mean sum dz).  Measured worst ratio (MI355X), over dgamma / dbeta / ds / df / dx:
    2.03 fp32, 1.85 fp16, 1.11 bf16; bar GN_BAR = 20."""
    name, c0, c1, P, B, act, film, add0, add1, alias = case
    L = N.lib()
    C, T = c0 + c1, TDT[dtype]
    cg = C // 32
    g = torch.Generator().manual_seed(C * 7 + P + B + act * 3 + dtype)
    x = _rt(torch.randn(B, P, C, generator=g) * 1.3 + 0.4, dtype)
    gin = _rt(torch.randn(B, P, C, generator=g), dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    s = torch.randn(B, C, generator=g) * 0.3 if film else torch.zeros(B, C)
    f = torch.randn(B, C, generator=g) * 0.3 if film else torch.zeros(B, C)
    a0 = _rt(torch.randn(B, P, C, generator=g), dtype) if add0 else None
    a1 = _rt(torch.randn(B, P, C, generator=g), dtype) if add1 else None
    # forward record in fp32 (what llie_groupnorm_finalize leaves): mean / rstd per group, the affine scale / shift
    xg = x.double().view(B, P, 32, cg)
    mean64 = xg.mean((1, 3))
    var64 = xg.var((1, 3), unbiased=False)
    mean_f, rstd_f = mean64.float(), (1.0 / torch.sqrt(var64 + 1e-5)).float()
    rc = lambda t: t.repeat_interleave(cg, dim=1)  # noqa: E731  [B][32] -> [B][C]
    G_f = (gamma[None, :].double() * (1 + s.double())).float()
    scale = (rc(rstd_f).double() * G_f.double()).float()
    shift = ((beta[None, :].double() - rc(mean_f).double() * rc(rstd_f).double() * gamma[None, :].double()) * (1 + s.double())
             + f.double()).float()
    # dz = g * act'(z), z = fma(x, scale, shift) in fp32, stored in T
    z = (x.double() * scale.double()[:, None, :] + shift.double()[:, None, :]).float().double()
    if act == 1:
        dz_ex = gin.double() * ((z > 0) & (z < 6)).double()
    elif act == 2:
        sg = torch.sigmoid(z)
        dz_ex = gin.double() * sg * (1 + z * (1 - sg))
    else:
        dz_ex = gin.double()
    # device buffers
    d = lambda t: t.contiguous().to(dev) if t is not None else None  # noqa: E731
    xd0, xd1 = d(x[:, :, :c0]), d(x[:, :, c0:]) if c1 else None
    filmt = torch.full((B, 2 * C + 6), CANARY)
    filmt[:, :C], filmt[:, C:2 * C] = s, f
    args_common = dict(mean=d(mean_f), rstd=d(rstd_f), gamma=d(gamma), beta=d(beta), scale=d(scale), shift=d(shift),
                       film=d(filmt) if film else None)
    a1_0, a1_1 = (d(a1[:, :, :c0]), d(a1[:, :, c0:]) if c1 else None) if add1 else (None, None)
    a0d = d(a0)
    nscr = int(L.llie_groupnorm_backward_scratch_floats(B, C, P))
    results = []
    for _ in range(2):
        gd = d(gin)
        dzd = gd if alias else torch.full_like(gd, float("nan"))
        dx0 = torch.full((B, P, c0), float("nan"), dtype=T, device=dev)
        dx1 = torch.full((B, P, c1), float("nan"), dtype=T, device=dev) if c1 else None
        dgam = torch.full((C + 8,), CANARY, device=dev)
        dbet = torch.full((C + 8,), CANARY, device=dev)
        dgam[:C], dbet[:C] = float("nan"), float("nan")
        dfl = torch.full((B, 2 * C + 6), CANARY, device=dev)
        if film:
            dfl[:, :2 * C] = float("nan")
        scr = torch.full((nscr,), float("nan"), device=dev)
        A = N.GnBackwardArgs()
        A.g, A.dz = gd.data_ptr(), (dzd.data_ptr() if act else None)
        A.x0, A.x1, A.c0, A.c1 = xd0.data_ptr(), xd1.data_ptr() if c1 else None, c0, c1
        A.scale, A.shift, A.act = args_common["scale"].data_ptr(), args_common["shift"].data_ptr(), act
        A.mean, A.rstd = args_common["mean"].data_ptr(), args_common["rstd"].data_ptr()
        A.gamma, A.beta = args_common["gamma"].data_ptr(), args_common["beta"].data_ptr()
        A.film, A.film_stride = (args_common["film"].data_ptr(), 2 * C + 6) if film else (None, 0)
        A.dfilm, A.dfilm_stride = (dfl.data_ptr(), 2 * C + 6) if film else (None, 0)
        A.dgamma, A.dbeta = dgam.data_ptr(), dbet.data_ptr()
        A.add0 = a0d.data_ptr() if add0 else None
        A.add1_0, A.add1_1 = (a1_0.data_ptr(), a1_1.data_ptr() if c1 else None) if add1 else (None, None)
        A.dx0, A.dx1, A.batch, A.pixels = dx0.data_ptr(), dx1.data_ptr() if c1 else None, B, P
        N.check(L.llie_groupnorm_backward(dtype, ctypes.byref(A), scr.data_ptr(), nscr, _st()), "groupnorm_backward")
        torch.cuda.synchronize()
        dxk = torch.cat([dx0.cpu(), dx1.cpu()], -1) if c1 else dx0.cpu()
        r = dict(dx=dxk, dgamma=dgam.cpu(), dbeta=dbet.cpu(), dfilm=dfl.cpu(), dz=dzd.cpu() if act else None)
        results.append(r)
    for k in ("dx", "dgamma", "dbeta", "dfilm") + (("dz",) if act else ()):
        a, b = results[0][k], results[1][k]
        assert torch.equal(a.float().view(torch.int32), b.float().view(torch.int32)), f"{k}: two calls differ"
    res = results[0]
    assert (res["dgamma"][C:] == CANARY).all() and (res["dbeta"][C:] == CANARY).all() and (res["dfilm"][:, 2 * C:] == CANARY).all()
    if not film:
        assert (res["dfilm"] == CANARY).all()
    # (1) dz against round_T(g * act'(z)): equal except where rounding or the ReLU6 edges are ambiguous (one ulp there)
    if act:
        dzk = res["dz"].double()
        ref_dz = _r64(dz_ex, dtype)
        # fp32 error of g * sg (1 + z (1 - sg)) with __expf: absolute, |g| 2^-20 (1 + |z|) -- the bracket cancels near z = -1.28, so
        # there the error spans several ulps of the tiny dz (measured: 3 bf16 ulps at dz = 6e-8, g = 0.05)
        e32 = gin.double().abs() * 2.0 ** -20 * (1 + z.abs()) if act == 2 else torch.zeros_like(z)
        amb = _flip_slack(dz_ex, dtype, e32 + dz_ex.abs() * 2.0 ** -18) if dtype else e32
        edge = ((z.abs() < 1e-4) | ((z - 6).abs() < 1e-4)) if act == 1 else torch.zeros_like(z, dtype=torch.bool)
        bad = ((dzk - ref_dz).abs() > amb) & ~edge
        if bad.any():
            at = bad.nonzero()[:4].t().tolist()
            rows = [(z[i, j, k].item(), gin[i, j, k].item(), dzk[i, j, k].item(), ref_dz[i, j, k].item(), dz_ex[i, j, k].item())
                    for i, j, k in zip(*at)]
            raise AssertionError(f"dz: {int(bad.sum())} entries differ beyond the rounding ambiguity; (z, g, kernel, round_T(ref), ref): {rows}")
        dz = dzk
    else:
        dz = gin.double()
    # (2) the rest, float64 autograd with the kernel's dz as the cotangent; the record's fp32 mean / rstd values, the true derivative
    xv = x.double().requires_grad_(True)
    gam, bet = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    sv, fv = s.double().requires_grad_(True), f.double().requires_grad_(True)
    xg = xv.view(B, P, 32, cg)
    m_t, r_t = xg.mean((1, 3)), 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + 1e-5)
    m_v = mean_f.double() + (m_t - m_t.detach())
    r_v = rstd_f.double() + (r_t - r_t.detach())
    xhat = ((xg - m_v[:, None, :, None]) * r_v[:, None, :, None]).view(B, P, C)
    n = (xhat * gam + bet) * (1 + sv[:, None, :]) + fv[:, None, :]
    gx, ggam, gbet, gs_, gf_ = torch.autograd.grad(n, [xv, gam, bet, sv, fv], dz)
    if add0:
        gx = gx + a0.double()
    if add1:
        gx = gx + a1.double()
    # absolute sums of the kernel's terms
    mb, rb = rc(mean_f).double(), rc(rstd_f).double()                       # [B][C]
    S1a, S2a = dz.abs().sum(1), (dz * x.double()).abs().sum(1)              # [B][C]
    dGa = rb * (S2a + mb.abs() * S1a)
    one_s = (1 + s.double()).abs()
    Ga = G_f.double().abs()
    c1a = (Ga * S1a).view(B, 32, cg).sum(-1) / (cg * P)
    c2a = (Ga * dGa).view(B, 32, cg).sum(-1) / (cg * P)
    dxa = (dz.abs() * (rb * Ga)[:, None, :] + (x.double().abs() + mb.abs()[:, None, :]) * (rb * rb * rc(c2a))[:, None, :]
           + (rb * rc(c1a))[:, None, :])
    if add0:
        dxa = dxa + a0.double().abs()
    if add1:
        dxa = dxa + a1.double().abs()
    tag = f"gn/{name}/dt{dtype}"
    _ratio(res["dgamma"][:C], ggam, (one_s * dGa).sum(0), _ulp(ggam, 0), GN_BAR, tag + "/dgamma")
    _ratio(res["dbeta"][:C], gbet, (one_s * S1a).sum(0), _ulp(gbet, 0), GN_BAR, tag + "/dbeta")
    if film:
        _ratio(res["dfilm"][:, :C], gs_, gamma.double().abs() * dGa + beta.double().abs() * S1a, _ulp(gs_, 0), GN_BAR, tag + "/ds")
        _ratio(res["dfilm"][:, C:2 * C], gf_, S1a, _ulp(gf_, 0), GN_BAR, tag + "/df")
    _ratio(res["dx"], gx, dxa, _ulp(gx, dtype), GN_BAR, tag + "/dx")


# =============================================================================================
# llie_linattn_backward (both passes and the partial reduce between them)
LA_BAR = 7.5  # measured worst: 0.74 fp32, 0 fp16 (within the one ulp of the stored value), 0.12 bf16
LA_CASES = [(64, 1, 2), (81, 4, 2), (256, 8, 1), (324, 4, 2), (1296, 8, 2), (1296, 1, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,heads,B", LA_CASES)
def test_linattn_backward_vs_float64_autograd(dev, n, heads, B, dtype):
    """llie_linattn_backward against float64 autograd of the forward restatement of test_linattn_entry_point_vs_torch
    (phi = elu + 1), for N in {64, 81, 256, 324, 1296} (81 and 324: a partly-empty last tile) and 1 / 4 / 8 heads.  kv: what
    llie_linattn leaves in its scratch.  The absolute sums propagate |.| through the same expression tree (den > 0).
    Measured worst ratio (MI355X): 0.74 fp32, 0 fp16, 0.12 bf16; bar LA_BAR = 7.5."""
    L = N.lib()
    T, inner = TDT[dtype], heads * 32
    g = torch.Generator().manual_seed(n * 13 + heads + B + dtype)
    qkv = _rt(torch.randn(B, n, 3 * inner, generator=g) * 0.8, dtype)
    dout = _rt(torch.randn(B, n, inner, generator=g), dtype)
    qd, dod = qkv.to(dev), dout.to(dev)
    kv = torch.full((int(L.llie_linattn_splits(n)) * B * heads * 32 * 33,), float("nan"), device=dev)
    fo = torch.empty(B, n, inner, dtype=T, device=dev)
    N.check(L.llie_linattn(dtype, qd.data_ptr(), kv.data_ptr(), fo.data_ptr(), B, n, heads, _st()), "linattn")
    nd = int(L.llie_linattn_dkv_floats(B, n, heads))
    outs = []
    for _ in range(2):
        dkv = torch.full((nd,), float("nan"), device=dev)
        dq = torch.full((B, n, 3 * inner), float("nan"), dtype=T, device=dev)
        N.check(L.llie_linattn_backward(dtype, qd.data_ptr(), kv.data_ptr(), dod.data_ptr(), dq.data_ptr(), dkv.data_ptr(), nd, B, n,
                                        heads, _st()), "linattn_backward")
        torch.cuda.synchronize()
        outs.append(dq.cpu())
    assert torch.equal(outs[0].float().view(torch.int32), outs[1].float().view(torch.int32))
    # reference
    x = qkv.double().requires_grad_(True)
    q, k, v = (zz.view(B, n, heads, 32).permute(0, 2, 3, 1) for zz in x.split(inner, dim=2))  # [b][h][d][n]
    Q, K = F.elu(q) + 1, F.elu(k) + 1
    kvr = torch.einsum("bhdn,bhen->bhde", K, v)
    num = torch.einsum("bhdn,bhde->bhen", Q, kvr)
    den = torch.einsum("bhdn,bhd->bhn", Q, K.sum(-1))[:, :, None, :] + 1e-6
    out = (num / den).permute(0, 3, 1, 2).reshape(B, n, inner)
    (ref,) = torch.autograd.grad(out, [x], dout.double())
    # absolute sums through the same tree
    with torch.no_grad():
        Q, K, V = Q.detach(), K.detach(), v.detach().abs()
        do = dout.double().view(B, n, heads, 32).permute(0, 2, 3, 1).abs()      # [b][h][e][n]
        kvA, ks = torch.einsum("bhdn,bhen->bhde", K, V), K.sum(-1)
        kvv = kvr.detach()
        denv = den.detach()[:, :, 0, :]                                            # [b][h][n]
        numA = torch.einsum("bhdn,bhde->bhen", Q, kvA)
        outv = (num.detach() / den.detach())
        dn, dnA = do / denv[:, :, None, :], 2 * do / denv[:, :, None, :]
        outA = numA / denv[:, :, None, :] + outv.abs()
        ddA = (dnA * outv.abs() + dn * outA).sum(2)                               # [b][h][n]
        dd = (dn * outv.abs()).sum(2)
        dQA = ddA[:, :, None, :] * ks[..., None] + dd[:, :, None, :] * ks[..., None] + torch.einsum("bhen,bhde->bhdn", dnA, kvv.abs()) \
            + torch.einsum("bhen,bhde->bhdn", dn, kvA)
        dkvA = torch.einsum("bhdn,bhen->bhde", Q, dnA)
        dksA = torch.einsum("bhdn,bhn->bhd", Q, ddA)
        dKA = torch.einsum("bhen,bhde->bhdn", V, dkvA) + dksA[..., None]
        dVA = torch.einsum("bhdn,bhde->bhen", K, dkvA)
        dphq = torch.where(q.detach() > 0, 1.0, Q)
        dphk = torch.where(k.detach() > 0, 1.0, K)
        to_rows = lambda t: t.permute(0, 3, 1, 2).reshape(B, n, inner)  # noqa: E731
        absr = torch.cat([to_rows(dQA * dphq), to_rows(dKA * dphk), to_rows(dVA)], -1)
    _ratio(outs[0], ref, absr, _ulp(ref, dtype), LA_BAR, f"linattn_bwd/n{n}/h{heads}/b{B}/dt{dtype}")


# =============================================================================================
# bilinear x2 adjoint and the stride-2 dilation
UP_BAR = 20.0  # measured worst: 1.99 fp32, 0 fp16 / bf16 (within the one ulp of the stored value)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hi", [4, 9, 25])
def test_upsample2x_backward_and_dilate2x(dev, hi, dtype):
    """llie_upsample2x_backward against float64 autograd of F.interpolate(bilinear, align_corners=False) and the adjoint identity
    <up x, y> = <x, up* y>; llie_dilate2x bit-exact.  Hi = Wi in {4, 9, 25}.  Measured worst ratio (MI355X): 1.99 fp32, 0 fp16 /
    bf16 (inside the one ulp of the stored value); bar UP_BAR = 20."""
    L = N.lib()
    T, B, Cc = TDT[dtype], 2, 32
    g = torch.Generator().manual_seed(hi * 5 + dtype)
    dy = _rt(torch.randn(B, 2 * hi, 2 * hi, Cc, generator=g), dtype)
    dyd = dy.to(dev)
    outs = []
    for _ in range(2):
        din = torch.full((B, hi, hi, Cc), float("nan"), dtype=T, device=dev)
        N.check(L.llie_upsample2x_backward(dtype, dyd.data_ptr(), din.data_ptr(), B, hi, hi, Cc, _st()), "upsample2x_backward")
        torch.cuda.synchronize()
        outs.append(din.cpu())
    assert torch.equal(outs[0].float().view(torch.int32), outs[1].float().view(torch.int32))
    x = torch.zeros(B, Cc, hi, hi, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    (ref,) = torch.autograd.grad(up, [x], dy.double().permute(0, 3, 1, 2))
    (absr,) = torch.autograd.grad(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), [x],
                                  dy.double().abs().permute(0, 3, 1, 2))
    ref, absr = ref.permute(0, 2, 3, 1), absr.permute(0, 2, 3, 1)
    _ratio(outs[0], ref, absr, _ulp(ref, dtype), UP_BAR, f"upsample2x_bwd/hi{hi}/dt{dtype}")
    # adjoint identity with the kernel's up* (before its rounding to T the bar would be fp32 only: allow the T rounding)
    xr = torch.randn(B, hi, hi, Cc, generator=g, dtype=torch.float64)
    lhs = (F.interpolate(xr.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
           * dy.double()).sum()
    rhs = (xr * outs[0].double()).sum()
    bound = (xr.abs() * (_ulp(ref, dtype) + UP_BAR * U * absr)).sum()
    assert (lhs - rhs).abs() <= bound, (lhs.item(), rhs.item(), bound.item())
    # dilation: exact
    src = _rt(torch.randn(B, hi, hi, Cc, generator=g), dtype)
    dil = torch.full((B, 2 * hi, 2 * hi, Cc), float("nan"), dtype=T, device=dev)
    N.check(L.llie_dilate2x(dtype, src.to(dev).data_ptr(), dil.data_ptr(), B, hi, hi, Cc, _st()), "dilate2x")
    torch.cuda.synchronize()
    want = torch.zeros(B, 2 * hi, 2 * hi, Cc, dtype=T)
    want[:, ::2, ::2] = src
    assert torch.equal(dil.cpu().float().view(torch.int32), want.float().view(torch.int32))


# =============================================================================================
# the Linears of the SE MLP, FiLM and time embedding: linear_dx (chunked scratch) and linear_dw
LIN_BAR = 12.0  # measured worst: 1.18 / 1.21 / 1.12 (weights fp32 / fp16 / bf16)
FINAL_BAR = 26.0  # measured worst: 2.60 fp32, 0.28 fp16, 0.03 bf16


@pytest.mark.parametrize("wdtype", DTYPES)
@pytest.mark.parametrize("R,Kc,B,stride_pad", [(200, 96, 3, 0), (1000, 128, 3, 40), (4096, 64, 2, 8)])
def test_linear_dx_dw_vs_float64(dev, wdtype, R, Kc, B, stride_pad):
    """llie_linear_dx (R > 256: chunked scratch, linear_dx_chunks(R) > 1) with weights of every dtype, and llie_linear_dw, from a
    dy slice of a wider table (dy_stride > R).  Measured worst ratio (MI355X): 1.18 / 1.21 / 1.12 with fp32 / fp16 / bf16
    weights; bar LIN_BAR = 12."""
    L = N.lib()
    g = torch.Generator().manual_seed(R + Kc + B + wdtype)
    ld = R + stride_pad
    dyt = torch.randn(B, ld, generator=g)
    w = _rt(torch.randn(R, Kc, generator=g) / math.sqrt(R), wdtype)
    x = torch.randn(B, Kc, generator=g)
    dyd, wd, xd = dyt.to(dev), w.to(dev), x.to(dev)
    dy = dyt[:, :R].double()
    ref_dx, abs_dx = dy @ w.double(), dy.abs() @ w.double().abs()
    ref_dw, abs_dw = dy.t() @ x.double(), dy.abs().t() @ x.double().abs()
    ref_db, abs_db = dy.sum(0), dy.abs().sum(0)
    ns = int(L.llie_linear_dx_scratch_floats(B, R, Kc))
    assert (ns > B * Kc) == (R > 256)
    res = []
    for _ in range(2):
        dx = torch.full((B * Kc + 8,), CANARY, device=dev)
        dx[:B * Kc] = float("nan")
        scr = torch.full((ns,), float("nan"), device=dev)
        N.check(L.llie_linear_dx(wdtype, dyd.data_ptr(), ld, wd.data_ptr(), dx.data_ptr(), B, R, Kc, scr.data_ptr(), ns, _st()), "linear_dx")
        dw = torch.full((R * Kc + 8,), CANARY, device=dev)
        db = torch.full((R + 8,), CANARY, device=dev)
        dw[:R * Kc], db[:R] = float("nan"), float("nan")
        N.check(L.llie_linear_dw(dyd.data_ptr(), ld, xd.data_ptr(), dw.data_ptr(), db.data_ptr(), B, R, Kc, _st()), "linear_dw")
        torch.cuda.synchronize()
        res.append((dx.cpu(), dw.cpu(), db.cpu()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    dx, dw, db = res[0]
    assert (dx[B * Kc:] == CANARY).all() and (dw[R * Kc:] == CANARY).all() and (db[R:] == CANARY).all()
    tag = f"linear/R{R}/K{Kc}/wdt{wdtype}"
    _ratio(dx[:B * Kc].view(B, Kc), ref_dx, abs_dx, _ulp(ref_dx, 0), LIN_BAR, tag + "/dx")
    _ratio(dw[:R * Kc].view(R, Kc), ref_dw, abs_dw, _ulp(ref_dw, 0), LIN_BAR, tag + "/dw")
    _ratio(db[:R], ref_db, abs_db, _ulp(ref_db, 0), LIN_BAR, tag + "/db")


# =============================================================================================
# output head: input gradient of the final 3x3 conv
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", [(16, 32), (18, 64)])
def test_final_bwd_data_vs_float64(dev, H, C, dtype):
    """llie_final_bwd_data against float64 autograd of conv2d(a, W, padding=1) w.r.t. a (Cout = 3, weights [9][C][4]).
    Measured worst ratio (MI355X): 2.60 fp32, 0.28 fp16, 0.03 bf16; bar FINAL_BAR = 26."""
    L = N.lib()
    B, Co = 2, 3
    g = torch.Generator().manual_seed(H * C + dtype)
    deps = torch.randn(B, Co, H, H, generator=g)
    W = torch.randn(Co, C, 3, 3, generator=g) / math.sqrt(9 * C)
    wr = torch.zeros(9, C, 4)
    wr[:, :, :Co] = W.permute(2, 3, 1, 0).reshape(9, C, Co)
    a = torch.zeros(B, C, H, H, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(F.conv2d(a, W.double(), padding=1), [a], deps.double())
    (absr,) = torch.autograd.grad(F.conv2d(a, W.double().abs(), padding=1), [a], deps.double().abs())
    ref, absr = ref.permute(0, 2, 3, 1), absr.permute(0, 2, 3, 1)
    dd, wd = deps.to(dev), wr.to(dev)
    outs = []
    for _ in range(2):
        da = torch.full((B, H, H, C), float("nan"), dtype=TDT[dtype], device=dev)
        N.check(L.llie_final_bwd_data(dtype, dd.data_ptr(), wd.data_ptr(), da.data_ptr(), B, H, H, C, Co, _st()), "final_bwd_data")
        torch.cuda.synchronize()
        outs.append(da.cpu())
    assert torch.equal(outs[0].float().view(torch.int32), outs[1].float().view(torch.int32))
    _ratio(outs[0], ref, absr, _ulp(ref, dtype), FINAL_BAR, f"final_bwd_data/H{H}/C{C}/dt{dtype}")
