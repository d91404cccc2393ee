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

The depthwise input gradient, the norm site fed by its slab and the remaining glue of the backward pass (bias gradient, pack_planes,
add_into, the pointwise fp32 kernels, the time embedding) follow at the end of the file; their cases, references and bars stand in
tests/kernel_refs.py, shared with tests/test_backward_refs_host.py, and LLIE_FWD_TEST_SEED (default 0) shifts their seeds: the bars
were measured over seeds 0, 1 and 2.
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
import kernel_refs as R  # noqa: E402
from kernel_refs import NAN, TDT, U, Guarded, _flip_slack, _r64, _ratio, _rt, _same, _slab, _split, _ulp  # noqa: E402  (the comparison helpers: one copy)

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

CANARY = 12345.5
DTYPES = [0, 1, 2]
TNAME = {0: "float", 1: "_Float16", 2: "__bf16"}
SEED0 = int(os.environ.get("LLIE_FWD_TEST_SEED", "0"))  # shifts the seeds of the tests whose bars stand in kernel_refs.py (measured over 0, 1, 2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _last():
    return N.lib().llie_last_kernel().decode()


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


def _rc(t, cg):
    return t.repeat_interleave(cg, dim=1)  # [B][32] -> [B][C]


def _gn_record(x, gamma, beta, s, f):
    """The forward record in fp32 (what llie_groupnorm_finalize leaves) of x [B][P][C] of T: mean / rstd per group, G = gamma (1 + s),
    the affine scale / shift.  -> (mean_f, rstd_f, G_f, scale, shift)"""
    B, P, C = x.shape
    cg = C // 32
    xg = x.double().view(B, P, 32, cg)
    mean64 = xg.mean((1, 3))
    var64 = xg.var((1, 3), unbiased=False)
    mean_f, rstd_f = mean64.float(), (1.0 / torch.sqrt(var64 + 1e-5)).float()
    G_f = (gamma[None, :].double() * (1 + s.double())).float()
    scale = (_rc(rstd_f, cg).double() * G_f.double()).float()
    shift = ((beta[None, :].double() - _rc(mean_f, cg).double() * _rc(rstd_f, cg).double() * gamma[None, :].double()) * (1 + s.double())
             + f.double()).float()
    return mean_f, rstd_f, G_f, scale, shift


def _gn_forward64(x, gamma, beta, s, f, mean_f, rstd_f):
    """n = (xhat gamma + beta) (1 + s) + f in float64 with autograd leaves x, gamma, beta, s, f: the record's fp32 mean / rstd values, the
    true derivative.  -> (n [B][P][C], leaves)"""
    B, P, C = x.shape
    cg = C // 32
    xv = x.double().requires_grad_(True)
    gam, bet = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    sv, fv = s.double().requires_grad_(True), f.double().requires_grad_(True)
    xg = xv.view(B, P, 32, cg)
    m_t, r_t = xg.mean((1, 3)), 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + 1e-5)
    m_v = mean_f.double() + (m_t - m_t.detach())
    r_v = rstd_f.double() + (r_t - r_t.detach())
    xhat = ((xg - m_v[:, None, :, None]) * r_v[:, None, :, None]).view(B, P, C)
    return (xhat * gam + bet) * (1 + sv[:, None, :]) + fv[:, None, :], [xv, gam, bet, sv, fv]


def _gn_abs_sums(dz, x, mean_f, rstd_f, G_f, gamma, beta, s, a0=None, a1=None):
    """Absolute sums of a norm site's outputs from the dz the later stages read, following the kernel's algebra: dG = rstd (sum dz x -
    mean sum dz).  -> dict dgamma / dbeta [C], ds / df [B][C], dx [B][P][C]"""
    B, P, C = x.shape
    cg = C // 32
    mb, rb = _rc(mean_f, cg).double(), _rc(rstd_f, cg).double()             # [B][C]
    S1a, S2a = dz.abs().sum(1), (dz * x.double()).abs().sum(1)              # [B][C]
    dGa = rb * (S2a + mb.abs() * S1a)
    one_s = (1 + s.double()).abs()
    Ga = G_f.double().abs()
    c1a = (Ga * S1a).view(B, 32, cg).sum(-1) / (cg * P)
    c2a = (Ga * dGa).view(B, 32, cg).sum(-1) / (cg * P)
    dxa = (dz.abs() * (rb * Ga)[:, None, :] + (x.double().abs() + mb.abs()[:, None, :]) * (rb * rb * _rc(c2a, cg))[:, None, :]
           + (rb * _rc(c1a, cg))[:, None, :])
    if a0 is not None:
        dxa = dxa + a0.double().abs()
    if a1 is not None:
        dxa = dxa + a1.double().abs()
    return dict(dgamma=(one_s * dGa).sum(0), dbeta=(one_s * S1a).sum(0), ds=gamma.double().abs() * dGa + beta.double().abs() * S1a,
                df=S1a, dx=dxa)


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
    mean_f, rstd_f, G_f, scale, shift = _gn_record(x, gamma, beta, s, f)
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
    n, leaves = _gn_forward64(x, gamma, beta, s, f, mean_f, rstd_f)
    gx, ggam, gbet, gs_, gf_ = torch.autograd.grad(n, leaves, dz)
    if add0:
        gx = gx + a0.double()
    if add1:
        gx = gx + a1.double()
    ab = _gn_abs_sums(dz, x, mean_f, rstd_f, G_f, gamma, beta, s, a0, a1)  # absolute sums of the kernel's terms
    tag = f"gn/{name}/dt{dtype}"
    _ratio(res["dgamma"][:C], ggam, ab["dgamma"], _ulp(ggam, 0), GN_BAR, tag + "/dgamma")
    _ratio(res["dbeta"][:C], gbet, ab["dbeta"], _ulp(gbet, 0), GN_BAR, tag + "/dbeta")
    if film:
        _ratio(res["dfilm"][:, :C], gs_, ab["ds"], _ulp(gs_, 0), GN_BAR, tag + "/ds")
        _ratio(res["dfilm"][:, C:2 * C], gf_, ab["df"], _ulp(gf_, 0), GN_BAR, tag + "/df")
    _ratio(res["dx"], gx, ab["dx"], _ulp(gx, dtype), GN_BAR, tag + "/dx")


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


# =============================================================================================
# llie_dwconv3x3_backward: the depthwise input gradient with its ReLU6 mask and norm-2 partial sums (dwconv.hip, BWD = true).
# Cases, inputs, references and bars (BAR_DW_BWD, BAR_DW_BWD_STATS) stand in kernel_refs.py; tests/test_backward_refs_host.py checks
# without a GPU that the reference is float64 autograd's, that the mask is decided for every case here, and that the bars have teeth.
def _dwb_call(dev, dtype, dd, B, H, W, C):
    """dd: the device tensors (g, gs, gb, flipped taps, bx, bas, bab) -> (dz, slab, tiles per image), every buffer guarded"""
    L = N.lib()
    out = Guarded((B, H, W, C), dev, TDT[dtype])
    nt = int(L.llie_dwconv3x3_tiles(H, W))
    slab = _slab(dev, B, nt, 2, C)
    N.check(L.llie_dwconv3x3_backward(dtype, *[t.data_ptr() for t in dd], out.ptr, slab.ptr, B, H, W, C, _st()), "dwconv3x3_backward")
    torch.cuda.synchronize()
    return out, slab, nt


def _dwb_check(tag, dtype, inp, o, slab, nt, tx):
    ref, ab, sl, unsure = R.dwconv3x3_bwd_ref(dtype, *inp)
    assert R.mask_unsure_ok(unsure, tx), f"{tag}: the reference cannot decide the mask of this case"
    _ratio(o, ref, ab, sl, R.BAR_DW_BWD, f"dw_bwd/{tag}")
    sref, sab, ssl = R.strip_stats2_ref(o, inp[4], tx)
    assert sref.shape[1] == nt
    _ratio(slab, sref, sab, ssl, R.BAR_DW_BWD_STATS, f"dw_bwd_stats/{tag}")


@pytest.mark.parametrize("case", R.DW_BWD_CASES, ids=[f"{c[0]}x{c[1]}-dt{c[4]}-c{c[5]}" for c in R.DW_BWD_CASES])
def test_dwconv3x3_backward_vs_float64(dev, case):
    """llie_dwconv3x3_backward on the forward test's maps (strips 8 / 16 / 32 wide, ragged W and H, ragged H on W = 8 mod 16, non-square
    both ways) plus a four-row last segment (12 x 16), two channel chunks, B = 3 with per-image tables, every dtype: the kernel name with
    its template arguments; dz entry by entry (masked entries must be exact zeros); the slab [B][llie_dwconv3x3_tiles][2][C] entry by
    entry against the sums of the stored dz and of dz * bx over each (8-row segment, strip) tile's pixels inside the map; nothing
    written outside dz and the helper's tile count (canaries); an image alone gives the bits of its row in the batch.
    Measured worst ratio (MI355X, seeds 0..2), dz: 3.25 fp32, 0.24 fp16, 0.00 bf16, bar BAR_DW_BWD = 32; slab: 1.11 / 0.80 / 0.56, bar
    BAR_DW_BWD_STATS = 11."""
    L = N.lib()
    H, W, tx, ragged, dtype, C = case
    B = 3
    inp = R.dw_bwd_case_inputs(case, SEED0)
    dd = [t.to(dev) for t in inp]
    assert int(L.llie_dwconv3x3_strip_rows(dtype, B, H, W, C)) == 8 and int(L.llie_dwconv3x3_strip_rows(dtype, 1, H, W, C)) == 8
    want = f"dwconv3x3_bwd_{'ragged_' if ragged else ''}kernel<{TNAME[dtype]}, {tx}, 4>"
    tag = f"{H}x{W}x{C}/dt{dtype}"
    runs = []
    for _ in range(2):
        out, slab, nt = _dwb_call(dev, dtype, dd, B, H, W, C)
        assert _last() == want, _last()
        runs.append((out.cpu("dw_bwd dz"), _split(slab.cpu("dw_bwd slab"), B, nt, "dw_bwd slab")))
    _same(runs[0][0], runs[1][0], tag + " dz")
    _same(runs[0][1], runs[1][1], tag + " slab")
    o, s = runs[0]
    _dwb_check(tag, dtype, inp, o, s, nt, tx)
    one = [t if t.shape == (9, C) else t[2:3].contiguous() for t in dd]
    out1, slab1, _ = _dwb_call(dev, dtype, one, 1, H, W, C)
    _same(out1.cpu("dw_bwd dz")[0], o[2], tag + " image 2 alone (dz)")
    _same(_split(slab1.cpu("dw_bwd slab"), 1, nt, "dw_bwd slab")[0], s[2], tag + " image 2 alone (slab)")


@pytest.mark.parametrize("H,rows,B,dtype", R.DW_BWD_STRIPS, ids=[f"{h}rows{r}-dt{d}" for h, r, _, d in R.DW_BWD_STRIPS])
def test_dwconv3x3_backward_strip_heights(dev, H, rows, B, dtype):
    """Strips of 16, 32 and 64 rows (W = 8, one channel chunk, B = 1024 made of three distinct images, as test_dwconv3x3_strip_heights):
    the 12-row unroll wraps (up to 66 input rows) and a strip writes slab segments 1 to 7; and a 32-row map in two 16-row strips (B =
    512), where the second strip's segments start at 2.  llie_dwconv3x3_strip_rows must name the height; images 0..2 are checked
    against float64 (dz and slab), every other image must equal its twin bit for bit.  Bars and measured ratios as
    test_dwconv3x3_backward_vs_float64 (worst here: dz 2.40 / 0.11 / 0.00, slab 0.85 / 0.80 / 0.62)."""
    L = N.lib()
    W, C = 8, 32 if dtype == 0 else 64
    assert int(L.llie_dwconv3x3_strip_rows(dtype, B, H, W, C)) == rows
    inp = R.dw_bwd_strip_inputs(H, rows, dtype, SEED0)
    idx = torch.arange(B) % 3
    dd = [(t if t.shape == (9, C) else t[idx].contiguous()).to(dev) for t in inp]
    runs = []
    for _ in range(2):
        out, slab, nt = _dwb_call(dev, dtype, dd, B, H, W, C)
        assert _last() == f"dwconv3x3_bwd_kernel<{TNAME[dtype]}, 8, 4>", _last()
        runs.append((out.cpu("dw_bwd dz"), _split(slab.cpu("dw_bwd slab"), B, nt, "dw_bwd slab")))
    _same(runs[0][0], runs[1][0], "dz")
    _same(runs[0][1], runs[1][1], "slab")
    o, s = runs[0]
    _same(o, o[idx], "an image and its twin (dz)")
    _same(s, s[idx], "an image and its twin (slab)")
    _dwb_check(f"strip{H}rows{rows}/dt{dtype}", dtype, inp, o[:3], s[:3], nt, 8)


def test_dwconv3x3_backward_refusals(dev):
    """NULL tensors, C off the chunk size, sizes < 1, an unknown dtype: LLIE_ERR_ARG before any HIP call; the NaN-filled dz stays NaN."""
    L = N.lib()
    t = torch.zeros(2 * 8 * 8 * 64, device=dev)
    out = torch.full((2 * 8 * 8 * 64,), NAN, device=dev)
    p = t.data_ptr()

    def call(dtype=1, C=64, B=2, H=8, **kw):
        a = dict(g=p, gs=p, gb=p, w=p, bx=p, bas=p, bab=p, dz=out.data_ptr(), slab=p)
        a.update(kw)
        return L.llie_dwconv3x3_backward(dtype, a["g"], a["gs"], a["gb"], a["w"], a["bx"], a["bas"], a["bab"], a["dz"], a["slab"], B, H, 8, C, _st())
    for kw in ([dict(dtype=3), dict(C=32), dict(dtype=0, C=48), dict(B=0), dict(H=0)]
               + [{k: None} for k in ("g", "gs", "gb", "w", "bx", "bas", "bab", "dz", "slab")]):
        assert call(**kw) == N.ERR_ARG, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"


# =============================================================================================
# norm2 of an inverted-residual block in training: llie_dwconv3x3_backward feeds llie_groupnorm_backward_from_slab (slab_ready = 1)
N2_CASES = [(16, 24, 8, 128), (12, 9, 16, 128), (16, 24, 8, 2048), (12, 9, 16, 2048), (8, 8, 8, 2112)]  # (H, W, strip width, C)
N2_PARAMS = [(c, d) for c in N2_CASES for d in (0, 2)]


@pytest.mark.parametrize("case,dtype", N2_PARAMS, ids=[f"{c[0]}x{c[1]}x{c[3]}-dt{d}" for c, d in N2_PARAMS])
def test_norm2_site_from_depthwise_slab(dev, case, dtype):
    """llie_dwconv3x3_backward, then llie_groupnorm_backward_from_slab with FiLM, in place as Back::irb_bwd runs them (dh1 over dz),
    against float64 autograd of depthwise3x3(relu6(gn_film(h1))) w.r.t. h1, gamma, beta and the FiLM rows, from the stored tensors:
    B = 3; 16 x 24 (six tiles of 64 pixels) and the ragged 12 x 9 (tiles of 72 and 36 pixels); C = 128 (cg = 4: 64 tile lanes in
    gn_bwd_coef_kernel), 2048 (cg = 64, the widest group it sums itself) and 2112 at 8 x 8 (slab_reduce); fp32 and bf16.  The
    reference mirrors the kernel's mask (relu6_mask_ref) and its rounding of dz to T: autograd's dz is first checked against the
    kernel's under BAR_DW_BWD (worst 2.95 fp32, 0.16 bf16), then replaced by it, the values every later stage reads.  Measured worst
    ratio (MI355X, seeds 0..2) over dgamma / dbeta / ds / df / dh1: 2.04 fp32, 0.98 bf16; bar GN_BAR = 20."""
    L = N.lib()
    H, W, tx, C = case
    B, P = 3, H * W
    g = R.seeded(SEED0, "norm2", case, dtype)
    h1 = _rt(torch.randn(B, H, W, C, generator=g) * 1.3 + 0.4, dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5 + 0.8
    s, f = torch.randn(B, C, generator=g) * 0.3, torch.randn(B, C, generator=g) * 0.3
    da3 = _rt(torch.randn(B, H, W, C, generator=g), dtype)
    gate, dmean = torch.rand(B, C, generator=g) * 0.9 + 0.05, torch.randn(B, C, generator=g) * 0.1
    w = torch.randn(9, C, generator=g) / 3                 # the forward taps; the kernel is given them in reverse order
    x = h1.view(B, P, C)
    mean_f, rstd_f, G_f, scale, shift = _gn_record(x, gamma, beta, s, f)
    filmt = torch.full((B, 2 * C + 6), CANARY)
    filmt[:, :C], filmt[:, C:2 * C] = s, f
    d = lambda t: t.contiguous().to(dev)  # noqa: E731
    dd = [d(t) for t in (da3, gate, dmean, w.flip(0), h1, scale, shift)]
    rec = {k: d(v) for k, v in dict(mean=mean_f, rstd=rstd_f, gamma=gamma, beta=beta, film=filmt).items()}
    nt = int(L.llie_dwconv3x3_tiles(H, W))
    results = []
    for _ in range(2):
        dzg, slab, _ = _dwb_call(dev, dtype, dd, B, H, W, C)
        dz_k = dzg.cpu("dz")
        dgam, dbet = Guarded((C,), dev), Guarded((C,), dev)
        dfl = torch.full((B, 2 * C + 6), CANARY, device=dev)
        dfl[:, :2 * C] = NAN
        scr = Guarded((7 * B * C,), dev)
        A = N.GnBackwardArgs()
        A.g, A.dz, A.x0, A.c0, A.c1 = dzg.ptr, dzg.ptr, dd[4].data_ptr(), C, 0
        A.scale, A.shift, A.act = dd[5].data_ptr(), dd[6].data_ptr(), 1
        A.mean, A.rstd, A.gamma, A.beta = (rec[k].data_ptr() for k in ("mean", "rstd", "gamma", "beta"))
        A.film, A.film_stride, A.dfilm, A.dfilm_stride = rec["film"].data_ptr(), 2 * C + 6, dfl.data_ptr(), 2 * C + 6
        A.dgamma, A.dbeta, A.dx0, A.batch, A.pixels = dgam.ptr, dbet.ptr, dzg.ptr, B, P
        N.check(L.llie_groupnorm_backward_from_slab(dtype, ctypes.byref(A), slab.ptr, nt, scr.ptr, 7 * B * C, _st()), "groupnorm_backward_from_slab")
        torch.cuda.synchronize()
        scr.cpu("gn scratch")
        _split(slab.cpu("dw_bwd slab"), B, nt, "dw_bwd slab")
        results.append(dict(dz=dz_k, dx=dzg.cpu("dh1").view(B, P, C), dgamma=dgam.cpu("dgamma"), dbeta=dbet.cpu("dbeta"), dfilm=dfl.cpu()))
    for k in results[0]:
        _same(results[0][k], results[1][k], k)
    res = results[0]
    assert (res["dfilm"][:, 2 * C:] == CANARY).all()
    # float64 autograd of the whole chain; the mask and dz as the kernel rounds them
    wt = R.dw_weights(dtype, w)
    cot, _ = R.dw_operand(dtype, da3, gate, dmean, no_act=True)
    mask, unsure = R.relu6_mask_ref(h1, scale, shift)
    assert R.mask_unsure_ok(unsure, tx)
    n, leaves = _gn_forward64(x, gamma, beta, s, f, mean_f, rstd_f)
    seen = {}

    def swap(grad):
        seen["dz"] = grad.detach()
        return res["dz"].double().view(B, P, C)
    n.register_hook(swap)
    zc = (x.double() * scale.double()[:, None, :] + shift.double()[:, None, :]).float().double()
    a2 = n * mask.view(B, P, C).double() + 6.0 * (zc >= 6.0).double()
    y, _ = R.dw_from_padded(R.pad_zero(a2.view(B, H, W, C)), wt)
    gx, ggam, gbet, gs_, gf_ = torch.autograd.grad(y, leaves, cot)
    tag = f"norm2/{H}x{W}x{C}/dt{dtype}"
    ref, rab, rsl, _ = R.dwconv3x3_bwd_ref(dtype, *[da3, gate, dmean, w.flip(0), h1, scale, shift])
    sure = (~unsure).double()
    assert ((seen["dz"].view(B, H, W, C) - ref).abs() * sure <= 1e-12 * (rab + 1e-30)).all(), "autograd's dz and dwconv3x3_bwd_ref disagree"
    _ratio(res["dz"], ref, rab, rsl, R.BAR_DW_BWD, tag + "/dz")
    ab = _gn_abs_sums(res["dz"].double().view(B, P, C), x, mean_f, rstd_f, G_f, gamma, beta, s)
    _ratio(res["dgamma"], ggam, ab["dgamma"], _ulp(ggam, 0), GN_BAR, tag + "/dgamma")
    _ratio(res["dbeta"], gbet, ab["dbeta"], _ulp(gbet, 0), GN_BAR, tag + "/dbeta")
    _ratio(res["dfilm"][:, :C], gs_, ab["ds"], _ulp(gs_, 0), GN_BAR, tag + "/ds")
    _ratio(res["dfilm"][:, C:2 * C], gf_, ab["df"], _ulp(gf_, 0), GN_BAR, tag + "/df")
    _ratio(res["dx"], gx, ab["dx"], _ulp(gx, dtype), GN_BAR, tag + "/dh1")


def test_groupnorm_backward_from_slab_refusals(dev):
    """No activation, dz that is not g, a NULL slab, no tiles, a short scratch: LLIE_ERR_ARG before any HIP call."""
    L = N.lib()
    t = torch.zeros(2 * 64 * 64, device=dev)
    p = t.data_ptr()

    def call(slab=p, ntiles=1, nscr=7 * 2 * 64, **kw):
        A = N.GnBackwardArgs()
        for k, v in dict(g=p, dz=p, x0=p, c0=64, scale=p, shift=p, act=1, mean=p, rstd=p, gamma=p, beta=p, dgamma=p, dbeta=p, dx0=p,
                         batch=2, pixels=64).items():
            setattr(A, k, v)
        for k, v in kw.items():
            setattr(A, k, v)
        return L.llie_groupnorm_backward_from_slab(1, ctypes.byref(A), slab, ntiles, p, nscr, _st())
    for kw in (dict(act=0), dict(dz=p + 64), dict(slab=None), dict(ntiles=0), dict(nscr=7 * 2 * 64 - 1), dict(g=None)):
        assert call(**kw) == N.ERR_ARG, kw


# =============================================================================================
# llie_bias_grad: bwd_mask_reduce without activation or x, slab_reduce of the first of its two planes, batch_sum of Cstore < C columns
BIAS_CASES = [(3, 64, 32, 3), (3, 81, 64, 64), (2, 1296, 96, 64)]  # (B, P, C, Cstore): packed d(eps); ragged tiles; C % 64 != 0, 21 tiles


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,C,Cstore", BIAS_CASES)
def test_bias_grad_vs_float64(dev, B, P, C, Cstore, dtype):
    """llie_bias_grad, the chain Back::bias_grad runs for the conv biases: (M, C, P, Cstore) = (3 * 64, 32, 64, 3), the packed d(eps)
    of the output head; (3 * 81, 64, 81, 64), a partly empty last tile; (2 * 1296, 96, 1296, 64), C not a multiple of the 64-channel
    block and more tiles than slab_reduce's 16 groups.  Columns Cstore.. of out must stay untouched (canary), the scratch sized by
    llie_bias_grad_floats is not overrun.  Measured worst ratio (MI355X, seeds 0..2): 0.36 fp32, 0.32 fp16, 0.18 bf16; bar
    BAR_BIAS_GRAD = 3.6."""
    L = N.lib()
    g = _rt(torch.randn(B * P, C, generator=R.seeded(SEED0, "bias", B, P, C, dtype)) + 0.2, dtype)
    gd = g.to(dev)
    ns, nS = ctypes.c_int64(), ctypes.c_int64()
    N.check(L.llie_bias_grad_floats(B, C, P, ctypes.byref(ns), ctypes.byref(nS)), "bias_grad_floats")
    assert (ns.value, nS.value) == (B * ((P + 63) // 64) * 2 * C, B * C)
    outs = []
    for _ in range(2):
        slab, S = Guarded((ns.value,), dev), Guarded((nS.value,), dev)
        out = torch.full((C + 8,), CANARY, device=dev)
        out[:Cstore] = NAN
        N.check(L.llie_bias_grad(dtype, gd.data_ptr(), B * P, C, P, Cstore, slab.ptr, S.ptr, out.data_ptr(), _st()), "bias_grad")
        torch.cuda.synchronize()
        slab.cpu("bias_grad slab"), S.cpu("bias_grad S")
        outs.append(out.cpu())
    _same(outs[0], outs[1], "bias_grad")
    assert (outs[0][Cstore:] == CANARY).all(), "bias_grad wrote past out[Cstore]"
    ref, ab, sl = R.bias_grad_ref(g, Cstore)
    _ratio(outs[0][:Cstore], ref, ab, sl, R.BAR_BIAS_GRAD, f"bias_grad/{B}x{P}x{C}/dt{dtype}")


# =============================================================================================
# pack_planes, add_into, the four pointwise fp32 kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c0,c1", [(3, 3), (3, 0), (4, 2)])
def test_pack_planes_exact(dev, c0, c1, dtype):
    """llie_pack_planes: two 3-channel halves (the input conv's operand), one (the packed d(eps)) and unequal halves (4 + 2: x1 has its
    own plane stride), B = 3, P = 100 (the last workgroup is partial): equal bits with the rounded planes, channels c0 + c1 .. 31 zero,
    nothing past the last row."""
    L = N.lib()
    B, P = 3, 100
    g = R.seeded(SEED0, "pack", c0, c1, dtype)
    x0 = torch.randn(B, c0, P, generator=g)
    x1 = torch.randn(B, c1, P, generator=g) if c1 else None
    x0d, x1d = x0.to(dev), (x1.to(dev) if c1 else None)
    outs = []
    for _ in range(2):
        out = Guarded((B * P, 32), dev, TDT[dtype])
        N.check(L.llie_pack_planes(dtype, x0d.data_ptr(), c0, x1d.data_ptr() if c1 else None, c1, out.ptr, B, P, _st()), "pack_planes")
        torch.cuda.synchronize()
        outs.append(out.cpu("pack_planes"))
    _same(outs[0], outs[1], "pack_planes")
    _same(outs[0], R.pack_planes_ref(dtype, x0, x1), "pack_planes against the rounded planes")


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_into_exact(dev, dtype):
    """llie_add_into over n = 8 * 257 elements (a partial last workgroup): dst + src formed in fp32 and rounded once, equal bits."""
    L = N.lib()
    n = 8 * 257
    g = R.seeded(SEED0, "add_into", dtype)
    a, b = _rt(torch.randn(n, generator=g) * 3, dtype), _rt(torch.randn(n, generator=g), dtype)
    bd = b.to(dev)
    outs = []
    for _ in range(2):
        dst = Guarded((n,), dev, TDT[dtype])
        dst.v.copy_(a.to(dev))
        N.check(L.llie_add_into(dtype, dst.ptr, bd.data_ptr(), n, _st()), "add_into")
        torch.cuda.synchronize()
        outs.append(dst.cpu("add_into"))
    _same(outs[0], outs[1], "add_into")
    _same(outs[0], R.add_into_ref(dtype, a, b), "add_into against the fp32 sum")
    assert L.llie_add_into(dtype, bd.data_ptr(), bd.data_ptr(), n + 1, _st()) == N.ERR_ARG


@pytest.mark.parametrize("kind", [N.PW_SIGMOID_BWD, N.PW_RELU6_BWD, N.PW_SILU_BWD, N.PW_SCALE])
def test_pointwise_backward_vs_float64(dev, kind):
    """llie_pointwise_backward, n = 1000 (a partial last workgroup): sigmoid' from the gate; ReLU6' from the activation's output with y
    exactly 0 and exactly 6 among the values (both masked); SiLU' with |x| up to 20; the row scale.  ReLU6' and the scale must give
    equal bits.  Measured worst ratio (MI355X, seeds 0..2): sigmoid' 0.67, SiLU' 0.55; bar BAR_PW_BWD = 6.7."""
    L = N.lib()
    n = 1000
    g = R.seeded(SEED0, "pointwise", kind)
    a = torch.randn(n, generator=g)
    if kind == N.PW_SIGMOID_BWD:
        b = torch.sigmoid(torch.randn(n, generator=g) * 3)
    elif kind == N.PW_RELU6_BWD:
        b = (torch.randn(n, generator=g) * 3 + 3).clamp(0.0, 6.0)
        b[:4] = torch.tensor([0.0, 6.0, 1e-30, 6.0 - 2.0 ** -21])
        assert (b == 0).sum() > 4 and (b == 6).sum() > 4
    elif kind == N.PW_SILU_BWD:
        b = (torch.rand(n, generator=g) * 2 - 1) * 20
        b[:2] = torch.tensor([-20.0, 20.0])
    else:
        b = None
    scale = 1.0 / 324.0
    ad, bd = a.to(dev), (b.to(dev) if b is not None else None)
    outs = []
    for _ in range(2):
        out = Guarded((n,), dev)
        N.check(L.llie_pointwise_backward(kind, ad.data_ptr(), bd.data_ptr() if b is not None else None, out.ptr, n, scale, _st()), "pointwise_backward")
        torch.cuda.synchronize()
        outs.append(out.cpu("pointwise"))
    _same(outs[0], outs[1], "pointwise")
    ref, ab = R.pointwise_bwd_ref(kind, a, b, scale)
    if ab is None:
        _same(outs[0], ref.float(), f"pointwise kind {kind}")
    else:
        _ratio(outs[0], ref, ab, _ulp(ref, 0), R.BAR_PW_BWD, f"pointwise/kind{kind}")
    assert L.llie_pointwise_backward(4, ad.data_ptr(), ad.data_ptr(), ad.data_ptr(), n, 1.0, _st()) == N.ERR_ARG
    assert L.llie_pointwise_backward(0, ad.data_ptr(), None, ad.data_ptr(), n, 1.0, _st()) == N.ERR_ARG


# =============================================================================================
# the sinusoidal embedding and the time MLP
def test_sin_embed_and_time_embed_vs_float64(dev):
    """llie_time_embed on a `small` context (base_channels 32, time_embed_dim 128) with synthetic weights, t = 0, 1, 500, 999: emb against
    float64 cos / sin of the fp32 product float(t) * freqs[i]; temb and silu_temb against the float64 MLP of the kernel's own emb;
    llie_sin_embed with the same frequency table gives the bits of emb.  Measured worst ratio (MI355X, seeds 0..2): emb 0.00 (inside the
    ulp of the stored value; BAR_SIN_EMBED = 2 is reasoned, see kernel_refs.py), temb 0.68, silu_temb 0.53; bar BAR_TIME_EMBED = 6.8."""
    L = N.lib()
    Um = importlib.import_module("cv-diffusion-model_amd.unet")
    h = N.Handle(Um.create_efficient_unet("small", 64)._make_cfg(0))
    try:
        g = R.seeded(SEED0, "time_embed")
        names = [k for k, _ in h.params()]
        params = [(torch.randn(shape, generator=g) / math.sqrt(max(1, shape[-1] if len(shape) > 1 else 1))) for _, shape in h.params()]
        pd = [p.to(dev) for p in params]
        h.load_all(pd, _st())
        by = {k: p for k, p in zip(names, params)}
        w1, b1, w3, b3 = (next(v for k, v in by.items() if k.endswith(sfx)) for sfx in
                          ("time_mlp.1.weight", "time_mlp.1.bias", "time_mlp.3.weight", "time_mlp.3.bias"))
        dim, T = w1.shape[1], w1.shape[0]
        assert (dim, T) == (32, 128)
        t = torch.tensor([0, 1, 500, 999], dtype=torch.int64)
        td, rows = t.to(dev), 4
        freqs = R.sin_freqs(dim)
        fd = freqs.to(dev)
        runs = []
        for _ in range(2):
            emb, temb, st, emb2 = (Guarded((rows, k), dev) for k in (dim, T, T, dim))
            N.check(L.llie_time_embed(h.h, td.data_ptr(), rows, emb.ptr, temb.ptr, st.ptr, _st()), "time_embed")
            N.check(L.llie_sin_embed(td.data_ptr(), fd.data_ptr(), emb2.ptr, rows, dim, _st()), "sin_embed")
            torch.cuda.synchronize()
            runs.append([b.cpu("time_embed") for b in (emb, temb, st, emb2)])
        for a, b in zip(runs[0], runs[1]):
            _same(a, b, "time_embed")
        emb, temb, st, emb2 = runs[0]
        _same(emb2, emb, "sin_embed against time_embed's emb_out")
        ref, ab, sl = R.sin_embed_ref(t, freqs)
        _ratio(emb, ref, ab, sl, R.BAR_SIN_EMBED, "sin_embed")
        (tr, ta, tsl), (sr, sa, ssl) = R.time_embed_ref(emb, w1, b1, w3, b3)
        _ratio(temb, tr, ta, tsl, R.BAR_TIME_EMBED, "time_embed/temb")
        _ratio(st, sr, sa, ssl, R.BAR_TIME_EMBED, "time_embed/silu_temb")
        assert L.llie_sin_embed(td.data_ptr(), fd.data_ptr(), None, rows, dim, _st()) == N.ERR_ARG
        assert L.llie_sin_embed(td.data_ptr(), fd.data_ptr(), fd.data_ptr(), rows, 31, _st()) == N.ERR_ARG
    finally:
        h.close()
