"""The float64 references of the depthwise input gradient and the backward pass's glue (tests/kernel_refs.py), checked without a GPU,
as tests/test_forward_refs_host.py does for the forward kernels.

(a) On the fp32 path the references agree with torch's own float64 autograd and with direct sums.
(b) The bars have teeth: what a subtly wrong kernel would store is compared with the correct reference through the very function, bars
    and slack of tests/test_gpu_backward_kernels.py, in every dtype; each mutant must fail, the correct values must pass.
(c) For every case and seed of the GPU tests the reference alone decides the ReLU6 mask: entries whose mask depends on how the kernel
    rounds z are at most 0.1 % of a case and never a whole slab entry's worth (kernel_refs.mask_unsure_ok).
"""
import ctypes
import importlib
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402
from kernel_refs import _r64, _ratio, _rt  # noqa: E402
from test_forward_refs_host import _passes, _teeth  # noqa: E402  (one copy)

DTYPES = [0, 1, 2]


# ================================================================================================ (a) against torch's operators
@pytest.mark.parametrize("H,W,tx", [(9, 13, 16), (16, 16, 8)])
def test_dwconv_bwd_ref_vs_autograd(H, W, tx):
    """fp32: dz of dwconv3x3_bwd_ref is float64 autograd's gradient of conv2d(relu6(bx bas + bab), w, groups = C) w.r.t. the conv's
    input, times relu6', for the cotangent g gs + gb; the kernel's table is the forward's with the taps reversed."""
    B, C = 3, 32
    g, gs, gb, wk, bx, bas, bab = R.dw_bwd_inputs(B, H, W, C, 0, 0, ("host", H, W))
    ref, ab, sl, unsure = R.dwconv3x3_bwd_ref(0, g, gs, gb, wk, bx, bas, bab)
    assert R.mask_unsure_ok(unsure, tx)
    z = (bx.double() * bas.double()[:, None, None] + bab.double()[:, None, None]).permute(0, 3, 1, 2).requires_grad_(True)
    wf = wk.flip(0).double().t().reshape(C, 1, 3, 3)          # the forward conv's weights
    y = F.conv2d(F.relu6(z), wf, padding=1, groups=C)
    cot = (g.double() * gs.double()[:, None, None] + gb.double()[:, None, None]).permute(0, 3, 1, 2)
    (t,) = torch.autograd.grad(y, [z], cot)
    # the reference rounds the operand and z to fp32 once: half an ulp per operand; an unsure mask may go either way
    _ratio(t.permute(0, 2, 3, 1), ref, ab, torch.where(unsure, sl, torch.zeros_like(sl)), 2.0, "dwconv3x3_bwd_ref vs autograd")
    assert (ref[..., 0][(bx[..., 0] == 6) | (bx[..., 0] == 0)] == 0).all(), "exact zeros and sixes of channel 0 are masked"
    # the slab against direct sums
    dz = ref.float()
    sref, sab, _ = R.strip_stats2_ref(dz, bx, tx)
    ny, nx = (H + 7) // 8, (W + tx - 1) // tx
    assert sref.shape == (B, ny * nx, 2, C)
    q, x = dz.double(), bx.double()
    last = (ny - 1) * nx + nx - 1
    assert torch.allclose(sref[:, last, 0], q[:, 8 * (ny - 1):, tx * (nx - 1):].sum((1, 2)), rtol=0, atol=1e-12)
    assert torch.allclose(sref[:, 0, 1], (q * x)[:, :8, :tx].sum((1, 2)), rtol=0, atol=1e-12)
    assert torch.allclose(sref.sum(1)[:, 1], (q * x).sum((1, 2)), rtol=1e-12, atol=1e-12)
    assert torch.allclose(sab.sum(1)[:, 0], q.abs().sum((1, 2)), rtol=1e-12)


def test_glue_refs_vs_torch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3 * 81, 64, generator=g)
    ref, ab, _ = R.bias_grad_ref(x, 40)
    assert torch.equal(ref, x.double().sum(0)[:40]) and torch.equal(ab, x.double().abs().sum(0)[:40])
    x0, x1 = torch.randn(2, 4, 10, generator=g), torch.randn(2, 2, 10, generator=g)
    pk = R.pack_planes_ref(0, x0, x1).view(2, 10, 32)
    assert torch.equal(pk[1, 7, :4], x0[1, :, 7]) and torch.equal(pk[1, 7, 4:6], x1[1, :, 7]) and (pk[:, :, 6:] == 0).all()
    a, b = _rt(torch.randn(64, generator=g) * 3, 2), _rt(torch.randn(64, generator=g), 2)
    assert torch.equal(R.add_into_ref(2, a, b), (a.float() + b.float()).bfloat16())
    # the embedding and the MLP against torch's own float64 operators
    t = torch.tensor([0, 1, 500, 999])
    fr = R.sin_freqs(32)
    assert torch.allclose(fr.double(), torch.exp(-torch.log(torch.tensor(10000.0, dtype=torch.float64)) * torch.arange(16) / 16), rtol=1e-6)
    emb, _, _ = R.sin_embed_ref(t, fr)
    arg = t.double()[:, None] * fr.double()[None]
    assert (emb - torch.cat([arg.cos(), arg.sin()], 1)).abs().max() < 999 * 2.0 ** -24  # the fp32 product moves the argument
    w1, b1 = torch.randn(128, 32, generator=g) / 6, torch.randn(128, generator=g)
    w3, b3 = torch.randn(128, 128, generator=g) / 11, torch.randn(128, generator=g)
    (te, ta, _), (st, sa, _) = R.time_embed_ref(emb.float(), w1, b1, w3, b3)
    tt = F.linear(F.silu(F.linear(emb.float().double(), w1.double(), b1.double())), w3.double(), b3.double())
    assert torch.allclose(te, tt, rtol=1e-12, atol=1e-12) and torch.allclose(st, F.silu(tt), rtol=1e-12, atol=1e-12)
    assert (ta >= te.abs()).all() and (sa >= st.abs()).all()
    # the pointwise derivatives against autograd
    v = (torch.rand(100, generator=g, dtype=torch.float64) * 40 - 20).requires_grad_(True)
    dy = torch.randn(100, generator=g)
    (gs,) = torch.autograd.grad(F.silu(v), [v], dy.double())
    assert torch.allclose(R.pointwise_bwd_ref(2, dy, v.detach().float())[0], gs, rtol=1e-5, atol=1e-9)
    (gg,) = torch.autograd.grad(torch.sigmoid(v), [v], dy.double())
    assert torch.allclose(R.pointwise_bwd_ref(0, dy, torch.sigmoid(v.detach()))[0], gg, rtol=1e-12, atol=1e-15)
    y6 = torch.tensor([0.0, 6.0, 1e-30, 5.9, -0.0])
    assert R.pointwise_bwd_ref(1, torch.ones(5), y6)[0].tolist() == [0.0, 0.0, 1.0, 1.0, 0.0]


# ================================================================================================ (b) teeth
@pytest.mark.parametrize("dtype", DTYPES)
def test_dwconv_bwd_bars_reject_wrong_kernels(dtype):
    """16 x 16 in 8-wide strips (two strips, two slab segments) and the ragged 12 x 16 (a last segment of four rows), through
    BAR_DW_BWD and BAR_DW_BWD_STATS with the reference's own slack."""
    B, H, W, C, tx = 3, 16, 16, 32 if dtype == 0 else 64, 8
    inp = R.dw_bwd_inputs(B, H, W, C, dtype, 0, ("teeth", dtype))
    g, gs, gb, wk, bx, bas, bab = inp
    ref, ab, sl, unsure = R.dwconv3x3_bwd_ref(dtype, *inp)
    assert not unsure.any()
    mask, _ = R.relu6_mask_ref(bx, bas, bab)
    a, _ = R.dw_operand(dtype, g, gs, gb, no_act=True)
    acc, _ = R.dw_from_padded(R.pad_zero(a), R.dw_weights(dtype, wk))
    z = R._f32(bx.double() * bas.double()[:, None, None] + bab.double()[:, None, None])
    a_cut = a.clone()
    a_cut[:, :, tx - 1] = 0.0                                  # the second strip's left halo column never arrives
    halo = ref.clone()
    halo[:, :, tx] = (R.dw_from_padded(R.pad_zero(a_cut), R.dw_weights(dtype, wk))[0] * mask.double())[:, :, tx]
    mutants = {
        "unflipped taps": R.dwconv3x3_bwd_ref(dtype, g, gs, gb, wk.flip(0), bx, bas, bab)[0],
        "mask <= at 6": acc * ((z > 0) & (z <= 6)).double(),
        "mask >= at 0": acc * ((z >= 0) & (z < 6)).double(),
        "mask of the neighbouring pixel": acc * torch.roll(mask, 1, dims=2).double(),
        "dropped left halo column of the second strip": halo,
        "gb of image 0 for every image": R.dwconv3x3_bwd_ref(dtype, g, gs, gb[:1].expand(B, -1).contiguous(), wk, bx, bas, bab)[0],
        "no mask": acc,
    }
    _teeth(dtype, ref, ab, sl, R.BAR_DW_BWD, mutants)
    # the slab, from the dz a correct kernel stores
    dz = _rt(ref, dtype)
    sref, sab, ssl = R.strip_stats2_ref(dz, bx, tx)
    nx = W // tx
    v = sref.view(B, 2, nx, 2, C)
    slab_mutants = {
        "segments 0 and 1 of the 16-row strip swapped": v.flip(1).reshape(sref.shape),
        "strips swapped": v.flip(2).reshape(sref.shape),
        "the two planes swapped": sref.flip(2),
        "sum dz in both planes": torch.stack([sref[:, :, 0], sref[:, :, 0]], 2),
        "16-wide tiles": torch.stack([R.strip_stats2_ref(dz, bx, 16)[0][:, i // 2] for i in range(4)], 1),
    }
    _teeth(dtype, sref, sab, ssl, R.BAR_DW_BWD_STATS, slab_mutants, stored_in=0)
    # ragged rows: 12 x 16 in 16-wide strips, the last segment holds rows 8..11 only
    Hr, txr = 12, 16
    inp = R.dw_bwd_inputs(B, Hr, W, C, dtype, 0, ("teeth ragged", dtype))
    refr, _, _, _ = R.dwconv3x3_bwd_ref(dtype, *inp)
    dzr, bxr = _rt(refr, dtype), inp[4]
    sref, sab, ssl = R.strip_stats2_ref(dzr, bxr, txr)
    assert sref.shape == (B, 2, 2, C)
    extra = sref.clone()
    extra[:, 1, 1] += (dzr.double() * bxr.double())[:, Hr - 1].sum(1)   # a row past the image read as the last row again
    both = extra.clone()
    both[:, 1, 0] += dzr.double()[:, Hr - 1].sum(1)
    _teeth(dtype, sref, sab, ssl, R.BAR_DW_BWD_STATS,
           {"an out-of-image row in sum dz*bx": extra, "an out-of-image row in both sums": both}, stored_in=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_glue_bars_reject_wrong_kernels(dtype):
    g = torch.Generator().manual_seed(17 + dtype)
    B, P, C, Cstore = 3, 81, 64, 64
    x = _rt(torch.randn(B * P, C, generator=g) + 0.2, dtype)
    ref, ab, sl = R.bias_grad_ref(x, Cstore)
    xb = x.double().view(B, P, C)
    _teeth(dtype, ref, ab, sl, R.BAR_BIAS_GRAD, {
        "the j = 1 plane (sum g * 0) reduced in place of j = 0": torch.zeros_like(ref),
        "the last tile's rows past the image counted (the next image's)": ref + xb[1:, :128 - P].sum((0, 1)),
        "an image left out": xb[:2].sum((0, 1)),
    }, stored_in=0)
    # pack_planes: equal bits are asked for, so a mutant only has to differ
    x0, x1 = torch.randn(B, 4, 100, generator=g), torch.randn(B, 2, 100, generator=g)
    want = R.pack_planes_ref(dtype, x0, x1)
    flat = x1.reshape(-1)
    c0_stride = torch.stack([torch.stack([flat[((b * 4 + c) * 100) % flat.numel():][:100] for c in range(2)]) for b in range(B)])
    assert not torch.equal(R.pack_planes_ref(dtype, x0, c0_stride), want), "x1 indexed with c0's plane stride goes unnoticed"
    assert not torch.equal(R.pack_planes_ref(dtype, x0, x1.flip(1)), want)
    # the embedding: a swapped cos / sin half and a truncated timestep
    t, fr = torch.tensor([0, 1, 500, 999]), R.sin_freqs(32)
    eref, eab, esl = R.sin_embed_ref(t, fr)
    assert _passes(eref.float(), eref, eab, esl, R.BAR_SIN_EMBED)
    assert not _passes(torch.cat([eref[:, 16:], eref[:, :16]], 1).float(), eref, eab, esl, R.BAR_SIN_EMBED)
    assert not _passes(R.sin_embed_ref(t, fr.bfloat16().float())[0].float(), eref, eab, esl, R.BAR_SIN_EMBED)
    w1, b1 = torch.randn(128, 32, generator=g) / 6, torch.randn(128, generator=g)
    w3, b3 = torch.randn(128, 128, generator=g) / 11, torch.randn(128, generator=g)
    (te, ta, tsl), (st, sa, ssl) = R.time_embed_ref(eref.float(), w1, b1, w3, b3)
    assert _passes(te.float(), te, ta, tsl, R.BAR_TIME_EMBED) and _passes(st.float(), st, sa, ssl, R.BAR_TIME_EMBED)
    (te2, _, _), (st2, _, _) = R.time_embed_ref(eref.float(), w1, b1, w3, torch.zeros_like(b3))
    assert not _passes(te2.float(), te, ta, tsl, R.BAR_TIME_EMBED) and not _passes(st2.float(), st, sa, ssl, R.BAR_TIME_EMBED)
    (te3, _, _), _ = R.time_embed_ref(eref.float().half().float(), w1, b1, w3, b3)
    assert not _passes(te3.float(), te, ta, tsl, R.BAR_TIME_EMBED), "an embedding rounded to fp16 goes unnoticed"
    # the pointwise derivatives: sigmoid' with g (1 + g), SiLU' without its second term
    a, v = torch.randn(1000, generator=g), (torch.rand(1000, generator=g) * 2 - 1) * 20
    r0, a0 = R.pointwise_bwd_ref(0, a, torch.sigmoid(v))
    assert _passes(r0.float(), r0, a0, R._ulp(r0, 0), R.BAR_PW_BWD)
    assert not _passes((a.double() * torch.sigmoid(v).double() * (1 + torch.sigmoid(v).double())).float(), r0, a0, R._ulp(r0, 0), R.BAR_PW_BWD)
    r2, a2 = R.pointwise_bwd_ref(2, a, v)
    assert _passes(r2.float(), r2, a2, R._ulp(r2, 0), R.BAR_PW_BWD)
    assert not _passes((a.double() * torch.sigmoid(v.double())).float(), r2, a2, R._ulp(r2, 0), R.BAR_PW_BWD)
    assert not _passes(_r64(r2, 1), r2, a2, R._ulp(r2, 0), R.BAR_PW_BWD), "a result rounded to fp16 goes unnoticed"


# ================================================================================================ (c) the mask is decided
@pytest.mark.parametrize("seed0", [0, 1, 2])
def test_mask_is_decided_for_every_gpu_case(seed0):
    """Every case of test_dwconv3x3_backward_vs_float64 and test_dwconv3x3_backward_strip_heights, at the three seeds the bars were
    measured with: at most 0.1 % of the entries have a mask that depends on the kernel's rounding of z, no slab tile consists of such
    entries alone, and each case masks entries on both sides (so that a wrong comparison shows)."""
    for case in R.DW_BWD_CASES:
        _, _, _, _, bx, bas, bab = R.dw_bwd_case_inputs(case, seed0)
        mask, unsure = R.relu6_mask_ref(bx, bas, bab)
        assert R.mask_unsure_ok(unsure, case[2]), (case, seed0)
        frac = mask.float().mean().item()
        assert 0.5 < frac < 0.95, (case, seed0, frac)
    for H, rows, _, dtype in R.DW_BWD_STRIPS:
        _, _, _, _, bx, bas, bab = R.dw_bwd_strip_inputs(H, rows, dtype, seed0)
        assert R.mask_unsure_ok(R.relu6_mask_ref(bx, bas, bab)[1], 8), (H, rows, dtype, seed0)
    # the condition itself: a tile of nothing but unsure entries, or too many of them, is refused
    u = torch.zeros(1, 9, 8, 32, dtype=torch.bool)
    assert R.mask_unsure_ok(u, 8)
    u[0, 8, :, 3] = True                                        # the ragged last segment's only row
    assert not R.mask_unsure_ok(u, 8)
    u[:] = False
    u[0, :3, 0, 0] = True                                       # 3 of 2304 entries
    assert not R.mask_unsure_ok(u, 8)


# ================================================================================================ contracts, before any HIP call
def test_backward_glue_entry_points_refuse_bad_arguments():
    """LLIE_ERR_ARG before any HIP call, so this runs without a GPU; pointers are dummies that are never read."""
    N = importlib.import_module("cv-diffusion-model_amd._native")
    L = N.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    E = N.ERR_ARG

    def dwb(dtype=1, B=2, H=8, W=8, C=64, **kw):
        a = dict(g=p, gs=p, gb=p, w=p, bx=p, bas=p, bab=p, dz=p, slab=p)
        a.update(kw)
        return L.llie_dwconv3x3_backward(dtype, a["g"], a["gs"], a["gb"], a["w"], a["bx"], a["bas"], a["bab"], a["dz"], a["slab"], B, H, W, C, None)
    for kw in ([dict(dtype=3), dict(dtype=-1), dict(C=32), dict(dtype=0, C=48), dict(C=0), dict(B=0), dict(H=0), dict(W=0)]
               + [{k: None} for k in ("g", "gs", "gb", "w", "bx", "bas", "bab", "dz", "slab")]):
        assert dwb(**kw) == E, kw
    ns, nS = ctypes.c_int64(), ctypes.c_int64()
    assert L.llie_bias_grad_floats(3, 96, 81, ctypes.byref(ns), ctypes.byref(nS)) == 0 and (ns.value, nS.value) == (3 * 2 * 2 * 96, 3 * 96)
    assert L.llie_bias_grad_floats(0, 96, 81, ctypes.byref(ns), ctypes.byref(nS)) == E and L.llie_bias_grad_floats(3, 96, 81, None, ctypes.byref(nS)) == E
    for args in ((3, p, 128, 64, 64, 64, p, p, p), (1, None, 128, 64, 64, 64, p, p, p), (1, p, 128, 64, 64, 64, None, p, p),
                 (1, p, 128, 64, 64, 64, p, None, p), (1, p, 128, 64, 64, 64, p, p, None), (1, p, 100, 64, 64, 64, p, p, p),
                 (1, p, 128, 48, 64, 48, p, p, p), (1, p, 128, 64, 64, 65, p, p, p), (1, p, 128, 64, 64, 0, p, p, p), (1, p, 32, 64, 64, 64, p, p, p)):
        assert L.llie_bias_grad(*args, None) == E, args
    for args in ((3, p, 3, p, 3, p, 2, 64), (1, None, 3, p, 3, p, 2, 64), (1, p, 3, p, 3, None, 2, 64), (1, p, 0, p, 3, p, 2, 64),
                 (1, p, 6, p, 3, p, 2, 64), (1, p, 3, None, 3, p, 2, 64), (1, p, 3, p, 0, p, 2, 64), (1, p, 3, p, 3, p, 0, 64), (1, p, 3, p, 3, p, 2, 0)):
        assert L.llie_pack_planes(*args, None) == E, args
    for args in ((3, p, p, 64), (1, None, p, 64), (1, p, None, 64), (1, p, p, 0), (1, p, p, 12), (0, p, p, 6)):
        assert L.llie_add_into(*args, None) == E, args
    for args in ((None, p, p, 4, 32), (p, None, p, 4, 32), (p, p, None, 4, 32), (p, p, p, 0, 32), (p, p, p, 4, 0), (p, p, p, 4, 31)):
        assert L.llie_sin_embed(*args, None) == E, args
    for args in ((-1, p, p, p, 64, 1.0), (4, p, p, p, 64, 1.0), (0, None, p, p, 64, 1.0), (1, p, None, p, 64, 1.0), (2, p, p, None, 64, 1.0),
                 (3, p, None, None, 64, 1.0), (0, p, p, p, 0, 1.0)):
        assert L.llie_pointwise_backward(*args, None) == E, args

    def gns(slab=p, ntiles=2, nscr=7 * 2 * 64, **kw):
        A = N.GnBackwardArgs()
        for k, v in dict(g=p, dz=p, x0=p, c0=64, scale=p, shift=p, act=1, mean=p, rstd=p, gamma=p, beta=p, dgamma=p, dbeta=p, dx0=p,
                         batch=2, pixels=81).items():
            setattr(A, k, v)
        for k, v in kw.items():
            setattr(A, k, v)
        return L.llie_groupnorm_backward_from_slab(2, ctypes.byref(A), slab, ntiles, p, nscr, None)
    for kw in (dict(act=0), dict(dz=p + 64), dict(slab=None), dict(ntiles=0), dict(nscr=7 * 2 * 64 - 1), dict(g=None), dict(c0=48)):
        assert gns(**kw) == E, kw
