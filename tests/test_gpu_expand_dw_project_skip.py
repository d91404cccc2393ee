"""The 96 -> 32 decoder block (skip conv, concatenated input) without h2: expand_pool + expand_dw_project in its skip form
(irbx.hip, entry point llie_expand_dw_project_skip, knob "irbx_project" = 1; 2 keeps the identity-residual shapes only).

  * the entry point against float64, with its GroupNorm slab, next to a float64 emulation that rounds where the kernel rounds
  * one block: unfused / expand_dw + project GEMM / expand_pool + expand_dw_project against the CPU oracle
  * the whole network at small@64: knob 1 against knob 2, reproducible, batch-invariant
"""
import importlib
import math

import pytest
import torch

import oracle
from oracle import unet_ref
from oracle.weightgen import synth_tensor
from conftest import max_abs, synth_input

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")

CIN, COUT, CHID = 96, 32, 384


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def psnr01(a, b):
    a = (torch.as_tensor(a).double().clamp(-1, 1) + 1) / 2
    b = (torch.as_tensor(b).double().clamp(-1, 1) + 1) / 2
    mse = ((a - b) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


def block_inputs(cin, H, W, B, tdt, seed):
    """Operands of the recompute kernels as the engine hands them over (CPU): x NHWC in T, norm1's tables already / 6,
    norm2 + FiLM tables undivided, expand weights in T, depthwise weights fp32 [9][Chid]."""
    g = torch.Generator().manual_seed(seed)
    chid = 4 * cin
    t = {}
    t["x"] = torch.randn(B, H, W, cin, generator=g).to(tdt)
    t["s1"] = 0.15 + 0.1 * torch.rand(B, cin, generator=g)
    t["b1"] = 0.3 + 0.2 * torch.rand(B, cin, generator=g)
    t["w1"] = (torch.randn(chid, cin, generator=g) / math.sqrt(cin)).to(tdt)
    t["s2"] = 0.5 + torch.rand(B, chid, generator=g)
    t["b2"] = 1.0 + 2.0 * torch.rand(B, chid, generator=g)
    t["wd"] = 0.3 * torch.randn(9, chid, generator=g)
    return t


def depthwise64(a, wd9):
    """a [B][H][W][C] float64, wd9 [9][C] tap-major -> conv2d(padding=1, groups=C), NCHW float64"""
    C = a.shape[-1]
    w = wd9.double().t().reshape(C, 1, 3, 3)
    return torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), w, padding=1, groups=C)


def front64(t, tdt, emulate):
    """float64 h2 = dw3x3(relu6(norm2(W1 relu6(norm1 x)))) [B][H][W][Chid] from the T-rounded x and weights.  emulate: round the
    depthwise input and the staged weights 6 w to T, as the kernel does; else neither."""
    ap = (t["x"].double() * t["s1"].double()[:, None, None, :] + t["b1"].double()[:, None, None, :]).clamp(0, 1).to(tdt).double()
    acc = ap @ t["w1"].double().t()                                                   # h1 / 6
    a = (acc * t["s2"].double()[:, None, None, :] + t["b2"].double()[:, None, None, :] / 6).clamp(0, 1)   # relu6(.) / 6
    if emulate:
        a = a.to(tdt).double()
    w6 = (6 * t["wd"]).to(tdt).double() if emulate else 6 * t["wd"].double()
    return depthwise64(a, w6).permute(0, 2, 3, 1)


# ------------------------------------------------------------------ 1. the entry point
@pytest.mark.parametrize("dtype,tdt,tol", [(1, torch.float16, 4e-3), (2, torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("c0,c1", [(64, 32), (32, 64)])
@pytest.mark.parametrize("H,W,B", [(8, 16, 2),      # one tile, every pixel class is a border
                                   (16, 32, 3),     # 2 x 2 tiles, no interior tile
                                   (24, 48, 1)])    # one interior tile, a width that is no power of two
def test_expand_dw_project_skip_entry_point_vs_float64(dev, dtype, tdt, tol, c0, c1, H, W, B):
    """y = Wp (gate * dw3x3(relu6(norm2(W1 relu6(norm1 x))))) + Wskip x with a gate the test supplies, against float64 from the
    same T-rounded inputs; the slab's sums against the stored y.  Outputs start as NaN so that an unwritten pixel or slab entry
    shows.  A float64 emulation that rounds to T where the kernel does (the depthwise input, 6 w, gate * h2, y) is printed next
    to the kernel: on these inputs it sits at 0.10-0.17 of the bound in both types, and a kernel error several times the
    emulation's is a bug even where it is under the bound."""
    L = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    t = block_inputs(CIN, H, W, B, tdt, 77 * CIN + H + c0)
    g = torch.Generator().manual_seed(CIN + W + c0)
    gate = torch.rand(B, CHID, generator=g)
    ld = CHID + CIN
    wps = (torch.randn(COUT, ld, generator=g) / math.sqrt(ld)).to(tdt)
    wp, wsk = wps[:, :CHID].double(), wps[:, CHID:].double()
    shortcut = t["x"].double() @ wsk.t()
    ref = (front64(t, tdt, False) * gate.double()[:, None, None, :]) @ wp.t() + shortcut
    # the kernel's fp32 product gate * h2 is rounded to T once; float32 first, as the accumulators are
    gh = (front64(t, tdt, True) * gate.double()[:, None, None, :]).float().to(tdt).double()
    emu = (gh @ wp.t() + shortcut).float().to(tdt).double()
    d = {k: v.to(dev) for k, v in t.items()}
    x0 = t["x"][..., :c0].contiguous().to(dev)
    x1 = t["x"][..., c0:].contiguous().to(dev)
    gd, wd_ = gate.to(dev), wps.to(dev)
    nt = int(L.llie_irbx_project_tiles(H, W))
    assert nt == (H // 8) * (W // 16)
    y = torch.full((B, H, W, COUT), float("nan"), dtype=tdt, device=dev)
    stats = torch.full((B, nt, 2, COUT), float("nan"), device=dev)
    N.check(L.llie_expand_dw_project_skip(dtype, x0.data_ptr(), c0, x1.data_ptr(), c1, d["s1"].data_ptr(), d["b1"].data_ptr(),
                                          d["w1"].data_ptr(), d["s2"].data_ptr(), d["b2"].data_ptr(), d["wd"].data_ptr(), gd.data_ptr(),
                                          wd_.data_ptr(), ld, COUT, y.data_ptr(), stats.data_ptr(), B, H, W, st), "expand_dw_project_skip")
    torch.cuda.synchronize()
    got = y.cpu().double()
    rmax = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    err_emu = (emu - ref).abs().max().item()
    bound = tol * max(1.0, rmax)
    msg = (f"max |y - float64|: kernel {err:.3e}, emulation {err_emu:.3e}, bound {bound:.3e}, |ref|max {rmax:.3e}"
           " (a kernel error several times the emulation's is a bug even under the bound)")
    print(msg)
    assert err < bound, msg
    o = got.view(B, H * W, COUT)
    s = stats.cpu().double().sum(1)
    assert torch.allclose(s[:, 0], o.sum(1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(s[:, 1], (o * o).sum(1), rtol=1e-4, atol=1e-2)


# ------------------------------------------------------------------ 2. one block, three paths
@pytest.mark.parametrize("cd,cap", [("fp16", 1.5e-3), ("bf16", 1.2e-2)])
@pytest.mark.parametrize("hw,b", [(16, 2), (64, 2)])
def test_project_skip_block_vs_both_other_paths_and_oracle(dev, cd, cap, hw, b):
    """The decoder's 96 -> 32 block (64 + 32 concatenated channels): the unfused pair (irbx 0), expand_dw + project GEMM (irbx 1,
    irbx_project 0) and expand_pool + expand_dw_project (both 1) against the CPU oracle; irbx_project 2 leaves this block to
    expand_dw + project GEMM, bit for bit."""
    name = f"xs_{CIN}_{COUT}_{hw}"
    blk = M.InvertedResidualBlock(CIN, COUT, 128, concat_split=64)
    blk.load_state_dict({k: synth_tensor(name + "." + k, tuple(v.shape)) for k, v in blk.state_dict().items()})
    blk = blk.to(dev)
    blk.compute_dtype = cd
    sd = {name + "." + k: v.detach().cpu() for k, v in blk.state_dict().items()}
    x = synth_input(name + ".x", (b, CIN, hw, hw), -2, 2)
    te = synth_input(name + ".temb", (b, 128), -1, 1)
    ref = unet_ref.irb_forward(sd, name, x, te)
    L = N.lib()
    ys = []
    try:
        for irbx, proj in ((0, 1), (1, 0), (1, 1), (1, 2)):
            N.check(L.llie_tune(b"irbx", irbx))
            N.check(L.llie_tune(b"irbx_project", proj))
            with torch.no_grad():
                ys.append(blk(x.to(dev), te.to(dev)).cpu())
    finally:
        N.check(L.llie_tune(b"irbx", 1))
        N.check(L.llie_tune(b"irbx_project", 1))
    r_unfused, r_pair, r_new = (((y - ref).norm() / ref.norm()).item() for y in ys[:3])
    print(f"relative L2 error vs the oracle: unfused {r_unfused:.3e}, expand_dw + pw_gemm {r_pair:.3e}, project form {r_new:.3e}")
    assert not torch.equal(ys[2], ys[0]) and not torch.equal(ys[2], ys[1])      # really a third set of kernels
    assert r_new < cap and r_new < 1.15 * r_unfused + 1e-5, (r_unfused, r_pair, r_new)
    assert torch.equal(ys[3], ys[1])


# ------------------------------------------------------------------ 3. whole network
def test_project_skip_form_whole_network_properties(dev):
    """small@64 fp16, B = 3: irbx_project 1 (all shapes) against 2 (the identity-residual shapes only) within the bounds of
    test_project_form_whole_network_properties, value 1 bitwise reproducible, and a sample alone equal to its slice of the batch."""
    spec = oracle.make_spec("small", 64)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4, compute_dtype="fp16")
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    L = N.lib()
    gen = torch.Generator().manual_seed(5)
    low = (torch.rand(3, 3, 64, 64, generator=gen) * 2 - 1).to(dev)
    noise = torch.randn(4, 3, 3, 64, 64, generator=gen).to(dev)
    try:
        outs = []
        for v in (2, 1, 1):
            N.check(L.llie_tune(b"irbx_project", v))
            o = m.enhance(low, 4, noise=noise, return_intermediate=True, return_noise_pred=True)
            outs.append((o.noise_pred[0].clone(), o.intermediate[-1].clone(), o.enhanced.clone()))
        assert not torch.equal(outs[0][1], outs[1][1])                          # the knob selects different kernels
        rel = max_abs(outs[0][0].cpu(), outs[1][0].cpu()) / outs[0][0].abs().max().item()
        psnr = psnr01(outs[0][2].cpu(), outs[1][2].cpu())
        print(f"irbx_project 1 vs 2: relative max-abs of noise_pred {rel:.3e}, PSNR of enhanced {psnr:.1f} dB")
        assert rel < 5e-3, rel
        assert psnr > 45.0, psnr
        assert torch.equal(outs[1][1], outs[2][1])
        one = m.enhance(low[1:2], 4, noise=noise[:, 1:2], return_intermediate=True).intermediate[-1]
        assert torch.equal(outs[1][1][1:2], one)
    finally:
        N.check(L.llie_tune(b"irbx_project", 1))
