"""The up-sampling conv from nine low-resolution tap maps on the GPU (csrc/upconv.hip: conv3x3_upmaps_kernel; csrc/engine.h:
upconv_maps_supported), through the C ABI and through the network.  The identity and an emulation with the kernel's rounding
points are pinned in test_upconv_maps_host.py.  TH x TW = 8 x 16 is the kernel's low-resolution tile."""
import functools
import importlib
import math

import pytest
import torch

import oracle
from test_upconv_fold_host import upconv_ref_f64
from test_upconv_maps_host import upconv_maps_f64

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")
U = importlib.import_module("cv-diffusion-model_amd.unet")

TH, TW = 8, 16
DTYPES = [(1, torch.float16), (2, torch.bfloat16)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_upmaps(dev, dtype, tdt, xd, wd, bd, B, H, W, C):
    """-> (out [B][2H * 2W][C], stats [B][tiles][2][C]); buffers NaN-filled first, so anything left unwritten shows."""
    L = N.lib()
    assert L.llie_conv3x3_upmaps_supported(dtype, H, W, C) == 1
    out = torch.full((B, 4 * H * W, C), float("nan"), dtype=tdt, device=dev)
    nt = int(L.llie_conv3x3_tiles(2 * H, 2 * W))
    assert nt == 4 * (H // TH) * (W // TW)
    stats = torch.full((B, nt, 2, C), float("nan"), device=dev)
    N.check(L.llie_conv3x3_upmaps(dtype, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), stats.data_ptr(), B, H, W, C, _stream()),
            "conv3x3_upmaps")
    torch.cuda.synchronize()
    return out, stats


def _run_blend(dev, dtype, tdt, xd, wd, bd, B, H, W, C):
    """The kernel that blends the patch itself (llie_conv3x3 mode 1) on the same inputs and weights."""
    out = torch.full((B, 4 * H * W, C), float("nan"), dtype=tdt, device=dev)
    N.check(N.lib().llie_conv3x3(dtype, 1, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), None, B, H, W, C, C, _stream()), "conv3x3")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _case(C, H, W, tdt, B=2):
    """Inputs and weights rounded to the compute dtype, and the float64 reference (interpolate + conv2d) on them, once per shape.
    -> x NHWC [B][H * W][C] tdt, w [9][C][C] tdt (tap-major, as the kernels read it), bias fp32, ref [B][C][2H][2W] float64."""
    g = torch.Generator().manual_seed(C + 10 * H + W)
    x = torch.randn(B, C, H, W, generator=g).to(tdt)
    w = (torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)).to(tdt)
    b = torch.randn(C, generator=g) * 0.1
    ref = upconv_ref_f64(x.float(), w.float(), b)
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous(), w.permute(2, 3, 0, 1).reshape(9, C, C).contiguous(), b, ref, (x, w)


def _nchw(out, B, H, W, C):
    return out.cpu().double().view(B, 2 * H, 2 * W, C).permute(0, 3, 1, 2)


NEW_C = [32, 64, 96, 160]  # the widths of the contract (C % 32 == 0) that no engine runs: one K chunk, two, and odd chunk counts


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W,C", [(H, W, C) for C in (128, 256) for H, W in [(TH, TW), (2 * TH, 2 * TW), (3 * TH, 3 * TW), (TH, 3 * TW)]] +
                         [(H, W, C) for C in NEW_C for H, W in [(TH, TW), (2 * TH, 2 * TW)]])
def test_upmaps_entry_point_vs_float64(dev, dtype, tdt, C, H, W):
    """llie_conv3x3_upmaps against float64 interpolate + conv2d on inputs and weights rounded to T: one tile (all four edges), 2 x 2
    tiles (every halo crosses a seam), 3 x 3 (a tile with no edge), 1 x 3.  Bound: at most 1.5 x the max-abs error of llie_conv3x3
    mode 1 (the kernel it replaces) on the same inputs; the formulation alone, maps rounded to T, is at 0.98 - 1.13 x, the rest is
    room for another fp32 summation order.  The emulation with the kernel's rounding points is printed beside them.
    C = 32 (a single K chunk: the second operand load is never issued, for this item or the next), 64 (no load inside the K loop),
    96 and 160 (odd chunk counts: the K loop ends on buffer and register set 0) run one tile and 2 x 2 tiles under the same bound;
    measured 0.98 - 1.31 x there (profiles/r25), the emulation giving the kernel's figure in every case."""
    B = 2
    xq, wq, b, ref, (x, w) = _case(C, H, W, tdt)
    xd, wd, bd = xq.to(dev), wq.to(dev), b.to(dev)
    out, stats = _run_upmaps(dev, dtype, tdt, xd, wd, bd, B, H, W, C)
    got = _nchw(out, B, H, W, C)
    old = _nchw(_run_blend(dev, dtype, tdt, xd, wd, bd, B, H, W, C), B, H, W, C)
    emu = upconv_maps_f64(x.float(), w.float(), b, tdt)
    err, err_old, err_emu = (got - ref).abs().max().item(), (old - ref).abs().max().item(), (emu - ref).abs().max().item()
    print(f"C={C} {H}x{W} {tdt}: max-abs error maps {err:.3e}, blending kernel {err_old:.3e} (ratio {err / err_old:.3f}), emulation {err_emu:.3e}")
    assert torch.isfinite(got).all()
    assert err <= 1.5 * err_old, (err, err_old)


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", [(TH, TW), (2 * TH, 2 * TW)])
def test_upmaps_border_is_exact_for_ones(dev, dtype, tdt, H, W):
    """x = 1, w = 1, bias 0, C = 128: every map value, coefficient and partial sum is representable, so the output is exactly
    9 * 128 = 1152 inside, 6 * 128 = 768 on an edge and 4 * 128 = 512 in a corner; a clamp or dropped-term mistake shows as a wrong
    integer."""
    B, C = 2, 128
    xd = torch.ones(B, H * W, C, dtype=tdt, device=dev)
    wd = torch.ones(9, C, C, dtype=tdt, device=dev)
    bd = torch.zeros(C, device=dev)
    out, _ = _run_upmaps(dev, dtype, tdt, xd, wd, bd, B, H, W, C)
    got = out.cpu().float().view(B, 2 * H, 2 * W, C)
    want = torch.full((2 * H, 2 * W), 1152.0)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = 768.0
    want[0, 0] = want[0, -1] = want[-1, 0] = want[-1, -1] = 512.0
    assert torch.equal(got, want.view(1, 2 * H, 2 * W, 1).expand_as(got))


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("C", [128, 256])
def test_upmaps_reproducible_and_batch_invariant(dev, dtype, tdt, C):
    """Two runs are equal bit for bit, and image k alone equals its slice of a batch of 3 (output and statistics)."""
    H, W = 2 * TH, 2 * TW
    xq, wq, b, _, _ = _case(C, H, W, tdt, 3)
    xd, wd, bd = xq.to(dev), wq.to(dev), b.to(dev)
    o1, s1 = _run_upmaps(dev, dtype, tdt, xd, wd, bd, 3, H, W, C)
    o2, s2 = _run_upmaps(dev, dtype, tdt, xd, wd, bd, 3, H, W, C)
    assert torch.equal(o1, o2) and torch.equal(s1, s2)
    for k in range(3):
        oa, sa = _run_upmaps(dev, dtype, tdt, xd[k:k + 1].contiguous(), wd, bd, 1, H, W, C)
        assert torch.equal(oa, o1[k:k + 1]) and torch.equal(sa, s1[k:k + 1]), k


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("C,H,W", [(128, TH, TW), (128, 2 * TH, 2 * TW), (256, TH, 3 * TW)] + [(C, TH, TW) for C in NEW_C])
def test_upmaps_slab_is_written_and_sums_the_rounded_output(dev, dtype, tdt, C, H, W):
    """The slab is pre-filled with NaN: after the launch every entry is finite, and per channel the entries add up to the float64
    sum (sum of squares) of the returned, rounded output within n 2^-24 sum|q| (n 2^-24 sum q^2), n = Ho Wo: the worst case of any
    fp32 summation order of n terms."""
    B = 2
    xq, wq, b, _, _ = _case(C, H, W, tdt)
    out, stats = _run_upmaps(dev, dtype, tdt, xq.to(dev), wq.to(dev), b.to(dev), B, H, W, C)
    st = stats.cpu().double()
    assert torch.isfinite(st).all()
    q = out.cpu().double()
    n = 4 * H * W
    u = n * 2.0 ** -24
    d1 = (st.sum(1)[:, 0] - q.sum(1)).abs()
    d2 = (st.sum(1)[:, 1] - (q * q).sum(1)).abs()
    print(f"C={C} {H}x{W} {tdt}: worst sum error / bound {(d1 / (u * q.abs().sum(1))).max().item():.3f}, squares {(d2 / (u * (q * q).sum(1))).max().item():.3f}")
    assert (d1 <= u * q.abs().sum(1)).all()
    assert (d2 <= u * (q * q).sum(1)).all()


def _up_module(dev, dtype_name, H, W, C, taped=False, knobs=()):
    """One forward of a bare Upsample engine (or, taped, the training forward llie_module_backward re-runs) under the engine's
    profiler, with `knobs` = ((name, value), ...) set for its duration -> the conv kernel names."""
    L = N.lib()
    cfg = U._module_cfg(N.LLIE_UP, C, C)
    cfg.compute_dtype = N.dtype_code(dtype_name)
    h = N.Handle(cfg)
    B = 2
    try:
        for k, v in knobs:
            N.check(L.llie_tune(k, v))
        g = torch.Generator().manual_seed(H * 100 + W)
        shapes = dict(h.params())
        w = torch.randn(shapes["conv.weight"], generator=g) / math.sqrt(9 * C)
        b = torch.randn(shapes["conv.bias"], generator=g) * 0.1
        h.load_all([{"conv.weight": w, "conv.bias": b}[k].to(dev) for k, _ in h.params()], _stream())
        xd = torch.randn(B, C, H, W, generator=g).to(dev)
        h.profile_begin(N.K_CONV3)
        if taped:
            nbytes = h.train_workspace_bytes(B, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dyd, res = torch.randn(B, C, 2 * H, 2 * W, generator=g).to(dev), torch.empty(B, C, H, W, device=dev)
            flat = torch.empty(h.grad_numel(), device=dev)
            N.check(L.llie_module_backward(h.h, xd.data_ptr(), None, dyd.data_ptr(), res.data_ptr(), None, flat.data_ptr(), B, H, W,
                                           ws.data_ptr(), nbytes, _stream()), "backward")
        else:
            nbytes = h.workspace_bytes(B, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            res = torch.empty(B, C, 2 * H, 2 * W, device=dev)
            N.check(L.llie_module_forward(h.h, xd.data_ptr(), None, res.data_ptr(), B, H, W, ws.data_ptr(), nbytes, _stream()), "forward")
        torch.cuda.synchronize()
        assert torch.isfinite(res).all()
        return sorted(k for k in h.profile_report() if k.startswith("conv3x3"))
    finally:
        L.llie_tune(b"upconv_maps", 1)
        L.llie_tune(b"upconv_fold", 1)
        h.close()


def _up_forward(dev, dtype_name, H, W, C, B, chunk):
    """A bare Upsample engine with random weights on B random images: one forward of all B, then the same images in batches of
    at most `chunk`, under the engine's profiler -> (whole, batched: [B][C][2H][2W] fp32 on the CPU; the conv kernel names of the
    whole-batch forward; x [B][C][H][W], w OIHW, bias: fp32 on the CPU)."""
    L = N.lib()
    cfg = U._module_cfg(N.LLIE_UP, C, C)
    cfg.compute_dtype = N.dtype_code(dtype_name)
    h = N.Handle(cfg)
    try:
        g = torch.Generator().manual_seed(H * 100 + W + B)
        shapes = dict(h.params())
        w = torch.randn(shapes["conv.weight"], generator=g) / math.sqrt(9 * C)
        b = torch.randn(shapes["conv.bias"], generator=g) * 0.1
        h.load_all([{"conv.weight": w, "conv.bias": b}[k].to(dev) for k, _ in h.params()], _stream())
        x = torch.randn(B, C, H, W, generator=g)
        xd = x.to(dev)

        def forward(xs):
            n = xs.shape[0]
            nbytes = h.workspace_bytes(n, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            res = torch.full((n, C, 2 * H, 2 * W), float("nan"), device=dev)
            N.check(L.llie_module_forward(h.h, xs.data_ptr(), None, res.data_ptr(), n, H, W, ws.data_ptr(), nbytes, _stream()), "forward")
            torch.cuda.synchronize()
            return res.cpu()

        h.profile_begin(N.K_CONV3)
        whole = forward(xd)
        names = sorted(k for k in h.profile_report() if k.startswith("conv3x3"))
        batched = torch.cat([forward(xd[k:k + chunk].contiguous()) for k in range(0, B, chunk)])
        return whole, batched, names, x, w, b
    finally:
        h.close()


@pytest.mark.parametrize("dtype_name,C,taped,knobs,want", [
    ("fp16", 128, False, (), "conv3x3_upmaps_kernel<"),
    ("bf16", 128, False, (), "conv3x3_upmaps_kernel<"),
    ("fp16", 128, False, ((b"upconv_maps", 0),), "conv3x3_upfold_kernel<"),
    ("fp16", 128, False, ((b"upconv_maps", 0), (b"upconv_fold", 0)), "conv3x3_kernel<"),
    ("fp32", 128, False, (), "conv3x3_kernel<"),
    ("fp16", 128, True, (), "conv3x3_kernel<"),
    ("fp16", 64, False, (), "conv3x3_upfold_kernel<"),
])
def test_rule_picks_the_kernel(dev, dtype_name, C, taped, knobs, want):
    """Which kernel a bare Upsample engine launches on a 16 x 16 map, by the profile report's names: the tap-map kernel at C = 128
    on a 2-byte engine; the folded kernel with upconv_maps = 0 and the blending kernel with both knobs at 0 (what ran before);
    the fp32 engine and the taped forward keep conv3x3_kernel; C = 64 keeps the folded kernel."""
    names = _up_module(dev, dtype_name, 16, 16, C, taped=taped, knobs=knobs)
    assert names and all(n.startswith(want) for n in names), names


def test_rule_keeps_the_blending_kernel_on_ragged_maps(dev):
    """small@96 fp16 (a bare module takes no 12-row map): the 12 x 12 map at C = 256 and the 24 x 24 map at C = 128 have no whole
    8 x 16 tiles and keep conv3x3_kernel."""
    m = M.LowLightDiffusion(unet_variant="small", image_size=96, num_inference_steps=4, compute_dtype="fp16").to(dev).eval()
    low = torch.rand(1, 3, 96, 96, generator=torch.Generator().manual_seed(96)).to(dev) * 2 - 1
    m.enhance(low, 1)
    h = m.unet._prepare(1, dev)[0]
    h.profile_begin(N.K_CONV3)
    m.enhance(low, 1)
    torch.cuda.synchronize()
    ups = {tag: name.split("<")[0] for _cls, name, tag, _ms, _b in h.profile_dump() if tag.startswith("conv3 mode=1")}
    assert ups["conv3 mode=1 C=256 12x12"] == "conv3x3_kernel" and ups["conv3 mode=1 C=128 24x24"] == "conv3x3_kernel", ups


def _psnr01(a, b):
    """PSNR on [0, 1]-denormalised images, MAX = 1 (as in test_gpu_upconv_fold.py)."""
    a = (torch.as_tensor(a).double().clamp(-1, 1) + 1) / 2
    b = (torch.as_tensor(b).double().clamp(-1, 1) + 1) / 2
    mse = ((a - b) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


def test_upconv_maps_whole_network_properties(dev):
    """small@128 fp16, B = 2, 4 steps (C = 256 runs at 16 x 16, C = 128 at 32 x 32), knob 1 against knob 0: the outputs differ
    (different kernels ran), PSNR of `enhanced` above 45 dB (the bar of test_upconv_fold_whole_network_properties), and each
    setting is bitwise equal over eager run, graph capture and replay."""
    spec = oracle.make_spec("small", 128)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    m = M.LowLightDiffusion(unet_variant="small", image_size=128, num_inference_steps=4, compute_dtype="fp16")
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    L = N.lib()
    gen = torch.Generator().manual_seed(24)
    low = (torch.rand(2, 3, 128, 128, generator=gen) * 2 - 1).to(dev)
    noise = torch.randn(4, 2, 3, 128, 128, generator=gen).to(dev)
    try:
        outs = {}
        for v in (0, 1):
            N.check(L.llie_tune(b"upconv_maps", v))
            runs = [m.enhance(low, 4, noise=noise).clone() for _ in range(3)]  # eager, capture, replay
            assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), v
            outs[v] = runs[0]
        assert not torch.equal(outs[0], outs[1])
        psnr = _psnr01(outs[0].cpu(), outs[1].cpu())
        print(f"small@128 fp16 enhanced: tap maps against what ran before {psnr:.2f} dB")
        assert psnr > 45.0, psnr
    finally:
        N.check(L.llie_tune(b"upconv_maps", 1))
