"""The up-sampling conv from folded weights on the GPU (csrc/upconv.hip: conv3x3_upfold_kernel; csrc/small.hip: upconv_fold_kernel;
csrc/engine.h: upconv_fold_supported), through the C ABI and through the network.  The float64 fold and its identity are pinned in
test_upconv_fold_host.py, whose helpers are reused here.  TH x TW = 8 x 16 is the kernel's low-resolution tile."""
import functools
import importlib
import math

import pytest
import torch

import oracle
from test_upconv_fold_host import fold_blob_f64, upconv_ref_f64

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")
U = importlib.import_module("cv-diffusion-model_amd.unet")

TH, TW = 8, 16
DTYPES = [(1, torch.float16, 4e-3), (2, torch.bfloat16, 3e-2)]  # tolerances of test_conv3x3_entry_point_vs_torch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nhwc(x, tdt):
    return x.permute(0, 2, 3, 1).contiguous().to(tdt)


def _fold_on_device(dev, dtype, tdt, w):
    L = N.lib()
    C = w.shape[0]
    n = int(L.llie_upconv_fold_elems(C))
    assert n == 64 * C * C
    blob = torch.full((n,), float("nan"), dtype=tdt, device=dev)
    wd = w.float().contiguous().to(dev)
    N.check(L.llie_upconv_fold_weights(dtype, wd.data_ptr(), blob.data_ptr(), C, torch.cuda.current_stream().cuda_stream), "fold")
    return blob


def _run_upfold(dev, dtype, tdt, xd, blob, bd, B, H, W, C):
    """-> (out [B][2H * 2W][C], stats [B][tiles][2][C]); buffers NaN-filled first, so anything left unwritten shows."""
    L = N.lib()
    out = torch.full((B, 4 * H * W, C), float("nan"), dtype=tdt, device=dev)
    nt = int(L.llie_conv3x3_upfold_tiles(2 * H, 2 * W))
    stats = torch.full((B, nt, 2, C), float("nan"), device=dev)
    N.check(L.llie_conv3x3_upfold(dtype, xd.data_ptr(), blob.data_ptr(), bd.data_ptr(), out.data_ptr(), stats.data_ptr(), B, H, W, C,
                                  torch.cuda.current_stream().cuda_stream), "conv3x3_upfold")
    torch.cuda.synchronize()
    return out, stats


def _run_blend(dev, dtype, tdt, xd, w, bd, B, H, W, C):
    """The kernel that blends the patch itself (llie_conv3x3 mode 1) on the same inputs, weights rounded to the compute dtype."""
    L = N.lib()
    wd = w.permute(2, 3, 0, 1).reshape(9, C, C).contiguous().to(tdt).to(dev)
    out = torch.full((B, 4 * H * W, C), float("nan"), dtype=tdt, device=dev)
    N.check(L.llie_conv3x3(dtype, 1, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), None, B, H, W, C, C,
                           torch.cuda.current_stream().cuda_stream), "conv3x3")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _case(C, H, W, tdt, B=2):
    """Inputs and the float64 reference (interpolate + conv2d of the 16-bit-rounded x and the fp32 w), computed once per shape."""
    g = torch.Generator().manual_seed(C + 10 * H + W)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(C, generator=g) * 0.1
    xq = _nhwc(x, tdt)
    ref = upconv_ref_f64(xq.float().permute(0, 3, 1, 2), w, b)
    return xq, w, b, ref


@pytest.mark.parametrize("dtype,tdt,mant", [(1, torch.float16, 10), (2, torch.bfloat16, 7)])
def test_device_fold_within_one_ulp_of_float64(dev, dtype, tdt, mant):
    """upconv_fold_kernel against the float64 fold, C = 64: every element within one ulp of the compute dtype."""
    g = torch.Generator().manual_seed(64)
    w = torch.randn(64, 64, 3, 3, generator=g) / math.sqrt(9 * 64)
    got = _fold_on_device(dev, dtype, tdt, w).cpu().double().view(64, 64, 64)
    ref = fold_blob_f64(w)
    min_normal = 2.0 ** -14 if tdt == torch.float16 else 2.0 ** -126
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(min_normal))) - mant)
    worst = ((got - ref).abs() / ulp).max().item()
    print(f"device fold {tdt}: worst error {worst:.3f} ulp")
    assert torch.isfinite(got).all()
    assert worst <= 1.0, worst


SHAPES = [(C, h * TH, w * TW) for C in (64, 128) for h, w in ((1, 1), (2, 2), (3, 3), (1, 3))] + [(256, TH, TW)]


@pytest.mark.parametrize("dtype,tdt,tol", DTYPES)
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_upfold_entry_point_vs_float64(dev, dtype, tdt, tol, C, H, W):
    """llie_conv3x3_upfold on a device-folded blob against float64 interpolate + conv2d: one tile (all four edges and corners), 2 x 2
    tiles (every tile holds two edges), 3 x 3 (a tile with no edge), 1 x 3, at C = 64 and 128, and C = 256 (eight K chunks)."""
    B = 2
    xq, w, b, ref = _case(C, H, W, tdt)
    xd, bd = xq.to(dev), b.to(dev)
    out, stats = _run_upfold(dev, dtype, tdt, xd, _fold_on_device(dev, dtype, tdt, w), bd, B, H, W, C)
    got = out.cpu().double().view(B, 2 * H, 2 * W, C).permute(0, 3, 1, 2)
    old = _run_blend(dev, dtype, tdt, xd, w, bd, B, H, W, C).cpu().double().view(B, 2 * H, 2 * W, C).permute(0, 3, 1, 2)
    err, err_old, bound = (got - ref).abs().max().item(), (old - ref).abs().max().item(), tol * max(1.0, ref.abs().max().item())
    print(f"C={C} {H}x{W} {tdt}: max-abs error folded {err:.3e}, blending kernel {err_old:.3e}, bound {bound:.3e}")
    assert torch.isfinite(got).all()
    assert err < bound, err
    o = out.cpu().double()
    assert torch.allclose(stats.cpu().double().sum(1)[:, 0], o.sum(1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(stats.cpu().double().sum(1)[:, 1], (o * o).sum(1), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("dtype,tdt", [(1, torch.float16), (2, torch.bfloat16)])
@pytest.mark.parametrize("H,W", [(TH, TW), (2 * TH, 2 * TW)])
def test_upfold_border_is_exact_for_ones(dev, dtype, tdt, H, W):
    """x = 1, w = 1, bias 0, C = 64: every coefficient and partial sum is representable, so the output is exactly 9 * 64 = 576
    inside, 6 * 64 = 384 on the ring and 4 * 64 = 256 at the corners; a clamp or zero-padding mistake shows as a wrong integer."""
    B, C = 2, 64
    xd = torch.ones(B, H * W, C, dtype=tdt, device=dev)
    bd = torch.zeros(C, device=dev)
    out, _ = _run_upfold(dev, dtype, tdt, xd, _fold_on_device(dev, dtype, tdt, torch.ones(C, C, 3, 3)), bd, B, H, W, C)
    got = out.cpu().float().view(B, 2 * H, 2 * W, C)
    want = torch.full((2 * H, 2 * W), 576.0)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = 384.0
    want[0, 0] = want[0, -1] = want[-1, 0] = want[-1, -1] = 256.0
    assert torch.equal(got, want.view(1, 2 * H, 2 * W, 1).expand_as(got))


@pytest.mark.parametrize("dtype,tdt", [(1, torch.float16), (2, torch.bfloat16)])
@pytest.mark.parametrize("C", [64, 128])
def test_upfold_reproducible_and_batch_invariant(dev, dtype, tdt, C):
    """Two runs are equal bit for bit, and a sample alone equals its slice of B = 3 (output and statistics)."""
    H, W = 2 * TH, 2 * TW
    xq, w, b, _ = _case(C, H, W, tdt, 3)
    xd, bd = xq.to(dev), b.to(dev)
    blob = _fold_on_device(dev, dtype, tdt, w)
    o1, s1 = _run_upfold(dev, dtype, tdt, xd, blob, bd, 3, H, W, C)
    o2, s2 = _run_upfold(dev, dtype, tdt, xd, blob, bd, 3, H, W, C)
    assert torch.equal(o1, o2) and torch.equal(s1, s2)
    oa, sa = _run_upfold(dev, dtype, tdt, xd[1:2].contiguous(), blob, bd, 1, H, W, C)
    assert torch.equal(oa, o1[1:2]) and torch.equal(sa, s1[1:2])


def _up_module(dev, dtype_name, H, W, C=64, taped=False, knob=1):
    """One forward of a bare Upsample engine (or, taped, the training forward llie_module_backward re-runs) under the engine's
    profiler -> (conv kernel names, y or dx, x, w, b)."""
    L = N.lib()
    cfg = U._module_cfg(N.LLIE_UP, C, C)
    cfg.compute_dtype = N.dtype_code(dtype_name)
    h = N.Handle(cfg)
    B = 2
    try:
        N.check(L.llie_tune(b"upconv_fold", knob))
        g = torch.Generator().manual_seed(H * 100 + W)
        stream = torch.cuda.current_stream(dev).cuda_stream
        shapes = dict(h.params())
        w = torch.randn(shapes["conv.weight"], generator=g) / math.sqrt(9 * C)
        b = torch.randn(shapes["conv.bias"], generator=g) * 0.1
        params = [{"conv.weight": w, "conv.bias": b}[k].to(dev) for k, _ in h.params()]
        h.load_all(params, stream)
        x = torch.randn(B, C, H, W, generator=g)
        xd = x.to(dev)
        h.profile_begin(N.K_CONV3)
        if taped:
            nbytes = h.train_workspace_bytes(B, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dy = torch.randn(B, C, 2 * H, 2 * W, generator=g)
            dyd, res = dy.to(dev), torch.empty(B, C, H, W, device=dev)
            flat = torch.empty(h.grad_numel(), device=dev)
            N.check(L.llie_module_backward(h.h, xd.data_ptr(), None, dyd.data_ptr(), res.data_ptr(), None, flat.data_ptr(), B, H, W,
                                           ws.data_ptr(), nbytes, stream), "backward")
            x = (x, dy)
        else:
            nbytes = h.workspace_bytes(B, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            res = torch.empty(B, C, 2 * H, 2 * W, device=dev)
            N.check(L.llie_module_forward(h.h, xd.data_ptr(), None, res.data_ptr(), B, H, W, ws.data_ptr(), nbytes, stream), "forward")
        torch.cuda.synchronize()
        names = sorted(k for k in h.profile_report() if k.startswith("conv3x3"))
        return names, res.cpu().double(), x, w, b
    finally:
        L.llie_tune(b"upconv_fold", 1)
        h.close()


@pytest.mark.parametrize("dtype_name,tdt,tol,H,W,knob,new", [
    ("fp16", torch.float16, 4e-3, 16, 16, 1, True),    # whole tiles, 2-byte engine: the folded kernel
    ("fp32", torch.float32, 2e-5, 16, 16, 1, False),   # the fp32 engine
    ("fp16", torch.float16, 4e-3, 16, 16, 0, False),   # the knob
])
def test_rule_picks_the_kernel(dev, dtype_name, tdt, tol, H, W, knob, new):
    """Which kernel an Upsample engine launches (by the profile report's names), and that its result matches float64 as before."""
    names, y, x, w, b = _up_module(dev, dtype_name, H, W, knob=knob)
    assert len(names) == 1 and names[0].startswith("conv3x3_upfold_kernel<" if new else "conv3x3_kernel<"), names
    ref = upconv_ref_f64(x.to(tdt).float(), w, b)
    err = (y - ref).abs().max().item()
    print(f"{dtype_name} {H}x{W} knob {knob}: {names[0]}, max-abs error {err:.3e}")
    assert err < tol * max(1.0, ref.abs().max().item()), err


def test_rule_keeps_the_blending_kernel_on_ragged_maps(dev):
    """small@96 fp16 (a bare module takes no 12-row map): the 12 x 12 and 24 x 24 maps have no whole 8 x 16 tiles and keep
    conv3x3_kernel, the 48 x 48 map runs the folded kernel.  (That these sizes still match the oracle is the business of
    test_gpu_round2.py's ragged-size tests.)"""
    m = M.LowLightDiffusion(unet_variant="small", image_size=96, num_inference_steps=4, compute_dtype="fp16").to(dev).eval()
    low = torch.rand(1, 3, 96, 96, generator=torch.Generator().manual_seed(96)).to(dev) * 2 - 1
    m.enhance(low, 1)
    h = m.unet._prepare(1, dev)[0]
    h.profile_begin(N.K_CONV3)
    m.enhance(low, 1)
    torch.cuda.synchronize()
    ups = {tag: name.split("<")[0] for _cls, name, tag, _ms, _b in h.profile_dump() if tag.startswith("conv3 mode=1")}
    assert ups == {"conv3 mode=1 C=256 12x12": "conv3x3_kernel", "conv3 mode=1 C=128 24x24": "conv3x3_kernel",
                   "conv3 mode=1 C=64 48x48": "conv3x3_upfold_kernel"}, ups


def test_rule_keeps_the_blending_kernel_on_the_training_tape(dev):
    """A taped forward (it keeps the up-sampled tensor for the weight gradient) runs the plain stride-1 conv3x3_kernel, and its
    input gradient matches float64 autograd within the fp16 bound of test_gpu_training.py's "up" module (relative L2 0.0014)."""
    names, dx, (x, dy), w, b = _up_module(dev, "fp16", 16, 16, taped=True)
    assert names and all(n.startswith("conv3x3_kernel<") for n in names), names
    xr = x.double().requires_grad_(True)
    upconv_ref_f64(xr, w, b).backward(dy.double())
    rel = ((dx - xr.grad).norm() / xr.grad.norm()).item()
    assert rel < 0.0014, rel


def _psnr01(a, b):
    """PSNR on [0, 1]-denormalised images, MAX = 1 (as in test_gpu_expand_dw_project.py)."""
    a = (torch.as_tensor(a).double().clamp(-1, 1) + 1) / 2
    b = (torch.as_tensor(b).double().clamp(-1, 1) + 1) / 2
    mse = ((a - b) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


def test_upconv_fold_whole_network_properties(dev):
    """small@64 fp16, knob 1 against knob 0: different kernels ran, PSNR of `enhanced` above 45 dB (the bar of
    test_project_form_whole_network_properties), each path bitwise reproducible over eager run and graph replays, and after
    load_state_dict with changed upsamplers.* weights the model equals a freshly built one bit for bit."""
    spec = oracle.make_spec("small", 64)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))

    def build(state):
        m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4, compute_dtype="fp16")
        m.load_state_dict(state)
        return m.to(dev).eval()

    m = build(sd)
    L = N.lib()
    gen = torch.Generator().manual_seed(9)
    low = (torch.rand(3, 3, 64, 64, generator=gen) * 2 - 1).to(dev)
    noise = torch.randn(4, 3, 3, 64, 64, generator=gen).to(dev)
    try:
        outs = {}
        for v in (0, 1):
            N.check(L.llie_tune(b"upconv_fold", v))
            runs = [m.enhance(low, 4, noise=noise).clone() for _ in range(3)]  # eager, capture, replay
            assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), v
            outs[v] = runs[0]
        assert not torch.equal(outs[0], outs[1])
        psnr = _psnr01(outs[0].cpu(), outs[1].cpu())
        print(f"small@64 fp16 enhanced: folded against blending kernel {psnr:.2f} dB")
        assert psnr > 45.0, psnr
        sd2 = {k: (v * 1.25 + 0.01 if "upsamplers." in k else v).clone() for k, v in sd.items()}
        assert sum(not torch.equal(sd2[k], sd[k]) for k in sd) == 6  # three convs: weight and bias
        m.load_state_dict(sd2)
        after = m.enhance(low, 4, noise=noise).clone()
        fresh = build(sd2).enhance(low, 4, noise=noise).clone()
        assert not torch.equal(after, outs[1])
        assert torch.equal(after, fresh)
    finally:
        N.check(L.llie_tune(b"upconv_fold", 1))
