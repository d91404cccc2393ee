"""Tiled enhancement with one latent canvas per image on the MI355X: the sync-step kernel against its NumPy twin (bit for bit,
through the C ABI), `enhance_tiled(sync="latents")` against the host loop with the engine's own denoiser, against `enhance` on
an S x S image and against the CPU oracle, and the default path, which must not change."""
import importlib

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
T = importlib.import_module("cv-diffusion-model_amd.tiling")
native = importlib.import_module("cv-diffusion-model_amd._native")

SHAPES = [(64, 64, 64, 16), (50, 70, 64, 8), (80, 104, 64, 8), (150, 70, 64, 32), (97, 130, 64, 0), (113, 64, 64, 31)]
F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def small64(dev):
    spec = oracle.make_spec("small", 64)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4)
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd, spec


def dark_image(h, w, seed):
    return (np.random.default_rng(seed).random((h, w, 3)) * 90).astype(np.uint8)


def canvas_for(h, w, s, seed, steps=4):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn(3, max(h, s), max(w, s), generator=g) for _ in range(steps)])


def engine_eps(m, dev):
    """eps_fn of the host loop on the engine's own denoiser: all tiles in one forward_split."""
    def eps_fn(lat, low, t):
        tt = torch.full((lat.shape[0],), t, dtype=torch.long, device=dev)
        return m.unet.forward_split(torch.from_numpy(lat).to(dev), torch.from_numpy(low).to(dev), tt, uniform_t=True).cpu().numpy()
    return eps_fn


def host_loop(m, dev, img, v, canvas, eps_fn):
    m.scheduler.set_timesteps(4, device=dev)
    ts = list(m.scheduler._timestep_list)
    coefs = [m.scheduler.step_coefficients(t) for t in ts]
    return T.enhance_tiled_sync_array(eps_fn, img, int(m.image_size), v, coefs, ts, canvas.numpy())


def psnr01(a, b):
    a = (torch.as_tensor(a).double().clamp(-1, 1) + 1) / 2
    b = (torch.as_tensor(b).double().clamp(-1, 1) + 1) / 2
    mse = ((a - b) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * np.log10(1.0 / mse)


# ------------------------------------------------------------------ 1. kernel == twin
@pytest.mark.parametrize("h,w,s,v", SHAPES)
def test_sync_step_kernel_bit_exact(dev, h, w, s, v):
    rng = np.random.default_rng(h * 7 + w)
    total = len(T.tile_origins(h, s, v)) * len(T.tile_origins(w, s, v))
    hc, wc = max(h, s), max(w, s)
    eps = rng.uniform(-4, 4, (total, 3, s, s)).astype(F)
    x, nz = rng.standard_normal((3, hc, wc), dtype=F), rng.standard_normal((3, hc, wc), dtype=F)
    eps_d, x_d, nz_d = (torch.from_numpy(a).to(dev) for a in (eps, x, nz))
    for vpred in (0, 1):
        for clamp in (0, 1):
            for last in (0, 1):
                c = native.StepCoef(0.8, 0.6, 0.9, 0.43, last, vpred, clamp)
                want = T.sync_step_array(eps, (h, w), v, x, None if last else nz, c)
                got = M.sync_step_device(eps_d, (h, w), v, x_d, None if last else nz_d, c)
                assert got.data_ptr() != x_d.data_ptr() and np.array_equal(x_d.cpu().numpy(), x)  # out of place: the input stays
                assert np.array_equal(got.cpu().numpy(), want), (vpred, clamp, last)
                inplace = x_d.clone()
                img = torch.full((h, w, 3), 77, dtype=torch.uint8, device=dev) if last else None
                assert M.sync_step_device(eps_d, (h, w), v, inplace, None if last else nz_d, c, out=inplace, image=img) is inplace
                assert np.array_equal(inplace.cpu().numpy(), want), (vpred, clamp, last, "in place")
                if last:
                    bytes_ = T.canvas_store_array(want, (h, w))
                    assert np.array_equal(img.cpu().numpy(), bytes_)
                    if not clamp:  # eps in +-4 takes x0 past +-1: the clip of the bytes acts at both ends
                        assert bytes_.min() == 0 and bytes_.max() == 255 and 0 < np.median(bytes_) < 255


def test_sync_step_refuses_bad_arguments(dev):
    eps = torch.zeros(4, 3, 64, 64, device=dev)
    x = torch.zeros(3, 80, 104, device=dev)
    img = torch.zeros(80, 104, 3, dtype=torch.uint8, device=dev)
    L = native.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    step, last = native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 0), native.StepCoef(0.8, 0.6, 0.9, 0.43, 1, 0, 0)
    p = (eps.data_ptr(), x.data_ptr(), img.data_ptr())
    assert L.llie_tile_sync_step(p[0], 80, 104, 64, 8, p[1], None, last, p[1], p[2], st) == 0
    assert L.llie_tile_sync_step(p[0], 80, 104, 64, 33, p[1], p[1], step, p[1], None, st) == native.ERR_ARG  # overlap > S / 2
    assert L.llie_tile_sync_step(p[0], 80, 104, 64, -1, p[1], p[1], step, p[1], None, st) == native.ERR_ARG
    assert L.llie_tile_sync_step(p[0], 0, 104, 64, 8, p[1], p[1], step, p[1], None, st) == native.ERR_ARG   # empty image
    assert L.llie_tile_sync_step(p[0], 80, 104, 64, 8, p[1], None, step, p[1], None, st) == native.ERR_ARG  # no noise, not last
    assert L.llie_tile_sync_step(None, 80, 104, 64, 8, p[1], p[1], step, p[1], None, st) == native.ERR_ARG
    assert L.llie_tile_sync_step(p[0], 80, 104, 64, 8, p[1], p[1], None, p[1], None, st) == native.ERR_ARG
    with pytest.raises(ValueError):
        M.sync_step_device(eps[:3], (80, 104), 8, x, x, step)
    with pytest.raises(ValueError):
        M.sync_step_device(eps, (80, 104), 8, x[:, :64].contiguous(), None, last)
    with pytest.raises(ValueError):
        M.sync_step_device(eps, (80, 104), 8, x, None, last, image=img[:64])
    with pytest.raises(ValueError):
        M.sync_step_device(eps, (80, 104), 8, x, None, step)  # the C ABI's refusal as an exception


# ------------------------------------------------------------------ 2. the loop == the host loop on the engine's denoiser
@pytest.mark.parametrize("h,w,s,v", SHAPES)
def test_loop_equals_host_loop(dev, small64, h, w, s, v):
    m = small64[0]
    img = dark_image(h, w, 40 + h)
    canvas = canvas_for(h, w, s, 50 + w)
    before = canvas.clone()
    got, x = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, overlap=v, tile_batch=3, noise=canvas, sync="latents", return_canvas=True)
    want, want_x = host_loop(m, dev, img, v, canvas, engine_eps(m, dev))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3)
    assert x.dtype == torch.float32 and tuple(x.shape) == (3, max(h, s), max(w, s))
    assert np.array_equal(x.cpu().numpy(), want_x)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(canvas, before)  # the caller's noise is read, not stepped
    assert int(want.astype(np.int64).std()) > 0


def test_loop_clamp_mode(dev, small64):
    """LCMDenoisingLoop's coefficients (x0 clamped before re-noising) reach the sync step through step_coefficients."""
    sd = small64[1]
    m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4, scheduler=M.LCMDenoisingLoop())
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    h, w, v = 80, 104, 8
    img = dark_image(h, w, 41)
    canvas = canvas_for(h, w, 64, 51)
    got, x = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, overlap=v, noise=canvas, sync="latents", return_canvas=True)
    want, want_x = host_loop(m, dev, img, v, canvas, engine_eps(m, dev))
    assert m.scheduler.step_coefficients(m.scheduler._timestep_list[0]).clamp_x0 == 1
    assert np.array_equal(x.cpu().numpy(), want_x) and np.array_equal(got.cpu().numpy(), want)
    assert x.abs().max() <= 1.0  # the last step's x0 is clamped


def test_tile_batch_invariance_and_reproducibility(dev, small64):
    m = small64[0]
    h, w, v = 150, 70, 32  # four tiles
    img = torch.from_numpy(dark_image(h, w, 42)).to(dev)
    canvas = canvas_for(h, w, 64, 52).to(dev)
    runs = [M.enhance_tiled(m, img, 4, overlap=v, tile_batch=tb, noise=canvas, sync="latents", return_canvas=True) for tb in (1, 3, 4, 32, 3)]
    for out, x in runs[1:]:
        assert torch.equal(out, runs[0][0]) and torch.equal(x, runs[0][1])
    plain = M.enhance_tiled(m, img, 4, overlap=v, noise=canvas, sync="latents")
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, runs[0][0])
    # another canvas is another image; a generator seeds the canvas as on the default path
    other = M.enhance_tiled(m, img, 4, overlap=v, noise=canvas_for(h, w, 64, 53), sync="latents")
    assert not torch.equal(other, plain)
    torch.manual_seed(9)
    a = M.enhance_tiled(m, img, 4, overlap=v, generator=torch.Generator(device=dev).manual_seed(5), sync="latents")
    torch.manual_seed(9)
    b = M.enhance_tiled(m, img, 4, overlap=v, generator=torch.Generator(device=dev).manual_seed(5), sync="latents")
    assert torch.equal(a, b)


def test_loop_does_not_wait_for_the_device(dev, small64):
    """After a first call (engine workspace, the cached timestep tensors) a whole call enqueues and returns: no host
    synchronisation and no host copy, inside the loop or around it."""
    m = small64[0]
    h, w, v = 80, 104, 8
    img = torch.from_numpy(dark_image(h, w, 46)).to(dev)
    canvas = canvas_for(h, w, 64, 57).to(dev)
    first = M.enhance_tiled(m, img, 4, overlap=v, tile_batch=3, noise=canvas, sync="latents")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # positive control: the mode catches a wait
            first[0, 0, 0].item()
        again, x = M.enhance_tiled(m, img, 4, overlap=v, tile_batch=3, noise=canvas, sync="latents", return_canvas=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(again, first) and bool(torch.isfinite(x).all())


# ------------------------------------------------------------------ 3. an S x S image is `enhance`
def test_single_tile_is_enhance(dev, small64):
    m = small64[0]
    img = torch.from_numpy(dark_image(64, 64, 43)).to(dev)
    canvas = canvas_for(64, 64, 64, 54)
    got, x = M.enhance_tiled(m, img, 4, noise=canvas, sync="latents", return_canvas=True)
    ref = m.enhance(M.preprocess_device(img, 64), 4, noise=canvas[:, None].to(dev), return_intermediate=True)
    err = (x - ref.intermediate[-1][0]).abs().max().item()
    print(f"S x S: canvas vs enhance's last latents, max-abs {err:.3e} (latents up to {x.abs().max().item():.1f})")
    assert err < 1e-3
    default = M.enhance_tiled(m, img, 4, noise=canvas)
    assert (got.int() - default.int()).abs().max().item() <= 1


# ------------------------------------------------------------------ 4. against the CPU oracle
@pytest.fixture(scope="module")
def oracle_loop(dev, small64):
    """80 x 104, four tiles, four steps: the host loop with the CPU oracle as the denoiser (16 forwards at 64 x 64)."""
    m, sd, spec = small64
    h, w, v = 80, 104, 8
    img = dark_image(h, w, 44)
    canvas = canvas_for(h, w, 64, 55)

    def eps_fn(lat, low, t):
        with torch.no_grad():
            tt = torch.full((lat.shape[0],), t, dtype=torch.long)
            return oracle.unet_forward(sd, spec, torch.cat([torch.from_numpy(lat), torch.from_numpy(low)], 1), tt).numpy()

    _, ref_x = host_loop(m, dev, img, v, canvas, eps_fn)
    return img, canvas, v, ref_x


def test_loop_vs_oracle_fp32(dev, small64, oracle_loop):
    m = small64[0]
    img, canvas, v, ref_x = oracle_loop
    _, x = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, overlap=v, noise=canvas, sync="latents", return_canvas=True)
    err = np.abs(x.cpu().numpy() - ref_x).max()
    print(f"80 x 104 fp32: canvas vs the oracle's loop, max-abs {err:.3e} (canvas up to {np.abs(ref_x).max():.1f})")
    assert err < 1e-3


def test_loop_vs_oracle_fp16(dev, small64, oracle_loop):
    m = small64[0]
    img, canvas, v, ref_x = oracle_loop
    m.compute_dtype = "fp16"
    try:
        _, x = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, overlap=v, noise=canvas, sync="latents", return_canvas=True)
    finally:
        m.compute_dtype = None
    p = psnr01(x.cpu(), ref_x)
    print(f"80 x 104 fp16: PSNR of the clamped canvas against the oracle's loop {p:.1f} dB")
    assert p > 40.0


# ------------------------------------------------------------------ 5. the default path and the evaluation keyword
def test_default_is_unchanged(dev, small64):
    m = small64[0]
    h, w, v = 80, 104, 8
    img = dark_image(h, w, 45)
    canvas = canvas_for(h, w, 64, 56)
    img_d = torch.from_numpy(img).to(dev)
    a = M.enhance_tiled(m, img_d, 4, overlap=v, noise=canvas)
    b = M.enhance_tiled(m, img_d, 4, overlap=v, noise=canvas, sync="none")
    assert torch.equal(a, b)
    # and both are still the composition of the parts: gather, `enhance` per tile, blend
    low = T.gather_tiles_array(img, 64, v)
    oys, oxs = T.tile_origins(h, 64, v), T.tile_origins(w, 64, v)
    draws = torch.stack([canvas[:, :, oy:oy + 64, ox:ox + 64] for oy in oys for ox in oxs], dim=1)
    tiles = m.enhance(torch.from_numpy(low).to(dev), 4, noise=draws.to(dev)).cpu().numpy()
    assert np.array_equal(a.cpu().numpy(), T.blend_tiles_array(tiles, (h, w), v))
    assert not torch.equal(a, M.enhance_tiled(m, img_d, 4, overlap=v, noise=canvas, sync="latents"))


def test_evaluate_full_resolution_sync(dev, small64):
    m = small64[0]
    sizes = [(80, 104), (64, 64)]
    low = [dark_image(h, w, 60 + i) for i, (h, w) in enumerate(sizes)]
    high = [np.random.default_rng(70 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(sizes)]
    store = M.DeviceFrameStore(low, high, device=dev)
    with pytest.raises(ValueError, match="sync"):
        M.evaluate_full_resolution(m, store, mode="frame", sync="latents")
    with pytest.raises(ValueError, match="sync"):
        M.evaluate_full_resolution(m, store, sync="pixels")
    res = M.evaluate_full_resolution(m, store, num_inference_steps=4, seed=6, overlap=8, sync="latents")
    g = torch.Generator(device=dev).manual_seed(6)
    for i, (h, w) in enumerate(sizes):
        canvas = torch.randn(4, 3, max(h, 64), max(w, 64), generator=g, device=dev)
        out = M.enhance_tiled(m, store.frame(i), 4, overlap=8, noise=canvas, sync="latents")
        want = M.image_metrics(out, store.frame(len(sizes) + i))
        assert abs(res["per_image"]["psnr"][i] - float(want.psnr)) <= 1e-9
    assert res["psnr"] != M.evaluate_full_resolution(m, store, num_inference_steps=4, seed=6, overlap=8)["psnr"]
