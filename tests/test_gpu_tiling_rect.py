"""Frame-sized rectangular tiles on the MI355X: the four per-axis tile kernels (`llie_tile_*_hw`) against their NumPy twins, bit
for bit; the square entries against the new ones; `enhance_tiled(tile=(TH, TW))` against the same path composed by hand from the
twins and `model.enhance_frame`, and with sync="latents" against the host loop on the engine's own frame forward and on the CPU
oracle; tile="auto"; the refusals, the CLI and `evaluate_full_resolution(tile=)`.  small at image_size 64 throughout."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
T = importlib.import_module("cv-diffusion-model_amd.tiling")
native = importlib.import_module("cv-diffusion-model_amd._native")
F = np.float32

# (H, W, TH, TW, vy, vx)
CASES = [(150, 233, 64, 96, 8, 12), (100, 80, 72, 104, 0, 0), (64, 96, 64, 96, 32, 48), (97, 131, 50, 75, 7, 9),
         (130, 70, 64, 64, 16, 16), (201, 333, 96, 64, 48, 9)]
PLAN = (150, 233, (64, 96), (8, 12))  # 3 x 3 tiles: chunks of 4, 4 and 1 at tile_batch 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_model(dev, **kw):
    spec = oracle.make_spec("small", 64)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4, **kw)
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd, spec


@pytest.fixture(scope="module")
def small64(dev):
    return make_model(dev)


def dark_image(h, w, seed):
    return (np.random.default_rng(seed).random((h, w, 3)) * 90).astype(np.uint8)


def canvas_for(h, w, tile, seed, steps=4):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn(3, max(h, tile[0]), max(w, tile[1]), generator=g) for _ in range(steps)])


def origins_of(h, w, tile, overlap):
    return [(oy, ox) for oy in T.tile_origins(h, tile[0], overlap[0]) for ox in T.tile_origins(w, tile[1], overlap[1])]


def noise_tiles_host(canvas, h, w, tile, overlap):
    """[steps,3,Hc,Wc] -> [steps,T,3,TH,TW] by plain slicing."""
    return np.stack([canvas[:, :, oy:oy + tile[0], ox:ox + tile[1]] for oy, ox in origins_of(h, w, tile, overlap)], axis=1)


class compute_dtype:
    def __init__(self, m, cd):
        self.m, self.cd = m, cd

    def __enter__(self):
        self.m.compute_dtype = self.cd

    def __exit__(self, *exc):
        self.m.compute_dtype = None


def frame_eps(m, dev):
    """eps_fn of the host loop on the engine's own denoiser at the tile's size: all tiles in one forward_split(frame=True)."""
    def eps_fn(lat, low, t):
        tt = torch.full((lat.shape[0],), t, dtype=torch.long, device=dev)
        return m.unet.forward_split(torch.from_numpy(lat).to(dev), torch.from_numpy(low).to(dev), tt, uniform_t=True,
                                    frame=True).cpu().numpy()
    return eps_fn


def host_loop(m, dev, img, tile, overlap, canvas, eps_fn, sampler="lcm"):
    if sampler == "ddim":
        ts, coefs = m.ddim_schedule(4)
    else:
        m.scheduler.set_timesteps(4, device=dev)
        ts = list(m.scheduler._timestep_list)
        coefs = [m.scheduler.step_coefficients(t) for t in ts]
    return T.enhance_tiled_sync_array(eps_fn, img, tile, overlap, coefs, ts, canvas.numpy(), sampler=sampler)


def psnr01(a, b):
    a = (torch.as_tensor(a).double().clamp(-1, 1) + 1) / 2
    b = (torch.as_tensor(b).double().clamp(-1, 1) + 1) / 2
    mse = ((a - b) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * np.log10(1.0 / mse)


# ------------------------------------------------------------------ 1. the four kernels == their twins
@pytest.mark.parametrize("h,w,th,tw,vy,vx", CASES)
def test_gather_and_blend_kernels_bit_exact(dev, h, w, th, tw, vy, vx):
    tile, v = (th, tw), (vy, vx)
    rng = np.random.default_rng(h * 7 + w)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img_d = torch.from_numpy(img).to(dev)
    ref = T.gather_tiles_array(img, tile, v)
    total = ref.shape[0]
    got = M.gather_tiles_device(img_d, tile, v)
    assert got.dtype == torch.float32 and tuple(got.shape) == (total, 3, th, tw) and np.array_equal(got.cpu().numpy(), ref)
    step = max(1, (total + 2) // 3)  # three chunks that together are the whole, the last one short
    firsts = list(range(0, total, step))
    parts = [M.gather_tiles_device(img_d, tile, v, first, min(step, total - first)) for first in firsts]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), ref)

    hc, wc = max(h, th), max(w, tw)
    canvas = rng.standard_normal((2, 3, hc, wc), dtype=F)
    canvas_d = torch.from_numpy(canvas).to(dev)
    nref = noise_tiles_host(canvas, h, w, tile, v)
    assert np.array_equal(M.gather_noise_device(canvas_d, (h, w), tile, v).cpu().numpy(), nref)
    nparts = [M.gather_noise_device(canvas_d, (h, w), tile, v, first, min(step, total - first)) for first in firsts]
    assert np.array_equal(torch.cat(nparts, dim=1).cpu().numpy(), nref)

    tiles = rng.random((total, 3, th, tw), dtype=F) * F(2.4) - F(1.2)  # the clip acts
    want = T.blend_tiles_array(tiles, (h, w), v)
    out = M.blend_tiles_device(torch.from_numpy(tiles).to(dev), (h, w), v)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(M.blend_tiles_device(got, (h, w), v).cpu().numpy(), T.blend_tiles_array(ref, (h, w), v))


@pytest.mark.parametrize("h,w,th,tw,vy,vx", CASES)
def test_sync_step_kernel_bit_exact(dev, h, w, th, tw, vy, vx):
    v = (vy, vx)
    rng = np.random.default_rng(h * 11 + w)
    total = len(origins_of(h, w, (th, tw), v))
    hc, wc = max(h, th), max(w, tw)
    eps = rng.uniform(-4, 4, (total, 3, th, tw)).astype(F)
    x, nz = rng.standard_normal((3, hc, wc), dtype=F), rng.standard_normal((3, hc, wc), dtype=F)
    eps_d, x_d, nz_d = (torch.from_numpy(a).to(dev) for a in (eps, x, nz))
    for sampler in (native.SAMPLER_LCM, native.SAMPLER_DDIM):
        for vpred in (0, 1):
            for last in (0, 1):
                c = native.StepCoef(0.8, 0.6, 0.9, 0.43, last, vpred, 0, sampler)
                draw, draw_d = (None, None) if last or sampler else (nz, nz_d)
                want = T.sync_step_array(eps, (h, w), v, x, draw, c)
                got = M.sync_step_device(eps_d, (h, w), v, x_d, draw_d, c)
                assert np.array_equal(x_d.cpu().numpy(), x)  # out of place: the input stays
                assert np.array_equal(got.cpu().numpy(), want), (sampler, vpred, last)
                inplace = x_d.clone()  # canvas_out == canvas_in
                img = torch.full((h, w, 3), 77, dtype=torch.uint8, device=dev) if last else None
                assert M.sync_step_device(eps_d, (h, w), v, inplace, draw_d, c, out=inplace, image=img) is inplace
                assert np.array_equal(inplace.cpu().numpy(), want), (sampler, vpred, last, "in place")
                if last:
                    assert np.array_equal(img.cpu().numpy(), T.canvas_store_array(want, (h, w)))


# ------------------------------------------------------------------ 2. the square entries are the new ones at SH = SW, vy = vx
@pytest.mark.parametrize("h,w,s,v", [(130, 70, 64, 16), (300, 500, 64, 16)])
def test_square_entries_unchanged(dev, h, w, s, v):
    L = native.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(h + w)
    img = torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).to(dev)
    total = len(origins_of(h, w, (s, s), (v, v)))
    hc, wc = max(h, s), max(w, s)
    a, b = (torch.zeros(total, 3, s, s, device=dev) for _ in range(2))
    assert L.llie_tile_gather_u8(img.data_ptr(), h, w, s, v, 0, total, a.data_ptr(), st) == 0
    assert L.llie_tile_gather_u8_hw(img.data_ptr(), h, w, s, s, v, v, 0, total, b.data_ptr(), st) == 0
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), T.gather_tiles_array(img.cpu().numpy(), s, v))
    canvas = torch.from_numpy(rng.standard_normal((2, 3, hc, wc), dtype=F)).to(dev)
    na, nb = (torch.zeros(2, total - 1, 3, s, s, device=dev) for _ in range(2))
    assert L.llie_tile_gather_f32(canvas.data_ptr(), 6, h, w, s, v, 1, total - 1, na.data_ptr(), st) == 0
    assert L.llie_tile_gather_f32_hw(canvas.data_ptr(), 6, h, w, s, s, v, v, 1, total - 1, nb.data_ptr(), st) == 0
    assert torch.equal(na, nb) and float(na.abs().sum()) > 0
    tiles = torch.from_numpy(rng.uniform(-1.2, 1.2, (total, 3, s, s)).astype(F)).to(dev)
    ia, ib = (torch.zeros(h, w, 3, dtype=torch.uint8, device=dev) for _ in range(2))
    assert L.llie_tile_blend_u8(tiles.data_ptr(), h, w, s, v, ia.data_ptr(), st) == 0
    assert L.llie_tile_blend_u8_hw(tiles.data_ptr(), h, w, s, s, v, v, ib.data_ptr(), st) == 0
    assert torch.equal(ia, ib) and np.array_equal(ia.cpu().numpy(), T.blend_tiles_array(tiles.cpu().numpy(), (h, w), v))
    x = canvas[0].contiguous()
    for c in (native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 0), native.StepCoef(0.8, 0.6, 0.9, 0.43, 1, 1, 0),
              native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 1, 0, native.SAMPLER_DDIM)):
        xa, xb = torch.zeros_like(x), torch.zeros_like(x)
        ia.zero_(), ib.zero_()
        assert L.llie_tile_sync_step(tiles.data_ptr(), h, w, s, v, x.data_ptr(), canvas[1].data_ptr(), c, xa.data_ptr(), ia.data_ptr(), st) == 0
        assert L.llie_tile_sync_step_hw(tiles.data_ptr(), h, w, s, s, v, v, x.data_ptr(), canvas[1].data_ptr(), c, xb.data_ptr(),
                                        ib.data_ptr(), st) == 0
        assert torch.equal(xa, xb) and torch.equal(ia, ib) and float(xa.abs().sum()) > 0


# ------------------------------------------------------------------ 3. tile=(TH, TW) == the hand composition
@pytest.mark.parametrize("cd", ["fp32", "fp16"])
def test_enhance_tiled_equals_hand_composition(dev, small64, cd):
    m = small64[0]
    h, w, tile, v = PLAN
    tb = 4
    img = dark_image(h, w, 21)
    canvas = canvas_for(h, w, tile, 31)
    with compute_dtype(m, cd):
        got = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, tile=tile, overlap=v, tile_batch=tb, noise=canvas)
        low = T.gather_tiles_array(img, tile, v)
        draws = noise_tiles_host(canvas.numpy(), h, w, tile, v)
        total = low.shape[0]
        assert total == 9  # 3 x 3 tiles: chunks of 4, 4 and 1
        outs = []
        for first in range(0, total, tb):
            sl = slice(first, min(first + tb, total))
            outs.append(m.enhance_frame(torch.from_numpy(low[sl]).to(dev), 4, noise=torch.from_numpy(draws[:, sl]).to(dev)).cpu().numpy())
        want = T.blend_tiles_array(np.concatenate(outs), (h, w), v)
        default_overlap = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, tile=tile, tile_batch=tb, noise=canvas)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(default_overlap, got)  # (TH // 8, TW // 8) = (8, 12)
    assert int(want.astype(np.int64).std()) > 0  # not a constant image


# ------------------------------------------------------------------ 4. sync="latents" == the host loop on the engine's frame forward
@pytest.mark.parametrize("sampler", ["lcm", "ddim"])
def test_sync_loop_equals_host_loop(dev, small64, sampler):
    m = small64[0]
    h, w, tile, v = PLAN
    img = dark_image(h, w, 22)
    canvas = canvas_for(h, w, tile, 32, steps=1 if sampler == "ddim" else 4)
    before = canvas.clone()
    got, x = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, tile=tile, overlap=v, tile_batch=4, noise=canvas, sync="latents",
                             return_canvas=True, sampler=sampler)
    want, want_x = host_loop(m, dev, img, tile, v, canvas, frame_eps(m, dev), sampler)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3)
    assert x.dtype == torch.float32 and tuple(x.shape) == (3, h, w)
    assert np.array_equal(x.cpu().numpy(), want_x)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(canvas, before)  # the caller's noise is read, not stepped
    assert int(want.astype(np.int64).std()) > 0


# ------------------------------------------------------------------ 5. tile=(S, S) is tile=None
def test_square_tile_is_the_default_path(dev, small64):
    m = small64[0]
    h, w = 150, 200
    img = torch.from_numpy(dark_image(h, w, 23)).to(dev)
    canvas = canvas_for(h, w, (64, 64), 33)
    for sync in ("none", "latents"):
        for kw in ({}, {"overlap": 16}):
            a = M.enhance_tiled(m, img, 4, tile_batch=5, noise=canvas, sync=sync, **kw)
            b = M.enhance_tiled(m, img, 4, tile=(64, 64), tile_batch=5, noise=canvas, sync=sync, **kw)
            assert torch.equal(a, b), (sync, kw)
    # and the default path is still the composition of its parts: gather, `enhance` per chunk, blend
    low = T.gather_tiles_array(img.cpu().numpy(), 64, 16)
    draws = noise_tiles_host(canvas.numpy(), h, w, (64, 64), (16, 16))
    outs = [m.enhance(torch.from_numpy(low[f:f + 5]).to(dev), 4, noise=torch.from_numpy(draws[:, f:f + 5]).to(dev)).cpu().numpy()
            for f in range(0, low.shape[0], 5)]
    want = T.blend_tiles_array(np.concatenate(outs), (h, w), 16)
    assert np.array_equal(M.enhance_tiled(m, img, 4, overlap=16, tile_batch=5, noise=canvas).cpu().numpy(), want)


# ------------------------------------------------------------------ 6. tile_batch, repeated calls, the graph cache
def test_tile_batch_invariance_and_graph_cache(dev):
    m = make_model(dev)[0]
    h, w, tile, v = PLAN
    img = torch.from_numpy(dark_image(h, w, 24)).to(dev)
    canvas = canvas_for(h, w, tile, 34).to(dev)
    L = native.lib()
    runs = {}
    for tb in (32, 4, 1):  # 9 tiles: one call of 9, then 4 + 4 + 1, then nine calls of 1; the workspace is sized by the first
        runs[tb] = M.enhance_tiled(m, img, 4, tile=tile, overlap=v, tile_batch=tb, noise=canvas)
    assert torch.equal(runs[4], runs[32]) and torch.equal(runs[1], runs[32])
    handle = m.unet._prepare(1, dev)[0]
    entries = L.llie_graph_cache_entries(handle.h)
    assert entries == 3  # one per (batch, shape): 9, 4 and 1 frames of 64 x 96
    for _ in range(3):  # three identical calls, and the cache stays
        for tb in (32, 4, 1):
            assert torch.equal(M.enhance_tiled(m, img, 4, tile=tile, overlap=v, tile_batch=tb, noise=canvas), runs[32])
        assert L.llie_graph_cache_entries(handle.h) == entries
    synced = [M.enhance_tiled(m, img, 4, tile=tile, overlap=v, tile_batch=tb, noise=canvas, sync="latents", return_canvas=True)
              for tb in (1, 4, 32, 4)]
    for out, x in synced[1:]:
        assert torch.equal(out, synced[0][0]) and torch.equal(x, synced[0][1])
    assert not torch.equal(synced[0][0], runs[32])


# ------------------------------------------------------------------ 7. an image that is one frame
def test_single_frame_is_enhance_frame(dev, small64):
    m = small64[0]
    h, w = 72, 104
    img = torch.from_numpy(dark_image(h, w, 25)).to(dev)
    canvas = canvas_for(h, w, (h, w), 35)
    got, x = M.enhance_tiled(m, img, 4, tile=(h, w), noise=canvas, sync="latents", return_canvas=True)
    ref = m.enhance_frame(M.frame_load_device(img)[None], 4, noise=canvas[:, None].to(dev), return_intermediate=True)
    err = (x - ref.intermediate[-1][0]).abs().max().item()
    print(f"72 x 104, one tile: canvas vs enhance_frame's last latents, max-abs {err:.3e} (latents up to {x.abs().max().item():.1f})")
    assert torch.equal(x, ref.intermediate[-1][0])
    assert torch.equal(got, M.frame_store_device(ref.intermediate[-1][0], (h, w)))
    # without sync the one tile still goes through the blend's num / den: within one byte step of the frame's own store
    plain = M.enhance_tiled(m, img, 4, tile=(h, w), noise=canvas)
    assert (plain.int() - M.enhance_frame_u8(m, img, 4, noise=canvas).int()).abs().max().item() <= 1


# ------------------------------------------------------------------ 8. tile="auto"
def test_auto_tile(dev, small64):
    m = small64[0]
    h, w = 150, 233
    img = dark_image(h, w, 26)
    img_d = torch.from_numpy(img).to(dev)
    canvas = canvas_for(h, w, (80, 88), 36)
    auto = M.enhance_tiled(m, img_d, 4, tile="auto", max_tile_pixels=8192, noise=canvas)
    assert M.auto_tile_plan((h, w), 8192) == ((80, 88), (10, 11))
    assert torch.equal(auto, M.enhance_tiled(m, img_d, 4, tile=(80, 88), overlap=(10, 11), noise=canvas))
    a2, x2 = M.enhance_tiled(m, img_d, 4, tile="auto", max_tile_pixels=8192, noise=canvas, sync="latents", return_canvas=True)
    b2, y2 = M.enhance_tiled(m, img_d, 4, tile=(80, 88), noise=canvas, sync="latents", return_canvas=True)
    assert torch.equal(a2, b2) and torch.equal(x2, y2) and tuple(x2.shape) == (3, h, w)
    # no budget of the caller's: the engine's cap, under which this image is one 152 x 240 frame
    big = canvas_for(h, w, (152, 240), 37)
    one = M.enhance_tiled(m, img_d, 4, tile="auto", noise=big)
    low = T.gather_tiles_array(img, (152, 240), (19, 30))
    assert low.shape == (1, 3, 152, 240) and np.array_equal(low[0], T.frame_load_array(img))
    frame = m.enhance_frame(torch.from_numpy(low).to(dev), 4, noise=big[:, None].to(dev)).cpu().numpy()
    assert np.array_equal(one.cpu().numpy(), T.blend_tiles_array(frame, (h, w), (19, 30)))
    with pytest.raises(ValueError):
        M.enhance_tiled(m, img_d, 4, tile="auto", noise=canvas)  # the canvas of another plan


# ------------------------------------------------------------------ 9. against the CPU oracle
@pytest.fixture(scope="module")
def oracle_loop(dev, small64):
    """80 x 136, tile (64, 96): four tiles, four steps -- the host loop with the CPU oracle as the denoiser (16 forwards)."""
    m, sd, spec = small64
    h, w, tile, v = 80, 136, (64, 96), (8, 12)
    img = dark_image(h, w, 44)
    canvas = canvas_for(h, w, tile, 55)

    def eps_fn(lat, low, t):
        with torch.no_grad():
            tt = torch.full((lat.shape[0],), t, dtype=torch.long)
            return oracle.unet_forward(sd, spec, torch.cat([torch.from_numpy(lat), torch.from_numpy(low)], 1), tt).numpy()

    _, ref_x = host_loop(m, dev, img, tile, v, canvas, eps_fn)
    assert len(origins_of(h, w, tile, v)) == 4
    return img, canvas, tile, v, ref_x


def test_loop_vs_oracle_fp32(dev, small64, oracle_loop):
    """Measured on an MI355X: max-abs of the fp32 canvas against the oracle's loop in the printed line."""
    m = small64[0]
    img, canvas, tile, v, ref_x = oracle_loop
    _, x = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, tile=tile, overlap=v, noise=canvas, sync="latents", return_canvas=True)
    err = np.abs(x.cpu().numpy() - ref_x).max()
    print(f"80 x 136, tile 64 x 96, fp32: canvas vs the oracle's loop, max-abs {err:.3e} (canvas up to {np.abs(ref_x).max():.1f})")
    assert err < 1e-3


def test_loop_vs_oracle_fp16(dev, small64, oracle_loop):
    m = small64[0]
    img, canvas, tile, v, ref_x = oracle_loop
    with compute_dtype(m, "fp16"):
        _, x = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, tile=tile, overlap=v, noise=canvas, sync="latents", return_canvas=True)
    p = psnr01(x.cpu(), ref_x)
    print(f"80 x 136, tile 64 x 96, fp16: PSNR of the clamped canvas against the oracle's loop {p:.1f} dB")
    assert p > 40.0


# ------------------------------------------------------------------ 10. the refusals
def test_refusals(dev, small64):
    m = small64[0]
    h, w, tile, v = PLAN
    img = torch.from_numpy(dark_image(h, w, 27)).to(dev)
    with pytest.raises(ValueError, match="element cap"):
        M.enhance_tiled(m, img, 4, tile=(2368, 2368))
    for bad in (canvas_for(h, w, tile, 1)[:, :, :100], canvas_for(h, w, tile, 1)[:3], canvas_for(h, w, tile, 1)[:, :, :, :200]):
        with pytest.raises(ValueError, match="canvas"):
            M.enhance_tiled(m, img, 4, tile=tile, noise=bad)
        with pytest.raises(ValueError, match="canvas"):
            M.enhance_tiled(m, img, 4, tile=tile, noise=bad, sync="latents")
    L = native.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    tiles = torch.zeros(9, 3, 64, 96, device=dev)
    x = torch.zeros(3, h, w, device=dev)
    out = torch.zeros(h, w, 3, dtype=torch.uint8, device=dev)
    p = (img.data_ptr(), tiles.data_ptr(), x.data_ptr(), out.data_ptr())
    last = native.StepCoef(0.8, 0.6, 0.9, 0.43, 1, 0, 0)
    assert L.llie_tile_gather_u8_hw(p[0], h, w, 64, 96, 8, 12, 0, 9, p[1], st) == 0
    assert L.llie_tile_gather_f32_hw(p[2], 3, h, w, 64, 96, 8, 12, 0, 9, p[1], st) == 0
    assert L.llie_tile_blend_u8_hw(p[1], h, w, 64, 96, 8, 12, p[3], st) == 0
    assert L.llie_tile_sync_step_hw(p[1], h, w, 64, 96, 8, 12, p[2], None, last, p[2], p[3], st) == 0
    for vy, vx in [(33, 12), (8, 49), (-1, 12), (8, -1)]:  # a bad overlap on either axis
        assert L.llie_tile_gather_u8_hw(p[0], h, w, 64, 96, vy, vx, 0, 1, p[1], st) == native.ERR_ARG
        assert L.llie_tile_gather_f32_hw(p[2], 3, h, w, 64, 96, vy, vx, 0, 1, p[1], st) == native.ERR_ARG
        assert L.llie_tile_blend_u8_hw(p[1], h, w, 64, 96, vy, vx, p[3], st) == native.ERR_ARG
        assert L.llie_tile_sync_step_hw(p[1], h, w, 64, 96, vy, vx, p[2], None, last, p[2], p[3], st) == native.ERR_ARG
    for first, count in [(0, 10), (9, 1), (-1, 1), (0, 0)]:  # a chunk outside the plan of 9 tiles
        assert L.llie_tile_gather_u8_hw(p[0], h, w, 64, 96, 8, 12, first, count, p[1], st) == native.ERR_ARG
        assert L.llie_tile_gather_f32_hw(p[2], 3, h, w, 64, 96, 8, 12, first, count, p[1], st) == native.ERR_ARG
    assert L.llie_tile_gather_f32_hw(p[2], 4, h, w, 64, 96, 8, 12, 0, 1, p[1], st) == native.ERR_ARG  # planes % 3
    step = native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 0)
    assert L.llie_tile_sync_step_hw(p[1], h, w, 64, 96, 8, 12, p[2], None, step, p[2], None, st) == native.ERR_ARG  # no noise, not last
    with pytest.raises(ValueError):
        M.gather_tiles_device(img, (64, 96), (8, 12), 8, 2)
    with pytest.raises(ValueError):
        M.blend_tiles_device(tiles[:8], (h, w), (8, 12))
    with pytest.raises(ValueError):
        M.sync_step_device(tiles, (h, w), (8, 12), x[:, :, :200].contiguous(), None, last)


# ------------------------------------------------------------------ 11. the CLI
@pytest.mark.parametrize("flag", ["64x96", "auto"])
def test_cli_tile_size(dev, small64, tmp_path, flag):
    from PIL import Image
    m, sd, _ = small64
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"epoch": 1, "model_state_dict": dict(sd)}, ckpt)
    h, w = 150, 233
    img = dark_image(h, w, 28)
    Image.fromarray(img).save(tmp_path / "dark.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "inference.py"), "--input", str(tmp_path / "dark.png"),
                        "--output", str(tmp_path / "out.png"), "--checkpoint", str(ckpt), "--variant", "small", "--image_size", "64",
                        "--num_steps", "4", "--noise_seed", "77", "--tile", "--tile_size", flag, "--tile_batch", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    out = np.asarray(Image.open(tmp_path / "out.png"))
    tile = (64, 96) if flag == "64x96" else "auto"
    shape = (64, 96) if flag == "64x96" else (152, 240)  # under the engine's cap "auto" is one frame
    want = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, tile=tile, tile_batch=4, noise=canvas_for(h, w, shape, 77))
    assert out.shape == (h, w, 3) and out.dtype == np.uint8
    assert np.array_equal(out, want.cpu().numpy())


# ------------------------------------------------------------------ 12. the evaluation keyword
def test_evaluate_full_resolution_tile(dev, small64):
    m = small64[0]
    sizes = [(150, 233), (64, 96), (70, 80)]
    low = [dark_image(h, w, 60 + i) for i, (h, w) in enumerate(sizes)]
    high = [np.random.default_rng(70 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(sizes)]
    store = M.DeviceFrameStore(low, high, device=dev)
    with pytest.raises(ValueError, match="mode"):
        M.evaluate_full_resolution(m, store, mode="frame", tile=(64, 96))
    for sync in ("none", "latents"):
        res = M.evaluate_full_resolution(m, store, num_inference_steps=4, seed=6, tile=(64, 96), tile_batch=4, sync=sync)
        g = torch.Generator(device=dev).manual_seed(6)
        for i, (h, w) in enumerate(sizes):
            canvas = torch.randn(4, 3, max(h, 64), max(w, 96), generator=g, device=dev)
            out = M.enhance_tiled(m, store.frame(i), 4, tile=(64, 96), tile_batch=4, noise=canvas, sync=sync)
            want = M.image_metrics(out, store.frame(len(sizes) + i))
            assert abs(res["per_image"]["psnr"][i] - float(want.psnr)) <= 1e-9
    auto = M.evaluate_full_resolution(m, store, num_inference_steps=4, seed=6, tile="auto", max_tile_pixels=8192)
    g = torch.Generator(device=dev).manual_seed(6)
    for i, (h, w) in enumerate(sizes):
        tile, overlap = M.auto_tile_plan((h, w), 8192)
        canvas = torch.randn(4, 3, max(h, tile[0]), max(w, tile[1]), generator=g, device=dev)
        out = M.enhance_tiled(m, store.frame(i), 4, tile="auto", max_tile_pixels=8192, noise=canvas)
        assert abs(auto["per_image"]["psnr"][i] - float(M.image_metrics(out, store.frame(len(sizes) + i)).psnr)) <= 1e-9
    assert auto["psnr"] != res["psnr"]
