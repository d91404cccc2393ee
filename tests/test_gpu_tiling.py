"""Tiled full-resolution enhancement on the MI355X: the three tile kernels against their NumPy twins (bit for bit, through
the C ABI), and `enhance_tiled` against the same path composed by hand from the host twins and `model.enhance`."""
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

SHAPES = [(300, 500, 64, 16), (64, 64, 64, 16), (65, 129, 64, 32), (50, 200, 64, 8), (481, 321, 128, 32), (97, 353, 64, 0),
          (1000, 777, 256, 32), (113, 64, 64, 31)]


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
    return m.to(dev).eval(), sd


def dark_image(h, w, seed):
    return (np.random.default_rng(seed).random((h, w, 3)) * 90).astype(np.uint8)


def canvas_for(h, w, s, seed, steps=4):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn(3, max(h, s), max(w, s), generator=g) for _ in range(steps)])


def noise_tiles_host(canvas, h, w, s, v):
    """[steps,3,Hc,Wc] -> [steps,T,3,S,S] by plain slicing."""
    oys, oxs = T.tile_origins(h, s, v), T.tile_origins(w, s, v)
    return np.stack([canvas[:, :, oy:oy + s, ox:ox + s] for oy in oys for ox in oxs], axis=1)


# ------------------------------------------------------------------ 5. kernels == host twins
@pytest.mark.parametrize("h,w,s,v", SHAPES)
def test_tile_kernels_bit_exact(dev, h, w, s, v):
    rng = np.random.default_rng(h * 7 + w)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img_d = torch.from_numpy(img).to(dev)
    ref = T.gather_tiles_array(img, s, v)
    total = ref.shape[0]
    got = M.gather_tiles_device(img_d, s, v)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), ref)
    # chunks that together are the whole, the last one short
    step = max(1, (total + 2) // 3)
    parts = [M.gather_tiles_device(img_d, s, v, first, min(step, total - first)) for first in range(0, total, step)]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), ref)

    canvas = rng.standard_normal((2, 3, max(h, s), max(w, s)), dtype=np.float32)
    canvas_d = torch.from_numpy(canvas).to(dev)
    nref = noise_tiles_host(canvas, h, w, s, v)
    assert np.array_equal(M.gather_noise_device(canvas_d, (h, w), s, v).cpu().numpy(), nref)
    nparts = [M.gather_noise_device(canvas_d, (h, w), s, v, first, min(step, total - first)) for first in range(0, total, step)]
    assert np.array_equal(torch.cat(nparts, dim=1).cpu().numpy(), nref)

    tiles = rng.random((total, 3, s, s), dtype=np.float32) * np.float32(2.4) - np.float32(1.2)  # the clip acts
    want = T.blend_tiles_array(tiles, (h, w), v)
    out = M.blend_tiles_device(torch.from_numpy(tiles).to(dev), (h, w), v)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3)
    assert np.array_equal(out.cpu().numpy(), want)
    # and the round trip of the image itself
    assert np.array_equal(M.blend_tiles_device(got, (h, w), v).cpu().numpy(), T.blend_tiles_array(ref, (h, w), v))


def test_tile_kernels_refuse_bad_arguments(dev):
    img = torch.zeros(100, 120, 3, dtype=torch.uint8, device=dev)
    out = torch.empty(4, 3, 64, 64, device=dev)
    L = native.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    for v, first, count in [(-1, 0, 1), (33, 0, 1), (8, 0, 5), (8, 4, 1), (8, -1, 1), (8, 0, 0)]:
        assert L.llie_tile_gather_u8(img.data_ptr(), 100, 120, 64, v, first, count, out.data_ptr(), st) == native.ERR_ARG
        assert L.llie_tile_gather_f32(out.data_ptr(), 3, 100, 120, 64, v, first, count, out.data_ptr(), st) == native.ERR_ARG
    assert L.llie_tile_gather_f32(out.data_ptr(), 4, 100, 120, 64, 8, 0, 1, out.data_ptr(), st) == native.ERR_ARG  # planes % 3
    assert L.llie_tile_blend_u8(out.data_ptr(), 100, 120, 64, 40, img.data_ptr(), st) == native.ERR_ARG
    assert L.llie_tile_blend_u8(out.data_ptr(), 0, 120, 64, 8, img.data_ptr(), st) == native.ERR_ARG
    with pytest.raises(ValueError):
        M.gather_tiles_device(img, 64, 8, 3, 2)
    with pytest.raises(ValueError):
        M.gather_tiles_device(img.float(), 64, 8)
    with pytest.raises(ValueError):
        M.blend_tiles_device(out[:3], (100, 120), 8)
    with pytest.raises(ValueError):
        M.enhance_tiled(M.LowLightDiffusion(unet_variant="small", image_size=64).to(dev), img, noise=torch.zeros(4, 3, 64, 64))


# ------------------------------------------------------------------ 6. the composition
@pytest.mark.parametrize("cd", ["fp32", "fp16"])
def test_enhance_tiled_equals_hand_composition(dev, small64, cd):
    m, _ = small64
    h, w, s, v, tb = 150, 200, 64, 16, 5
    img = dark_image(h, w, 21)
    canvas = canvas_for(h, w, s, 31)
    m.compute_dtype = cd
    try:
        got = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, overlap=v, tile_batch=tb, noise=canvas)
        low = T.gather_tiles_array(img, s, v)
        draws = noise_tiles_host(canvas.numpy(), h, w, s, v)
        total = low.shape[0]
        assert total == 12  # 3 x 4 tiles: chunks of 5, 5 and 2
        outs = []
        for first in range(0, total, tb):
            sl = slice(first, min(first + tb, total))
            outs.append(m.enhance(torch.from_numpy(low[sl]).to(dev), 4, noise=torch.from_numpy(draws[:, sl]).to(dev)).cpu().numpy())
        want = T.blend_tiles_array(np.concatenate(outs), (h, w), v)
    finally:
        m.compute_dtype = None
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(want.astype(np.int64).std()) > 0  # not a constant image


# ------------------------------------------------------------------ 7. tile_batch does not change the bytes
def test_tile_batch_invariance(dev, small64):
    m, _ = small64
    img = torch.from_numpy(dark_image(150, 200, 22)).to(dev)
    canvas = canvas_for(150, 200, 64, 32)
    a = M.enhance_tiled(m, img, 4, overlap=16, tile_batch=3, noise=canvas)
    b = M.enhance_tiled(m, img, 4, overlap=16, tile_batch=32, noise=canvas)
    assert torch.equal(a, b)


# ------------------------------------------------------------------ 8. one tile is the existing path
def test_single_tile_is_the_untiled_path(dev, small64):
    m, _ = small64
    img = torch.from_numpy(dark_image(64, 64, 23)).to(dev)
    canvas = canvas_for(64, 64, 64, 33)
    got = M.enhance_tiled(m, img, 4, noise=canvas)
    want = M.postprocess_device(m.enhance(M.preprocess_device(img, 64), 4, noise=canvas[:, None].to(dev)), (64, 64))[0]
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 9. seeds
def test_generator_seeds(dev, small64):
    m, _ = small64
    img = torch.from_numpy(dark_image(100, 130, 24)).to(dev)

    def run(seed):
        torch.manual_seed(seed + 1000)
        return M.enhance_tiled(m, img, 4, overlap=8, generator=torch.Generator(device=dev).manual_seed(seed))

    a, b, c = run(5), run(5), run(6)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)


# ------------------------------------------------------------------ 10. repeated calls replay captured graphs
def test_repeated_calls_add_no_graphs(dev):
    spec = oracle.make_spec("small", 64)
    m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4)
    m.load_state_dict(oracle.synth_state_dict(oracle.param_shapes(spec)))
    m = m.to(dev).eval()
    img = torch.from_numpy(dark_image(150, 200, 25)).to(dev)
    canvas = canvas_for(150, 200, 64, 35).to(dev)
    first = M.enhance_tiled(m, img, 4, overlap=16, tile_batch=5, noise=canvas)  # chunks of 5, 5, 2
    h = m.unet._prepare(1, dev)[0]
    L = native.lib()
    entries = L.llie_graph_cache_entries(h.h)
    assert entries == 2  # one per batch size
    for _ in range(2):
        assert torch.equal(M.enhance_tiled(m, img, 4, overlap=16, tile_batch=5, noise=canvas), first)
        assert L.llie_graph_cache_entries(h.h) == entries


# ------------------------------------------------------------------ 11. the CLI
def test_cli_tile(dev, small64, tmp_path):
    from PIL import Image
    m, sd = small64
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"epoch": 1, "model_state_dict": dict(sd)}, ckpt)
    img = dark_image(150, 200, 26)
    Image.fromarray(img).save(tmp_path / "dark.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "inference.py"), "--input", str(tmp_path / "dark.png"),
                        "--output", str(tmp_path / "out.png"), "--checkpoint", str(ckpt), "--variant", "small", "--image_size", "64",
                        "--num_steps", "4", "--noise_seed", "77", "--tile", "--tile_overlap", "16", "--tile_batch", "8"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    out = np.asarray(Image.open(tmp_path / "out.png"))
    want = M.enhance_tiled(m, torch.from_numpy(img).to(dev), 4, overlap=16, tile_batch=8, noise=canvas_for(150, 200, 64, 77))
    assert out.shape == (150, 200, 3) and out.dtype == np.uint8
    assert np.array_equal(out, want.cpu().numpy())
