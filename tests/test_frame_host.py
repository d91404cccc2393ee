"""Frame mode without a GPU: the frame rule of the engine (llie_frame_shape_ok, host only), the NumPy twins of the load / store
kernels against an independent restatement, and the reference's own EfficientUNet.forward at rectangular sizes
(tests/golden/unet_rect_kat.npz, tools/make_golden_rect.py) against the CPU oracle -- the yardstick of tests/test_gpu_frame.py."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import max_abs, synth_input

M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")
T = importlib.import_module("cv-diffusion-model_amd.tiling")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. the frame rule
@pytest.fixture(scope="module")
def h64():
    """A small@64 context: without a device it still describes the plans (no weights, cannot run)."""
    unet = M.create_efficient_unet("small", image_size=64, in_channels=6)
    return N.Handle(unet._make_cfg(N.LLIE_F16))


def test_frame_shape_ok_accepts_and_refuses(h64):
    L = N.lib()
    for hh, ww in [(64, 64), (64, 96), (72, 104), (400, 600)]:
        assert L.llie_frame_shape_ok(h64.h, 1, hh, ww) == 0, (hh, ww)
        assert L.llie_frame_shape_ok(h64.h, 2, hh, ww) == 0, (hh, ww)
    for hh, ww in [(56, 64), (64, 60), (60, 64)]:
        assert L.llie_frame_shape_ok(h64.h, 1, hh, ww) == N.ERR_SHAPE, (hh, ww)
        assert "multiples of 8 and at least 64" in N.last_error()
        with pytest.raises(ValueError, match="multiples of 8"):
            h64.frame_shape_ok(1, hh, ww)
        with pytest.raises(ValueError, match="multiples of 8"):
            h64.frame_workspace_bytes(1, hh, ww)
    # the batch clause is checked before the element cap (which 65536 frames of any size break as well) and is the one named
    assert L.llie_frame_shape_ok(h64.h, 65536, 64, 64) == N.ERR_SHAPE
    assert "65535" in N.last_error()
    assert L.llie_frame_shape_ok(h64.h, 1365, 64, 64) == 0 and 1365 * 4096 * 384 <= 2 ** 31 - 1 < 1366 * 4096 * 384
    assert L.llie_frame_shape_ok(h64.h, 1366, 64, 64) == N.ERR_SHAPE
    assert "element cap" in N.last_error()
    assert L.llie_frame_shape_ok(h64.h, 0, 64, 64) == N.ERR_ARG


def test_frame_shape_ok_element_cap(h64):
    """small: the widest tensor at full resolution is the 384-channel hidden map of decoder_blocks.3.0 ((64 + 32) * 4), so the cap
    is B * H * W * 384 <= 2^31 - 1."""
    L = N.lib()
    cap = 2 ** 31 - 1
    under, past = (64, 87376), (64, 87384)
    assert under[0] * under[1] * 384 <= cap < past[0] * past[1] * 384
    assert L.llie_frame_shape_ok(h64.h, 1, *under) == 0
    assert L.llie_frame_shape_ok(h64.h, 1, *past) == N.ERR_SHAPE
    assert "element cap" in N.last_error() and "tiles" in N.last_error()
    assert L.llie_frame_shape_ok(h64.h, 1, under[1], under[0]) == 0
    assert L.llie_frame_shape_ok(h64.h, 1, past[1], past[0]) == N.ERR_SHAPE
    # the batch counts: two frames of just over half the cap
    assert L.llie_frame_shape_ok(h64.h, 2, 64, 43688) == 0 and 2 * 64 * 43688 * 384 <= cap
    assert L.llie_frame_shape_ok(h64.h, 2, 64, 43696) == N.ERR_SHAPE and 2 * 64 * 43696 * 384 > cap
    # 1080p fits at B = 1 and B = 2, not at B = 3
    assert L.llie_frame_shape_ok(h64.h, 2, 1080, 1920) == 0
    assert L.llie_frame_shape_ok(h64.h, 3, 1080, 1920) == N.ERR_SHAPE


def test_frame_workspace_is_the_square_one_at_image_size(h64):
    """One implementation: the entry points without _hw are the frame ones at H = W = image_size."""
    for b in (1, 3):
        assert h64.frame_workspace_bytes(b, 64, 64) == h64.workspace_bytes(b)
        assert h64.frame_workspace_bytes(b, 64, 64, 8) == h64.enhance_workspace_bytes(b, 8)
    # a function of the size, symmetric in nothing it should not be: more pixels, more scratch
    assert h64.frame_workspace_bytes(1, 64, 96) > h64.frame_workspace_bytes(1, 64, 64)
    assert h64.frame_workspace_bytes(1, 72, 104, 4) > h64.frame_workspace_bytes(1, 72, 104)


def test_exports():
    for name in ("frame_pad", "frame_load_array", "frame_store_array", "frame_load_device", "frame_store_device", "enhance_frame_u8"):
        assert name in M.__all__ and hasattr(M, name)
    assert hasattr(M.LowLightDiffusion, "enhance_frame")
    import cv_diffusion_model_amd as shim
    assert shim.enhance_frame_u8 is M.enhance_frame_u8
    for sym in ("llie_frame_shape_ok", "llie_frame_workspace_bytes", "llie_unet_forward_hw", "llie_enhance_hw", "llie_frame_pad",
                "llie_frame_load_u8", "llie_frame_store_u8"):
        assert sym in N.EXPORTS and hasattr(N.lib(), sym)


# ------------------------------------------------------------------ 2. the twins
SIZES = [(1, 1), (11, 13), (63, 65), (64, 64), (400, 601)]


def pad_of(length):
    p = 64
    while p < length:
        p += 8
    return p


def test_frame_pad():
    for length in (1, 11, 63, 64, 65, 72, 400, 601, 1080):
        assert T.frame_pad(length) == pad_of(length) == N.lib().llie_frame_pad(length)
    assert N.lib().llie_frame_pad(0) == N.ERR_ARG
    with pytest.raises(ValueError):
        T.frame_pad(0)


@pytest.mark.parametrize("h,w", SIZES)
def test_load_twin_against_restatement(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    got = T.frame_load_array(img)
    hp, wp = pad_of(h), pad_of(w)
    assert got.dtype == np.float32 and got.shape == (3, hp, wp)
    # independent restatement: a table of the 256 values, indexed pixel by pixel through clamped coordinates
    table = np.array([np.float32(np.float32(v) / np.float32(127.5)) - np.float32(1.0) for v in range(256)], dtype=np.float32)
    ys = np.array([min(y, h - 1) for y in range(hp)])
    xs = np.array([min(x, w - 1) for x in range(wp)])
    for c in range(3):
        assert np.array_equal(got[c], table[img[ys][:, xs, c]])
    # the padded region is the replicated edge
    assert np.array_equal(got[:, h:, :w], np.broadcast_to(got[:, h - 1:h, :w], (3, hp - h, w)))
    assert np.array_equal(got[:, :, w:], np.broadcast_to(got[:, :, w - 1:w], (3, hp, wp - w)))
    assert got.min() >= -1.0 and got.max() <= 1.0


@pytest.mark.parametrize("h,w", SIZES)
def test_store_twin_against_restatement(h, w):
    rng = np.random.default_rng(h * 77 + w)
    hp, wp = pad_of(h), pad_of(w)
    x = rng.uniform(-1.3, 1.3, size=(3, hp, wp)).astype(np.float32)
    x[:, 0, 0] = [-1.0, 1.0, 0.0]
    got = T.frame_store_array(x, (h, w))
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    want = np.empty((h, w, 3), np.uint8)
    for c in range(3):
        v = (x[c, :h, :w] + np.float32(1.0)) * np.float32(127.5)
        want[:, :, c] = np.floor(np.minimum(np.maximum(v, np.float32(0)), np.float32(255))).astype(np.uint8)
    assert np.array_equal(got, want)
    assert tuple(got[0, 0]) == (0, 255, 127)
    with pytest.raises(ValueError):
        T.frame_store_array(x[:, :-8], (h, w))
    with pytest.raises(ValueError):
        T.frame_store_array(x, (0, w))


@pytest.mark.parametrize("h,w", SIZES)
def test_store_inverts_load_on_the_byte_grid(h, w):
    """store(load(img)) is within one LSB of img and never above it: byte / 127.5 - 1 comes back as (.. + 1) * 127.5, which lands
    on the byte or a rounding below it, and the truncation then loses a step (the untiled pair and the tiles behave alike)."""
    rng = np.random.default_rng(h + w)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    back = T.frame_store_array(T.frame_load_array(img), (h, w)).astype(np.int64)
    assert back.shape == img.shape
    assert np.all(back <= img) and np.all(img - back <= 1)
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    exact = T.frame_store_array(T.frame_load_array(ramp), (1, 256))[0, :, 0] == np.arange(256)
    assert exact.mean() > 0.5 and exact[0] and exact[255]


def test_twins_refuse_bad_images():
    with pytest.raises(ValueError):
        T.frame_load_array(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        T.frame_load_array(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        T.frame_load_array(np.zeros((0, 4, 3), np.uint8))


# ------------------------------------------------------------------ 3. refusals that need no device, and the CLIs
def test_refusals_without_a_device():
    model = M.LowLightDiffusion(unet_variant="small", image_size=64)
    img = torch.zeros(70, 90, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.enhance_frame_u8(model, img)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.frame_load_device(img)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.frame_store_device(torch.zeros(3, 72, 96), (70, 90))
    with pytest.raises(RuntimeError, match="HIP device"):
        model.enhance_frame(torch.zeros(1, 3, 64, 96))
    with pytest.raises(ValueError):
        M.enhance_frame_u8(model, img.float())
    with pytest.raises(ValueError):
        M.enhance_frame_u8(model, img.numpy())
    store = M.DeviceFrameStore([np.zeros((16, 16, 3), np.uint8)], [np.zeros((16, 16, 3), np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="mode"):
        M.evaluate_full_resolution(None, store, mode="whole")
    with pytest.raises(ValueError, match="tiled"):
        M.evaluate_full_resolution(None, store, mode="frame", overlap=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.evaluate_full_resolution(None, store, mode="frame")


def _script(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def test_cli_flags():
    inference = _script("inference")
    a = inference.parse_args(["--input", "a.png", "--output", "b.png", "--native"])
    assert a.native is True and a.tile is False
    assert inference.parse_args(["--input", "a.png", "--output", "b.png"]).native is False
    for extra in (["--tile"], ["--tile_overlap", "16"], ["--tile_batch", "8"]):
        with pytest.raises(SystemExit):
            inference.parse_args(["--input", "a.png", "--output", "b.png", "--native"] + extra)
    ev = _script("evaluate")
    assert ev.parse_args(["--data", "x"]).full_resolution is None
    assert ev.parse_args(["--data", "x", "--full_resolution"]).full_resolution == "tiled"
    assert ev.parse_args(["--data", "x", "--full_resolution", "--per_image"]).full_resolution == "tiled"
    assert ev.parse_args(["--data", "x", "--full_resolution", "frame"]).full_resolution == "frame"
    for extra in (["--tile_overlap", "16"], ["--tile_batch", "8"]):
        with pytest.raises(SystemExit):
            ev.parse_args(["--data", "x", "--full_resolution", "frame"] + extra)
    assert ev.parse_args(["--data", "x", "--full_resolution", "--tile_overlap", "16"]).tile_overlap == 16


# ------------------------------------------------------------------ 4. the reference at rectangular sizes against the oracle
@pytest.mark.parametrize("h,w,full", [(64, 96, True), (72, 104, True), (96, 64, False), (104, 72, False)])
def test_oracle_reproduces_the_reference_at_rectangular_sizes(golden, h, w, full):
    """The bar is the one tests/test_oracle_golden.py::test_unet_forward uses for unet_kat: 5e-5 x max(1, max |y|).  Measured when the
    golden was made: at most 4.2e-6 max-abs on outputs of magnitude 3.1 to 3.9."""
    g = golden("unet_rect_kat.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "unet_rect_kat.npz")) < 200 * 1024
    spec = oracle.make_spec("small", 64)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    x = synth_input(f"rect{h}x{w}.x", (1, 6, h, w), -1.5, 1.5)
    with torch.no_grad():
        y = oracle.unet_forward(sd, spec, x, torch.from_numpy(g["t"]))
    assert int(g["t"][0]) == 499 and tuple(y.shape) == (1, 3, h, w)
    want = g[f"rect{h}x{w}"]
    got = y if full else y[:, :, ::2, ::2]
    assert tuple(got.shape) == want.shape
    err = max_abs(got, want)
    print(f"{h}x{w}: max-abs {err:.2e} on outputs of magnitude {np.abs(want).max():.2f}")
    assert err < 5e-5 * max(1.0, np.abs(want).max())
