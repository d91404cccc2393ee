"""Device PSNR / SSIM and `evaluate` on the MI355X against the NumPy twin (metrics.image_metrics_host, the definition).

Tolerance against the twin: 1e-9 absolute on ssim, 1e-9 relative on mse, 1e-8 dB on finite psnr.  Both sides are float64 and
differ only in summation order; separable against direct 2-D summation differs by at most 2.5e-13 per map entry over noise,
near-identical, constant and quantised inputs, so 1e-9 leaves three orders of magnitude and still sits five orders below what an
fp32 kernel gives on the constant case (2e-4)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
MX = importlib.import_module("cv-diffusion-model_amd.metrics")

F32_SHAPES = [(1, 11, 11), (2, 12, 27), (3, 24, 40), (1, 64, 64), (2, 37, 130), (1, 100, 75)]
U8_SHAPES = [(1, 11, 11), (1, 50, 200), (2, 65, 129)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def synth_model(dev, salt=None):
    spec = oracle.make_spec("small", 64)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    if salt is not None:  # a second set of weights: the first, perturbed
        g = torch.Generator().manual_seed(salt)
        sd = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g) for k, v in sd.items()}
    m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4)
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd


@pytest.fixture(scope="module")
def small64(dev):
    return synth_model(dev)


def dark_image(h, w, seed):
    return (np.random.default_rng(seed).random((h, w, 3)) * 90).astype(np.uint8)


@pytest.fixture(scope="module")
def store(dev):
    sizes = [(80, 100)] * 4 + [(64, 64)]
    low = [dark_image(h, w, 100 + i) for i, (h, w) in enumerate(sizes)]
    high = [np.random.default_rng(200 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(sizes)]
    return M.DeviceFrameStore(low, high, device=dev, names=[f"im{i}.png" for i in range(5)])


def triples(m):
    """ImageMetrics of device tensors or arrays -> float64 [B,3] on the host."""
    return np.stack([v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in m], axis=1)


def assert_close(got, want, what=""):
    """got / want: [B,3] = (mse, psnr, ssim)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print(what, "mse rel", np.abs(got[:, 0] - want[:, 0]) / np.maximum(want[:, 0], 1e-300), "ssim abs", np.abs(got[:, 2] - want[:, 2]))
    assert got.shape == want.shape
    assert (np.abs(got[:, 0] - want[:, 0]) <= 1e-9 * want[:, 0]).all(), (what, got[:, 0], want[:, 0])
    fin = np.isfinite(want[:, 1])
    assert np.array_equal(np.isposinf(got[:, 1]), np.isposinf(want[:, 1])) and np.array_equal(np.isfinite(got[:, 1]), fin)
    assert (np.abs(got[fin, 1] - want[fin, 1]) <= 1e-8).all(), (what, got[:, 1], want[:, 1])
    assert (np.abs(got[:, 2] - want[:, 2]) <= 1e-9).all(), (what, got[:, 2], want[:, 2])


def f32_contents(b, h, w, seed):
    rng = np.random.default_rng(seed)
    u = lambda: (rng.random((b, 3, h, w)) * 2 - 1).astype(np.float32)  # noqa: E731
    a = u()
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.broadcast_to(((yy / max(h - 1, 1) + xx / max(w - 1, 1)) - 1.0).astype(np.float32), (b, 3, h, w)).copy()
    return {
        "noise": (a, u()),
        "near": (a, np.clip(a + np.float32(0.02) * rng.standard_normal(a.shape).astype(np.float32), -1, 1).astype(np.float32)),
        "constant": (np.full((b, 3, h, w), 0.8, np.float32), np.full((b, 3, h, w), 0.76, np.float32)),
        "identical": (a, a.copy()),
        "ramp": (ramp, (np.float32(0.9) * ramp + np.float32(0.03)).astype(np.float32)),
    }


# ------------------------------------------------------------------ 1. fp32 NCHW
@pytest.mark.parametrize("b,h,w", F32_SHAPES)
def test_kernel_vs_twin_f32(dev, b, h, w):
    for name, (x, y) in f32_contents(b, h, w, h * 131 + w).items():
        got = M.image_metrics(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
        assert all(v.dtype == torch.float64 and v.device.type == "cuda" and tuple(v.shape) == (b,) for v in got)
        g = triples(got)
        assert_close(g, triples(M.image_metrics_host(x, y)), f"{name} {b}x{h}x{w}")
        if name == "identical":
            assert (g[:, 0] == 0).all() and np.isposinf(g[:, 1]).all() and np.abs(g[:, 2] - 1).max() <= 1e-12
        if name == "constant":  # 0.9 vs 0.88 on [0, 1], up to the fp32 rounding of 0.8 and 0.76
            assert np.abs(g[:, 2] - (2 * 0.9 * 0.88 + 1e-4) / (0.81 + 0.7744 + 1e-4)).max() <= 1e-7


def test_data_range_f32(dev):
    rng = np.random.default_rng(5)
    x, y = rng.random((2, 3, 30, 41)).astype(np.float32), rng.random((2, 3, 30, 41)).astype(np.float32)
    got = M.image_metrics(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), data_range=(0.0, 1.0))
    assert_close(triples(got), triples(M.image_metrics_host(x, y, data_range=(0.0, 1.0))), "range 0..1")
    with pytest.raises(ValueError):
        M.image_metrics(torch.zeros(1, 3, 10, 30, device=dev), torch.zeros(1, 3, 10, 30, device=dev))
    with pytest.raises(ValueError):
        M.image_metrics(torch.zeros(1, 3, 12, 30, device=dev), torch.zeros(1, 3, 12, 30, device=dev), data_range=(1.0, 1.0))


# ------------------------------------------------------------------ 2. uint8 HWC
@pytest.mark.parametrize("b,h,w", U8_SHAPES)
def test_kernel_vs_twin_u8(dev, b, h, w):
    rng = np.random.default_rng(h * 17 + w)
    rnd = lambda: rng.integers(0, 256, size=(b, h, w, 3), dtype=np.uint8)  # noqa: E731
    a = rnd()
    cases = {"random": (a, rnd()), "dark": ((rng.random((b, h, w, 3)) * 90).astype(np.uint8), (rng.random((b, h, w, 3)) * 90).astype(np.uint8)),
             "extremes": (np.zeros((b, h, w, 3), np.uint8), np.full((b, h, w, 3), 255, np.uint8)), "identical": (a, a.copy())}
    for name, (x, y) in cases.items():
        g = triples(M.image_metrics(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)))
        assert_close(g, triples(M.image_metrics_host(x, y)), f"u8 {name} {b}x{h}x{w}")
        if name == "extremes":
            assert (g[:, 0] == 1).all() and (g[:, 1] == 0).all()
        if name == "identical":
            assert (g[:, 0] == 0).all() and np.isposinf(g[:, 1]).all() and np.abs(g[:, 2] - 1).max() <= 1e-12
    # a single image without the batch axis
    one = M.image_metrics(torch.from_numpy(a[0]).to(dev), torch.from_numpy(cases["random"][1][0]).to(dev))
    assert_close(triples(one), triples(M.image_metrics_host(a[0], cases["random"][1][0])), "u8 single")


# ------------------------------------------------------------------ 3. one changed value: halo and double counting
def test_single_pixel_sweep(dev):
    h, w = 48, 80
    th, tw = MX.TILE_H, MX.TILE_W  # the kernel's tiles of valid positions: boundaries at multiples of them
    assert (th, tw) == (16, 32)
    rng = np.random.default_rng(9)
    a = (rng.random((1, 3, h, w)) * 2 - 1).astype(np.float32)
    ys = [th - 1, th, 2 * th - 1, 2 * th, th + 9, th + 10]  # either side of a tile's first row, and of the end of its halo
    xs = [tw - 1, tw, 2 * tw - 1, 2 * tw, tw + 9, tw + 10]
    pos = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1), (5, 5), (10, 10),
           (11, 11)]
    pos += [(y, tw + 3) for y in ys] + [(th + 3, x) for x in xs] + [(th - 1, tw - 1), (th, tw), (2 * th - 1, 2 * tw - 1),
                                                                    (2 * th, 2 * tw), (th + 10, tw + 10), (h - 11, w - 11)]
    pos = list(dict.fromkeys(pos))
    assert len(pos) <= 32
    a_d = torch.from_numpy(a).to(dev)
    for i, (y, x) in enumerate(pos):
        c = i % 3
        b = a.copy()
        b[0, c, y, x] = -a[0, c, y, x] if abs(a[0, c, y, x]) > 0.1 else np.float32(0.7)
        g = triples(M.image_metrics(a_d, torch.from_numpy(b).to(dev)))
        assert_close(g, triples(M.image_metrics_host(a, b)), f"pixel ({c},{y},{x})")
        d = (float(a[0, c, y, x]) - float(b[0, c, y, x])) / 2.0
        assert abs(g[0, 0] - d * d / (3 * h * w)) <= 1e-9 * d * d / (3 * h * w)


# ------------------------------------------------------------------ 4. determinism and batch invariance
def test_determinism_and_batch_invariance(dev):
    rng = np.random.default_rng(11)
    xf = torch.from_numpy((rng.random((3, 3, 53, 91)) * 2 - 1).astype(np.float32)).to(dev)
    yf = torch.from_numpy((rng.random((3, 3, 53, 91)) * 2 - 1).astype(np.float32)).to(dev)
    xu = torch.from_numpy(rng.integers(0, 256, size=(3, 53, 91, 3), dtype=np.uint8)).to(dev)
    yu = torch.from_numpy(rng.integers(0, 256, size=(3, 53, 91, 3), dtype=np.uint8)).to(dev)
    for x, y in ((xf, yf), (xu, yu)):
        first = torch.stack(M.image_metrics(x, y))
        again = torch.stack(M.image_metrics(x, y))
        alone = torch.stack(M.image_metrics(x[1:2].clone(), y[1:2].clone()))
        assert torch.equal(first.view(torch.int64), again.view(torch.int64))
        assert torch.equal(first[:, 1:2].view(torch.int64), alone.view(torch.int64))


# ------------------------------------------------------------------ 5. a large ragged image
def test_large_ragged_u8(dev):
    rng = np.random.default_rng(13)
    a = rng.integers(0, 256, size=(1000, 777, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int32) + rng.integers(-20, 21, size=a.shape), 0, 255).astype(np.uint8)
    g = triples(M.image_metrics(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)))
    assert_close(g, triples(M.image_metrics_host(a, b)), "1000x777")


# ------------------------------------------------------------------ 6. evaluate
def hand_evaluate(m, loader, dev, seed, steps=4, loss=True):
    """The documented draw recipe by hand; the outputs are scored by the twin on the host."""
    g = torch.Generator(device=dev).manual_seed(seed)
    s, t_max = m.image_size, m.scheduler.config.num_train_timesteps
    rows, losses, names = [], [], []
    for batch in loader:
        low, normal = batch["low_light"], batch["normal_light"]
        b = low.shape[0]
        noise = torch.randn(steps, b, 3, s, s, generator=g, device=dev)
        if loss:
            t = torch.randint(0, t_max, (b,), generator=g, device=dev)
            eps = torch.randn(b, 3, s, s, generator=g, device=dev)
        out = m.enhance(low, steps, noise=noise)
        rows.append(triples(M.image_metrics_host(out.cpu().numpy(), normal.cpu().numpy())))
        if loss:
            with torch.no_grad():
                losses.append(F.mse_loss(m.forward(low, normal, timesteps=t, noise=eps)["noise_pred"], eps).item())
        names += list(batch["filename"])
    return np.concatenate(rows), (sum(losses) / len(loader) if loss else None), names


def per_image(res):
    p = res["per_image"]
    return np.stack([p["mse"], p["psnr"], p["ssim"]], axis=1)


def test_evaluate(dev, small64, store):
    m, _ = small64
    loader = M.DevicePairLoader(store, 2, 64, "val")
    assert len(loader) == 3
    torch.manual_seed(123)
    state = torch.cuda.get_rng_state(dev)
    res = M.evaluate(m, loader, num_inference_steps=4, seed=3)
    assert torch.equal(torch.cuda.get_rng_state(dev), state)
    want, want_loss, names = hand_evaluate(m, loader, dev, 3)
    assert res["n"] == 5 and res["per_image"]["filename"] == names == store.names
    assert_close(per_image(res), want, "evaluate")
    for j, key in enumerate(("mse", "psnr", "ssim")):
        assert abs(res[key] - sum(float(v) for v in per_image(res)[:, j]) / 5) <= 1e-12 * abs(res[key])
    assert abs(res["loss"] - want_loss) <= 1e-6 * abs(want_loss)
    torch.manual_seed(999)  # the global generator plays no part
    assert M.evaluate(m, loader, num_inference_steps=4, seed=3) == res
    other = M.evaluate(m, loader, num_inference_steps=4, seed=4, loss=False)
    assert "loss" not in other and other["psnr"] != res["psnr"]
    nl_want, _, _ = hand_evaluate(m, loader, dev, 4, loss=False)
    assert_close(per_image(other), nl_want, "evaluate without loss")


# ------------------------------------------------------------------ 7. evaluate_full_resolution
def test_evaluate_full_resolution(dev, small64, store):
    m, _ = small64
    res = M.evaluate_full_resolution(m, store, num_inference_steps=4, seed=6, overlap=16, tile_batch=4)
    assert res["n"] == 5 and "loss" not in res and res["per_image"]["filename"] == store.names
    g = torch.Generator(device=dev).manual_seed(6)
    rows, outs = [], []
    for i, (h, w) in enumerate(store.sizes):
        canvas = torch.randn(4, 3, max(h, 64), max(w, 64), generator=g, device=dev)
        out = M.enhance_tiled(m, store.frame(i), 4, overlap=16, tile_batch=4, noise=canvas)
        outs.append((out, canvas))
        assert torch.equal(store.frame(5 + i).cpu(), torch.from_numpy(store.host_frames()[5 + i]))
        rows.append(triples(M.image_metrics_host(out.cpu().numpy(), store.frame(5 + i).cpu().numpy())))
    assert_close(per_image(res), np.concatenate(rows), "full resolution")
    # the 64 x 64 pair is one tile: the untiled path
    out, canvas = outs[4]
    plain = M.postprocess_device(m.enhance(M.preprocess_device(store.frame(4), 64), 4, noise=canvas[:, None]), (64, 64))[0]
    assert torch.equal(out, plain)
    assert_close(per_image(res)[4:5], triples(M.image_metrics_host(plain.cpu().numpy(), store.frame(9).cpu().numpy())), "one tile")


# ------------------------------------------------------------------ 8. weights=
def test_evaluate_with_swapped_weights(dev, small64, store):
    m, _ = small64
    m2, _ = synth_model(dev, salt=77)
    loader = M.DevicePairLoader(store, 2, 64, "val")
    before = [p.detach().clone() for p in m.parameters()]
    w2 = [p.detach().clone() for p in m2.parameters()]
    got = M.evaluate(m, loader, num_inference_steps=4, seed=1, weights=w2)
    want = M.evaluate(m2, loader, num_inference_steps=4, seed=1)
    assert got == want
    assert got["psnr"] != M.evaluate(m, loader, num_inference_steps=4, seed=1)["psnr"]
    assert all(torch.equal(p.detach().view(torch.int32), q.view(torch.int32)) for p, q in zip(m.parameters(), before))
    # restored when the evaluation raises, too
    big = M.DeviceFrameStore([dark_image(130, 130, 1)], [dark_image(130, 130, 2)], device=dev)
    with pytest.raises(ValueError):
        M.evaluate(m, M.DevicePairLoader(big, 1, 128, "val"), weights=w2)
    assert all(torch.equal(p.detach().view(torch.int32), q.view(torch.int32)) for p, q in zip(m.parameters(), before))
    with pytest.raises(ValueError):
        M.evaluate(m, loader, weights=w2[:-1])


# ------------------------------------------------------------------ 9. the CLI
def test_cli(dev, small64, tmp_path):
    from PIL import Image
    m, sd = small64
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"epoch": 1, "model_state_dict": dict(sd)}, ckpt)
    sizes = [(70, 90), (64, 64), (80, 66)]
    for d in ("low", "high"):
        os.makedirs(tmp_path / "data" / d)
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(dark_image(h, w, 40 + i)).save(tmp_path / "data" / "low" / f"{i}.png")
        Image.fromarray(np.random.default_rng(50 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / "data" / "high" / f"{i}.png")
    base = [sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--data", str(tmp_path / "data"), "--checkpoint", str(ckpt),
            "--image_size", "64", "--batch_size", "2", "--per_image"]
    st = M.DeviceFrameStore.from_folder(str(tmp_path / "data"), device=dev)
    wants = {(): M.evaluate(m, M.DevicePairLoader(st, 2, 64, "val"), num_inference_steps=4, seed=0),
             ("--full_resolution",): M.evaluate_full_resolution(m, st, num_inference_steps=4, seed=0)}
    for extra, want in wants.items():
        out_file = tmp_path / f"res{len(extra)}.json"
        r = subprocess.run(base + list(extra) + ["--output", str(out_file)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        got = json.loads(r.stdout.strip().splitlines()[-1])
        assert json.loads(out_file.read_text()) == got
        assert got["n"] == 3 and got["per_image"]["filename"] == want["per_image"]["filename"] == ["0.png", "1.png", "2.png"]
        assert set(got) == set(want)
        for key in ("psnr", "ssim", "mse") + (("loss",) if not extra else ()):
            assert abs(got[key] - want[key]) <= 1e-9, (key, got[key], want[key])
        for key in ("psnr", "ssim", "mse"):
            assert np.abs(np.asarray(got["per_image"][key]) - np.asarray(want["per_image"][key])).max() <= 1e-9
