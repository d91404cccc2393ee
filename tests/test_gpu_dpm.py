"""DPM-Solver++ 2M (sampler="dpmpp_2m") on the MI355X: the step kernel against its fp32 NumPy twin, the engine's loop against the
same steps driven from Python, graph capture and replay, LLIE_NO_GRAPH, frame mode, guidance, tiles, evaluation and the trainer,
and the two existing samplers, which must be what they were.

Bounds.  The step kernel and every loop are compared on the bits: the kernel runs dpm.dpm_step_f32's operations in its order, and
the engine's loop launches the kernels the Python composition launches, on the same values.  The fp32 loop against
dpm_enhance_host (float64 steps around the same device network): test_gpu_ddim.py's bar for that comparison, 3.1e-5 x max|reference
latents of that step|, times max(1, max_i (|k_x| + |k_0| + |k_1|)) of the schedule -- a step forms its result from three terms
with those weights, where DDIM's weights sum to about 1."""
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
DPM = importlib.import_module("cv-diffusion-model_amd.dpm")
native = importlib.import_module("cv-diffusion-model_amd._native")

F = np.float32
LOOP_BAR = 3.1e-5  # tests/test_gpu_ddim.py
SAMPLER = "dpmpp_2m"
W = 2.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_scheduler(ptype):
    return M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type=ptype, rescale_betas_zero_snr=True)


_MODELS = {}


def small64(dev, ptype="epsilon"):
    """small at 64 x 64 with the oracle's synthetic weights, built once per prediction type."""
    if ptype not in _MODELS:
        spec = oracle.make_spec("small", 64)
        sd = oracle.synth_state_dict(oracle.param_shapes(spec))
        m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4, scheduler=make_scheduler(ptype))
        m.load_state_dict(sd)
        _MODELS[ptype] = m.to(dev).eval()
    return _MODELS[ptype]


def inputs(dev, b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(b, 3, h, w, generator=g) * 0.6 - 1.0
    return low.to(dev), torch.randn(1, b, 3, h, w, generator=g).to(dev)


class compute_dtype:
    def __init__(self, model, cd):
        self.model, self.cd = model, cd

    def __enter__(self):
        self.model.compute_dtype = self.cd

    def __exit__(self, *exc):
        self.model.compute_dtype = None


def cache_entries(m, b, dev):
    return native.lib().llie_graph_cache_entries(m.unet._prepare(b, dev)[0].h)


def dpm_step(out, x, hist, prev, clamped, coef, dev):
    n = x.numel()
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        native.check(native.lib().llie_dpm_step(ptr(out), ptr(x), ptr(hist), ptr(prev), ptr(clamped), n, coef,
                                                torch.cuda.current_stream(dev).cuda_stream), "llie_dpm_step")


def composition(m, low, x_init, n, frame=False, guidance=None):
    """The loop from public pieces: `unet.forward_split`, (the guidance combination,) llie_dpm_step with `dpm_schedule`'s
    coefficients -> (enhanced, latents after each step, the network output of each step)."""
    dev, b = low.device, low.shape[0]
    ts, coefs = m.dpm_schedule(n)
    x, hist = x_init, torch.empty_like(x_init)
    enhanced = torch.empty_like(x_init)
    inter, preds = [], []
    with torch.no_grad():
        for i, t in enumerate(ts):
            tt = torch.full((b,), t, dtype=torch.long, device=dev)
            out = m.unet.forward_split(x, low, tt, uniform_t=True, frame=frame)
            if guidance is not None:
                o_u = m.unet.forward_split(x, torch.zeros_like(low), tt, uniform_t=True, frame=frame)
                d = out - o_u
                p = d * guidance
                out = o_u + p
            prev = torch.empty_like(x)
            dpm_step(out, x, hist, prev, enhanced if i == n - 1 else None, coefs[i], dev)
            preds.append(out)
            inter.append(prev)
            x = prev
    return enhanced, inter, preds


# ------------------------------------------------------------------ 1. the step kernel, on the bits
SENTINEL = 777.0


def guarded(values, off, dev):
    """`values` inside a buffer of sentinels, starting `off` floats into it (off = 1: 4-byte but not 16-byte aligned)."""
    buf = torch.full((values.size + 8,), SENTINEL, dtype=torch.float32, device=dev)
    buf[off:off + values.size] = torch.from_numpy(values).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:off + values.size]


def untouched(buf, off, n):
    host = buf.cpu().numpy()
    return bool((host[:off] == SENTINEL).all() and (host[off + n:] == SENTINEL).all())


@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
def test_step_kernel_bitwise(dev, ptype):
    m = M.LowLightDiffusion(unet_variant="small", image_size=64, scheduler=make_scheduler(ptype))
    _, sched = m.dpm_schedule(8)
    c = sched[3]
    cases = {"order 1": sched[0], "order 2": c, "final": sched[-1],
             "final, order 2": native.DpmCoef(c.sqrt_alpha_t, c.sqrt_beta_t, c.k_x, c.k_0, c.k_1, c.v_prediction, 2, 1)}
    assert (sched[0].order, c.order, sched[-1].order, sched[-1].is_last) == (1, 2, 1, 1)
    rng = np.random.default_rng(3 + len(ptype))
    for n in (1, 3, 4, 5, 1027):
        x, out, h0 = ((rng.standard_normal(n) * s).astype(F) for s in (2.0, 1.5, 0.8))
        for off in (0, 1):  # float4 items + tail; every element a scalar item
            for name, coef in cases.items():
                want_prev, want_x0 = DPM.dpm_step_f32(out, x, h0, coef)
                # nothing aliases: every output is written, the inputs are unchanged, nothing outside the tensors is touched
                bufs = [guarded(v, off, dev) for v in (out, x, h0, np.zeros(n, F), np.zeros(n, F))]
                (_, d_out), (_, d_x), (_, d_h), (_, d_prev), (_, d_cl) = bufs
                dpm_step(d_out, d_x, d_h, d_prev, d_cl, coef, dev)
                tag = (ptype, n, off, name)
                assert np.array_equal(d_prev.cpu().numpy(), want_prev), tag
                assert np.array_equal(d_h.cpu().numpy(), want_x0), tag
                assert np.array_equal(d_cl.cpu().numpy(), np.clip(want_prev, -1, 1)), tag
                assert np.array_equal(d_out.cpu().numpy(), out) and np.array_equal(d_x.cpu().numpy(), x), tag
                assert all(untouched(b, off, n) for b, _ in bufs), tag
                # prev_out aliases sample, hist is updated in place, no clamped output
                bufs = [guarded(v, off, dev) for v in (out, x, h0)]
                (_, d_out), (_, d_x), (_, d_h) = bufs
                dpm_step(d_out, d_x, d_h, d_x, None, coef, dev)
                assert np.array_equal(d_x.cpu().numpy(), want_prev) and np.array_equal(d_h.cpu().numpy(), want_x0), tag
                assert np.array_equal(d_out.cpu().numpy(), out) and all(untouched(b, off, n) for b, _ in bufs), tag
        # the final first-order step takes no history
        (_, d_out), (_, d_x), (_, d_prev) = (guarded(v, 0, dev) for v in (out, x, np.zeros(n, F)))
        dpm_step(d_out, d_x, None, d_prev, None, sched[-1], dev)
        assert np.array_equal(d_prev.cpu().numpy(), DPM.dpm_step_f32(out, x, None, sched[-1])[0])


def test_step_kernel_refusals(dev):
    x = torch.zeros(16, device=dev)
    L, st = native.lib(), torch.cuda.current_stream(dev).cuda_stream
    p = x.data_ptr()
    ok = native.DpmCoef(0.8, 0.6, 0.9, 0.3, -0.1, 0, 2, 0)
    assert L.llie_dpm_step(p, p, p, p, None, 16, ok, st) == 0
    assert L.llie_dpm_step(p, p, None, p, None, 16, ok, st) == native.ERR_ARG            # a second-order step reads the history
    assert L.llie_dpm_step(p, p, p, p, None, 16, native.DpmCoef(0.8, 0.6, 0.9, 0.3, -0.1, 0, 3, 0), st) == native.ERR_ARG
    assert L.llie_dpm_step(p, p, p, p, None, 16, native.DpmCoef(0.8, 0.6, float("nan"), 0.3, -0.1, 0, 2, 0), st) == native.ERR_ARG
    assert L.llie_dpm_step(p, p, p, p + 2, None, 8, ok, st) == native.ERR_ARG            # not 4-byte aligned
    assert L.llie_dpm_step(p, p, p, p, None, 0, ok, st) == native.ERR_ARG
    # llie_lcm_step knows no third sampler
    assert L.llie_lcm_step(p, p, None, p, None, None, 16, native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 0, 2), st) == native.ERR_ARG


# ------------------------------------------------------------------ 2. the fp32 loop
@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_fp32_loop(dev, ptype, n):
    m = small64(dev, ptype)
    low, noise = inputs(dev, 2, 64, 64, seed=100 + n)
    out = m.enhance(low, n, noise=noise, return_intermediate=True, return_noise_pred=True, sampler=SAMPLER)
    want_e, want_i, want_p = composition(m, low, noise[0], n)
    assert len(out.intermediate) == len(out.noise_pred) == n
    for i in range(n):
        assert torch.equal(out.noise_pred[i], want_p[i]), i
        assert torch.equal(out.intermediate[i], want_i[i]), i
    assert torch.equal(out.enhanced, want_e) and torch.equal(out.enhanced, out.intermediate[-1].clamp(-1, 1))
    assert torch.equal(m.enhance(low, n, noise=noise, sampler=SAMPLER), out.enhanced)  # in place, without the per-step outputs
    only_inter = m.enhance(low, n, noise=noise, return_intermediate=True, sampler=SAMPLER)
    assert all(torch.equal(a, b) for a, b in zip(only_inter.intermediate, want_i))
    only_preds = m.enhance(low, n, noise=noise, return_noise_pred=True, sampler=SAMPLER)
    assert all(torch.equal(a, b) for a, b in zip(only_preds.noise_pred, want_p)) and torch.equal(only_preds.enhanced, want_e)

    # against the host definition (float64 steps) around the same device network
    def unet_fn(lat, lw, t):
        tt = torch.full((lat.shape[0],), t, dtype=torch.long, device=dev)
        with torch.no_grad():
            return m.unet.forward_split(torch.from_numpy(lat).to(dev), torch.from_numpy(lw).to(dev), tt, uniform_t=True).cpu().numpy()

    ref = M.dpm_enhance_host(unet_fn, low.cpu().numpy(), noise[0].cpu().numpy(), n, m.scheduler.alphas_cumprod.numpy(),
                             ptype == "v_prediction")
    assert ref["timesteps"] == m.dpm_schedule(n)[0]
    weight = max(1.0, max(abs(c.k_x) + abs(c.k_0) + abs(c.k_1) for c in ref["coefficients"]))
    worst = max(np.abs(out.intermediate[i].cpu().numpy().astype(np.float64) - r).max() / np.abs(r).max()
                for i, r in enumerate(ref["intermediate"]))
    print(f"{ptype} n={n}: worst max-abs / max|ref| over the steps {worst:.3e} (bar {LOOP_BAR * weight:.2e}, weight {weight:.3f})")
    assert worst <= LOOP_BAR * weight


# ------------------------------------------------------------------ 3. the 2-byte engines: composition, capture, replay
@pytest.mark.parametrize("b", [2, 16])  # 16: the captured loop splits the batch into two concurrent branches
@pytest.mark.parametrize("cd", ["fp16", "bf16"])
def test_two_byte_engines(dev, cd, b):
    m = small64(dev)
    low, noise = inputs(dev, b, 64, 64, seed=200 + b)
    with compute_dtype(m, cd):
        want_e, want_i, want_p = composition(m, low, noise[0], 4)
        before = cache_entries(m, b, dev)
        plain = [m.enhance(low, 4, noise=noise, sampler=SAMPLER) for _ in range(3)]  # eager, capture, replay
        assert cache_entries(m, b, dev) == before + 1
        full = [m.enhance(low, 4, noise=noise, return_intermediate=True, return_noise_pred=True, sampler=SAMPLER) for _ in range(3)]
        assert cache_entries(m, b, dev) == before + 2
        for run in plain:
            assert torch.equal(run, want_e)
        for run in full:
            assert torch.equal(run.enhanced, want_e)
            assert all(torch.equal(x, y) for x, y in zip(run.intermediate, want_i))
            assert all(torch.equal(x, y) for x, y in zip(run.noise_pred, want_p))
        assert bool(torch.isfinite(want_e).all()) and float(want_e.abs().max()) <= 1.0
        # past graph_max_steps the loop runs as plain launches: same bits, no new entry
        entries = cache_entries(m, b, dev)
        native.check(native.lib().llie_tune(b"graph_max_steps", 3))
        try:
            again = [m.enhance(low, 4, noise=noise, sampler=SAMPLER) for _ in range(2)]
            assert cache_entries(m, b, dev) == entries
        finally:
            native.check(native.lib().llie_tune(b"graph_max_steps", 0))  # the default
        assert all(torch.equal(o, want_e) for o in again)


def test_noise_and_generator(dev):
    m = small64(dev)
    low, noise = inputs(dev, 2, 64, 64, seed=7)
    with pytest.raises(ValueError, match="initial latents"):
        m.enhance(low, 6, noise=torch.cat([noise] * 6), sampler=SAMPLER)
    outs = []
    for seed in (1, 2):  # a generator seeds the only draw: the global generator is neither read nor advanced
        torch.manual_seed(seed)
        state = torch.cuda.get_rng_state(dev)
        outs.append(m.enhance(low, 6, generator=torch.Generator(device=dev).manual_seed(5), sampler=SAMPLER))
        assert torch.equal(torch.cuda.get_rng_state(dev), state)
    assert torch.equal(outs[0], outs[1])
    drawn = torch.empty(1, 2, 3, 64, 64, device=dev).normal_(generator=torch.Generator(device=dev).manual_seed(5))
    assert torch.equal(m.enhance(low, 6, noise=drawn, sampler=SAMPLER), outs[0])
    limit = DPM.dpm_max_steps(m.scheduler.alphas_cumprod.numpy())
    with pytest.raises(ValueError, match="ddim"):
        m.enhance(low, limit + 1, sampler=SAMPLER)
    out = m.enhance(low, limit, noise=noise, sampler=SAMPLER)  # the longest schedule the table allows
    assert bool(torch.isfinite(out).all())


def test_c_entry_refuses_bad_schedules(dev):
    m = small64(dev)
    low, noise = inputs(dev, 2, 64, 64, seed=80)
    ts, coefs = m.dpm_schedule(4)
    h, ws, nbytes = m.unet._prepare(2, dev, enhance_steps=8)
    t_dev = torch.tensor(ts, dtype=torch.long).repeat_interleave(2).to(dev)
    out = torch.empty(2, 3, 64, 64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(cs):
        arr = (native.DpmCoef * 4)(*cs)
        return native.lib().llie_enhance_dpm(h.h, low.data_ptr(), noise.data_ptr(), t_dev.data_ptr(), arr, 4, out.data_ptr(), None, None,
                                             2, ws.data_ptr(), nbytes, st)

    assert run(coefs) == 0
    good = out.clone()
    c = coefs[1]
    assert run([c] + coefs[1:]) == native.ERR_ARG and "order" in native.last_error()  # the first step has no history to read
    assert run([coefs[0], native.DpmCoef(c.sqrt_alpha_t, c.sqrt_beta_t, c.k_x, c.k_0, c.k_1, 0, 3, 0)] + coefs[2:]) == native.ERR_ARG
    assert run([coefs[0], native.DpmCoef(c.sqrt_alpha_t, c.sqrt_beta_t, float("inf"), c.k_0, c.k_1, 0, 2, 0)] + coefs[2:]) == native.ERR_ARG
    assert run(coefs) == 0 and torch.equal(out, good)
    assert torch.equal(good, m.enhance(low, 4, noise=noise, sampler=SAMPLER))


# ------------------------------------------------------------------ 4. LLIE_NO_GRAPH, in a fresh process
CHILD = """
import importlib, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import oracle
M = importlib.import_module("cv-diffusion-model_amd")
dev = torch.device("cuda:0")
spec = oracle.make_spec("small", 64)
sched = M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type="epsilon", rescale_betas_zero_snr=True)
m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4, scheduler=sched, compute_dtype="fp16")
m.load_state_dict(oracle.synth_state_dict(oracle.param_shapes(spec)))
m = m.to(dev).eval()
g = torch.Generator().manual_seed(300)
low = (torch.rand(2, 3, 64, 64, generator=g) * 0.6 - 1.0).to(dev)
noise = torch.randn(1, 2, 3, 64, 64, generator=g).to(dev)
runs = [m.enhance(low, 4, noise=noise, sampler="dpmpp_2m") for _ in range(3)]
h = m.unet._prepare(2, dev)[0].h
native = importlib.import_module("cv-diffusion-model_amd._native")
assert native.lib().llie_graph_cache_entries(h) == 0, "LLIE_NO_GRAPH=1 captured a graph"
assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
np.save(sys.argv[2], runs[0].cpu().numpy())
"""


def test_no_graph_environment(dev, tmp_path):
    m = small64(dev)
    low, noise = inputs(dev, 2, 64, 64, seed=300)
    with compute_dtype(m, "fp16"):
        captured = [m.enhance(low, 4, noise=noise, sampler=SAMPLER) for _ in range(3)][-1]
    env = dict(os.environ, LLIE_NO_GRAPH="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "plain.npy")], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert np.array_equal(np.load(tmp_path / "plain.npy"), captured.cpu().numpy())


# ------------------------------------------------------------------ 5. frame mode
def test_frame_mode(dev):
    m = small64(dev)
    low, noise = inputs(dev, 2, 64, 64, seed=81)
    a = m.enhance(low, 4, noise=noise, return_intermediate=True, sampler=SAMPLER)
    b = m.enhance_frame(low, 4, noise=noise, return_intermediate=True, sampler=SAMPLER)
    assert torch.equal(a.enhanced, b.enhanced) and all(torch.equal(x, y) for x, y in zip(a.intermediate, b.intermediate))
    low, noise = inputs(dev, 2, 64, 72, seed=82)
    for cd in ("fp32", "fp16"):
        with compute_dtype(m, cd):
            want_e, want_i, want_p = composition(m, low, noise[0], 4, frame=True)
            out = m.enhance_frame(low, 4, noise=noise, return_intermediate=True, return_noise_pred=True, sampler=SAMPLER)
            assert tuple(out.enhanced.shape) == (2, 3, 64, 72) and torch.equal(out.enhanced, want_e)
            assert all(torch.equal(x, y) for x, y in zip(out.intermediate, want_i))
            assert all(torch.equal(x, y) for x, y in zip(out.noise_pred, want_p))
            for _ in range(3):  # eager, capture, replay
                assert torch.equal(m.enhance_frame(low, 4, noise=noise, sampler=SAMPLER), want_e)
    img = torch.from_numpy((np.random.default_rng(5).random((70, 90, 3)) * 90).astype(np.uint8)).to(dev)
    canvas = torch.randn(1, 3, 72, 96, generator=torch.Generator().manual_seed(6))
    u8 = M.enhance_frame_u8(m, img, 5, noise=canvas, sampler=SAMPLER)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (70, 90, 3)
    assert torch.equal(u8, M.enhance_frame_u8(m, img, 5, noise=canvas, sampler=SAMPLER))
    assert not torch.equal(u8, M.enhance_frame_u8(m, img, 5, noise=canvas, sampler="ddim"))


# ------------------------------------------------------------------ 6. guidance
@pytest.mark.parametrize("cd", ["fp32", "fp16"])
def test_guidance(dev, cd):
    m = small64(dev)
    low, noise = inputs(dev, 2, 64, 64, seed=91)
    with compute_dtype(m, cd):
        want_e, want_i, want_p = composition(m, low, noise[0], 5, guidance=W)
        outs = {}
        for passes in (None, 1, 2):
            out = m.enhance(low, 5, noise=noise, return_intermediate=True, return_noise_pred=True, sampler=SAMPLER, guidance_scale=W,
                            _passes=passes)
            assert torch.equal(out.enhanced, want_e), passes
            assert all(torch.equal(x, y) for x, y in zip(out.intermediate, want_i)), passes
            assert all(torch.equal(x, y) for x, y in zip(out.noise_pred, want_p)), passes
            outs[passes] = m.enhance(low, 5, noise=noise, sampler=SAMPLER, guidance_scale=W, _passes=passes)
            assert torch.equal(outs[passes], want_e)
        assert torch.equal(outs[1], outs[2])
        base = m.enhance(low, 5, noise=noise, sampler=SAMPLER, return_intermediate=True)
        assert not torch.equal(base.enhanced, want_e)  # guidance does something
        for w in (None, 1.0):  # the unguided call, bit for bit
            out = m.enhance(low, 5, noise=noise, sampler=SAMPLER, return_intermediate=True, guidance_scale=w)
            assert torch.equal(out.enhanced, base.enhanced) and all(torch.equal(x, y) for x, y in zip(out.intermediate, base.intermediate))


# ------------------------------------------------------------------ 7. tiles
def test_enhance_tiled(dev):
    m = small64(dev)
    h, w, v = 80, 104, 8
    img_np = (np.random.default_rng(32).random((h, w, 3)) * 90).astype(np.uint8)
    img = torch.from_numpy(img_np).to(dev)
    canvas = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(33))
    a = M.enhance_tiled(m, img, 4, overlap=v, tile_batch=3, noise=canvas, sampler=SAMPLER)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (h, w, 3) and float(a.float().std()) > 0
    low = T.gather_tiles_array(img_np, 64, v)
    draws = torch.stack([canvas[:, :, oy:oy + 64, ox:ox + 64] for oy in T.tile_origins(h, 64, v) for ox in T.tile_origins(w, 64, v)], dim=1)
    tiles = m.enhance(torch.from_numpy(low).to(dev), 4, noise=draws.to(dev), sampler=SAMPLER).cpu().numpy()
    assert np.array_equal(a.cpu().numpy(), T.blend_tiles_array(tiles, (h, w), v))
    # frame tiles go through enhance_frame
    b = M.enhance_tiled(m, img, 4, tile=(64, 72), noise=canvas, sampler=SAMPLER)
    assert tuple(b.shape) == (h, w, 3) and torch.equal(b, M.enhance_tiled(m, img, 4, tile=(64, 72), noise=canvas, sampler=SAMPLER))
    with pytest.raises(ValueError, match=r'sync="latents".*dpmpp_2m'):
        M.enhance_tiled(m, img, 4, overlap=v, noise=canvas, sync="latents", sampler=SAMPLER)
    with pytest.raises(ValueError):
        M.enhance_tiled(m, img, 4, overlap=v, noise=torch.randn(4, 3, h, w), sampler=SAMPLER)  # the LCM loop's canvas


# ------------------------------------------------------------------ 8. evaluation and the trainer
def pair_store(dev, n=2):
    rng = np.random.default_rng(41)
    high = [rng.integers(0, 256, size=(72, 80, 3), dtype=np.uint8) for _ in range(n)]
    return M.DeviceFrameStore([f // 5 for f in high], high, device=dev, names=[f"p{i}.png" for i in range(n)])


def test_evaluate(dev):
    m = small64(dev)
    store = pair_store(dev)
    loader = M.DevicePairLoader(store, 2, 64, "val")
    a = M.evaluate(m, loader, sampler=SAMPLER, num_inference_steps=8)
    assert a["n"] == 2 and np.isfinite([a["psnr"], a["ssim"], a["mse"], a["loss"]]).all()
    assert a == M.evaluate(m, loader, sampler=SAMPLER, num_inference_steps=8)
    assert a["psnr"] != M.evaluate(m, loader, sampler="ddim", num_inference_steps=8)["psnr"]
    # the recipe of the docstring: one entry of noise per batch
    batch = next(iter(loader))
    noise = torch.randn(1, 2, 3, 64, 64, generator=torch.Generator(device=dev).manual_seed(0), device=dev)
    want = M.image_metrics(m.enhance(batch["low_light"], 8, noise=noise, sampler=SAMPLER), batch["normal_light"], data_range=(-1.0, 1.0))
    assert abs(a["per_image"]["psnr"][0] - float(want.psnr[0])) <= 1e-9
    for mode, kw in (("tiled", {"overlap": 8}), ("frame", {})):
        r1 = M.evaluate_full_resolution(m, store, num_inference_steps=5, mode=mode, sampler=SAMPLER, **kw)
        assert r1 == M.evaluate_full_resolution(m, store, num_inference_steps=5, mode=mode, sampler=SAMPLER, **kw)
        assert np.isfinite([r1["psnr"], r1["ssim"]]).all()
    with pytest.raises(ValueError, match="dpmpp_2m"):
        M.evaluate_full_resolution(m, store, num_inference_steps=5, sync="latents", sampler=SAMPLER)


def test_trainer_validation(dev, tmp_path):
    torch.manual_seed(0)
    model = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4).to(dev)
    store = pair_store(dev, 4)
    cfg = M.TrainingConfig(image_size=64, batch_size=2, epochs=1, use_amp=False, use_ema=False, scheduler_type="cosine", warmup_epochs=0,
                           log_interval=0, save_interval=100, sample_interval=1, seed=3, progress=False, output_dir=str(tmp_path / "out"),
                           checkpoint_dir=str(tmp_path / "ckpt"))
    trainer = M.LowLightTrainer(model, M.DevicePairLoader(store, 2, 64, "train", 3), M.DevicePairLoader(store, 2, 64, "val", 3), cfg,
                                val_sampler=SAMPLER, val_steps=8)
    trainer.train()  # one epoch: training, validation and the sample sheet
    first = dict(trainer.last_validation)
    assert np.isfinite([first["psnr"], first["ssim"], first["loss"]]).all()
    assert first == M.evaluate(model, trainer.val_loader, num_inference_steps=8, seed=3, sampler=SAMPLER)
    sheet = trainer.generate_samples(0)
    assert sheet.exists() and trainer.generate_samples(0).read_bytes() == sheet.read_bytes()


# ------------------------------------------------------------------ 9. the existing samplers are what they were
@pytest.mark.parametrize("cd", ["fp32", "fp16"])
def test_existing_samplers_unchanged(dev, cd):
    """`enhance` with the default sampler and with "ddim" against llie_enhance called directly with the scheduler's own
    coefficients: the route those samplers took before the loop learnt a second coefficient type."""
    m = small64(dev)
    low, noise1 = inputs(dev, 2, 64, 64, seed=95)
    noise4 = torch.randn(4, 2, 3, 64, 64, generator=torch.Generator().manual_seed(96)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with compute_dtype(m, cd):
        for sampler, n, noise in (("lcm", 4, noise4), ("ddim", 6, noise1)):
            runs = [m.enhance(low, n, noise=noise, return_intermediate=True, return_noise_pred=True, **({} if sampler == "lcm" else {"sampler": sampler}))
                    for _ in range(3)]
            if sampler == "lcm":
                m.scheduler.set_timesteps(n, device=dev)
                ts = list(m.scheduler._timestep_list)
                coefs = [m.scheduler.step_coefficients(t) for t in ts]
                assert torch.equal(runs[0].enhanced, m.enhance(low, n, noise=noise, sampler="lcm"))
            else:
                ts, coefs = m.ddim_schedule(n)
            h, ws, nbytes = m.unet._prepare(2, dev, enhance_steps=8)
            t_dev = torch.tensor(ts, dtype=torch.long).repeat_interleave(2).to(dev)
            out, inter, preds = torch.empty(2, 3, 64, 64, device=dev), torch.empty(n, 2, 3, 64, 64, device=dev), torch.empty(n, 2, 3, 64, 64, device=dev)
            arr = (native.StepCoef * n)(*coefs)
            for _ in range(3):  # eager, capture, replay
                native.check(native.lib().llie_enhance(h.h, low.data_ptr(), noise.data_ptr(), t_dev.data_ptr(), arr, n, out.data_ptr(), inter.data_ptr(),
                                                       preds.data_ptr(), 2, ws.data_ptr(), nbytes, st), "llie_enhance")
                for run in runs:
                    assert torch.equal(run.enhanced, out), sampler
                    assert all(torch.equal(run.intermediate[i], inter[i]) and torch.equal(run.noise_pred[i], preds[i]) for i in range(n)), sampler
            # the step of every latent is the scheduler's own step kernel on that step's output
            x = noise[0]
            for i, t in enumerate(ts):
                if sampler == "lcm":
                    nxt = m.scheduler.step(runs[0].noise_pred[i], t, x, noise=noise[i + 1] if i + 1 < n else None).prev_sample
                else:
                    nxt = m.scheduler.ddim_step(runs[0].noise_pred[i], t, t - 1000 // n, x).prev_sample
                if cd == "fp32":  # the 2-byte engines apply the step in the output head's epilogue, within rounding of the kernel
                    assert torch.equal(nxt, runs[0].intermediate[i]), (sampler, i)
                x = runs[0].intermediate[i]
        assert not torch.equal(m.enhance(low, 6, noise=noise1, sampler=SAMPLER), m.enhance(low, 6, noise=noise1, sampler="ddim"))
