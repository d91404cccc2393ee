"""The deterministic DDIM sampler on the MI355X: the step kernel, the fp32 loop, the fused output-head epilogue of the 2-byte
engines, determinism and graph replay, frame mode, tiles, and evaluation / the trainer's validation.

Bounds.  One DDIM step is a handful of fp32 operations on the terms below, each rounded to half an ulp, with scalars that are
themselves fp32 roundings of the float64 ones; the step's error is below 8 * 2^-24 times the sum of the absolute terms:
  epsilon:  alpha_p (|x| + sigma_t |out|) / alpha_t + sigma_p |out|            (final step: (|x| + sigma_t |out|) / alpha_t)
  v:        alpha_p (alpha_t |x| + sigma_t |out|) + sigma_p (alpha_t |out| + sigma_t |x|)   (final: alpha_t |x| + sigma_t |out|)
The fp32 loop against the CPU oracle: 3.1e-5 x max|reference latents of that step| -- the project's 1e-3 bar on latents of
magnitude ~32 (test_gpu_parity.py) made relative, because DDIM latents grow with synthetic weights."""
import importlib

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
T = importlib.import_module("cv-diffusion-model_amd.tiling")
P = importlib.import_module("cv-diffusion-model_amd.pipeline")
native = importlib.import_module("cv-diffusion-model_amd._native")

F = np.float32
EPS8 = 8 * 2.0 ** -24
LOOP_BAR = 3.1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_scheduler(ptype):
    return M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type=ptype, rescale_betas_zero_snr=True)


_MODELS = {}


def small64(dev, ptype="epsilon"):
    """small at 64 x 64 with the oracle's synthetic weights; (model, state dict, spec), built once per prediction type."""
    if ptype not in _MODELS:
        spec = oracle.make_spec("small", 64)
        sd = oracle.synth_state_dict(oracle.param_shapes(spec))
        m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4, scheduler=make_scheduler(ptype))
        m.load_state_dict(sd)
        _MODELS[ptype] = (m.to(dev).eval(), sd, spec)
    return _MODELS[ptype]


def inputs(b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(b, 3, h, w, generator=g) * 0.6 - 1.0
    return low, torch.randn(b, 3, h, w, generator=g)


def oracle_fn(sd, spec):
    def unet_fn(lat, low, t):
        with torch.no_grad():
            tt = torch.full((lat.shape[0],), t, dtype=torch.long)
            return oracle.unet_forward(sd, spec, torch.cat([torch.from_numpy(lat), torch.from_numpy(low)], 1), tt).numpy()
    return unet_fn


_REFS = {}


def reference(dev, ptype, h, w, n):
    """ddim_enhance_host over the CPU oracle at 2 x h x w, computed once and shared (never modified)."""
    key = (ptype, h, w, n)
    if key not in _REFS:
        m, sd, spec = small64(dev, ptype)
        low, x_init = inputs(2, h, w, seed=1000 * h + w + n)
        ref = M.ddim_enhance_host(oracle_fn(sd, spec), low.numpy(), x_init.numpy(), n, m.scheduler.alphas_cumprod.numpy(),
                                  ptype == "v_prediction")
        _REFS[key] = (low, x_init, ref)
    return _REFS[key]


def step_bound(sched, out, x, t, p):
    """The derived bound of the module docstring, per element (float64 arrays)."""
    acp = sched.alphas_cumprod.numpy().astype(np.float64)
    at, st = np.sqrt(acp[t]), np.sqrt(1 - acp[t])
    out, x = np.abs(np.asarray(out, dtype=np.float64)), np.abs(np.asarray(x, dtype=np.float64))
    if sched.config.prediction_type == "v_prediction":
        x0, e = at * x + st * out, at * out + st * x
    else:
        x0, e = (x + st * out) / at, out
    if p < 0:
        return EPS8 * x0
    return EPS8 * (np.sqrt(acp[p]) * x0 + np.sqrt(1 - acp[p]) * e)


class compute_dtype:
    def __init__(self, model, cd):
        self.model, self.cd = model, cd

    def __enter__(self):
        self.model.compute_dtype = self.cd

    def __exit__(self, *exc):
        self.model.compute_dtype = None


def cache_entries(m, b, dev):
    return native.lib().llie_graph_cache_entries(m.unet._prepare(b, dev)[0].h)


# ------------------------------------------------------------------ 1. the step kernel
@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("t", [0, 20, 500, 980])
def test_step_kernel(dev, ptype, t):
    s = make_scheduler(ptype)
    rng = np.random.default_rng(t + 1)
    x, out = (rng.standard_normal((2, 3, 8, 8)) * 3).astype(F), (rng.standard_normal((2, 3, 8, 8)) * 2).astype(F)
    x_d, out_d = torch.from_numpy(x).to(dev), torch.from_numpy(out).to(dev)
    for p in (max(t - 20, 0), -1):  # non-final (at t = 0 the step 0 -> 0), final
        want = s.ddim_step_host(out, t, p, x)
        res = s.ddim_step(out_d, t, p, x_d)
        got = res.prev_sample.cpu().numpy().astype(np.float64)
        bound = step_bound(s, out, x, t, p)
        ratio = float((np.abs(got - want) / bound).max())
        print(f"{ptype} t={t} -> {p}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0
        x0 = res.pred_original_sample.cpu().numpy().astype(np.float64)
        assert (np.abs(x0 - s.ddim_step_host(out, t, -1, x)) <= step_bound(s, out, x, t, -1)).all()
        if p < 0:
            assert torch.equal(res.prev_sample, res.pred_original_sample)
        elif ptype == "epsilon":
            tt = torch.full((2,), t, dtype=torch.long, device=dev)
            pp = torch.full((2,), p, dtype=torch.long, device=dev)
            tgt = P.consistency_target(s, x_d, out_d, tt, pp).cpu().numpy().astype(np.float64)
            assert (np.abs(tgt - want) <= bound).all() and (np.abs(tgt - got) <= bound).all()
    assert np.array_equal(x_d.cpu().numpy(), x) and np.array_equal(out_d.cpu().numpy(), out)  # inputs are read only


def test_step_kernel_refusals(dev):
    x = torch.zeros(16, device=dev)
    L, st = native.lib(), torch.cuda.current_stream(dev).cuda_stream
    ok = native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 0, 1)
    assert L.llie_lcm_step(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), None, None, 16, ok, st) == 0  # DDIM: no noise on any step
    for bad in (native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 1, 1), native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 0, 2)):
        assert L.llie_lcm_step(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, 16, bad, st) == native.ERR_ARG
    assert L.llie_lcm_step(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), None, None, 16,
                           native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 0, 0), st) == native.ERR_ARG  # the LCM step still needs it


# ------------------------------------------------------------------ 2. the fp32 loop against the CPU oracle
@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("n", [4, 10])
def test_fp32_loop_vs_oracle(dev, ptype, n):
    """Every step's latents within 3.1e-5 x max|reference latents of that step|.  Worst max-abs / max|ref| over the steps, measured
    on an MI355X: epsilon n = 4 1.308e-06, n = 10 1.203e-06 (last latents up to 24.4 / 99.3); v n = 4 1.473e-06, n = 10 8.183e-07."""
    m = small64(dev, ptype)[0]
    low, x_init, ref = reference(dev, ptype, 64, 64, n)
    out = m.enhance(low.to(dev), n, noise=x_init[None].to(dev), return_intermediate=True, return_noise_pred=True, sampler="ddim")
    assert len(out.intermediate) == n == len(out.noise_pred)
    worst = 0.0
    for i in range(n):
        r = ref["intermediate"][i]
        err = np.abs(out.intermediate[i].cpu().numpy().astype(np.float64) - r).max()
        worst = max(worst, err / np.abs(r).max())
    print(f"{ptype} n={n}: worst max-abs / max|ref| over the steps {worst:.3e} (bar {LOOP_BAR:.1e}); "
          f"last latents up to {np.abs(ref['intermediate'][-1]).max():.1f}")
    assert worst <= LOOP_BAR
    last = out.intermediate[-1]
    assert torch.equal(out.enhanced, last.clamp(-1, 1))


# ------------------------------------------------------------------ 3. the fused epilogue of the 2-byte engines
@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("cd", ["fp16", "bf16"])
def test_fused_epilogue(dev, ptype, cd):
    """Each step's latents are the DDIM step of that step's own noise prediction: the epilogue, apart from network precision."""
    m = small64(dev, ptype)[0]
    low, x_init = inputs(2, 64, 64, seed=77)
    ts, _ = m.ddim_schedule(4)
    with compute_dtype(m, cd):
        out = m.enhance(low.to(dev), 4, noise=x_init[None].to(dev), return_intermediate=True, return_noise_pred=True, sampler="ddim")
        plain = m.enhance(low.to(dev), 4, noise=x_init[None].to(dev), sampler="ddim")
    x = x_init.numpy()
    worst = 0.0
    for i, t in enumerate(ts):
        p = t - 250
        pred = out.noise_pred[i].cpu().numpy()
        want = m.scheduler.ddim_step_host(pred, t, p, x)
        got = out.intermediate[i].cpu().numpy()
        worst = max(worst, float((np.abs(got.astype(np.float64) - want) / step_bound(m.scheduler, pred, x, t, p)).max()))
        x = got
    print(f"{cd} {ptype}: worst error / bound over 4 steps {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(out.enhanced, out.intermediate[-1].clamp(-1, 1)) and torch.equal(plain, out.enhanced)


# ------------------------------------------------------------------ 4. determinism and replay
@pytest.mark.parametrize("cd", [None, "fp16"])
def test_determinism_and_replay(dev, cd):
    m = small64(dev)[0]
    low, x_init = inputs(2, 64, 64, seed=78)
    low_d, noise = low.to(dev), x_init[None].to(dev)
    with compute_dtype(m, cd):
        m.enhance(low_d, 4, noise=torch.cat([noise] * 4))  # the LCM loop's entry exists already: DDIM's key is its own
        before = cache_entries(m, 2, dev)
        runs = [m.enhance(low_d, 6, noise=noise, sampler="ddim") for _ in range(3)]  # eager, capture, replay
        assert cache_entries(m, 2, dev) == before + 1
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
        assert bool(torch.isfinite(runs[0]).all()) and runs[0].abs().max() <= 1.0
        # one entry of noise only
        with pytest.raises(ValueError, match="initial latents"):
            m.enhance(low_d, 6, noise=torch.cat([noise] * 6), sampler="ddim")
        # a generator seeds the only draw: the global generator is neither read nor advanced
        outs = []
        for seed in (1, 2):
            torch.manual_seed(seed)
            state = torch.cuda.get_rng_state(dev)
            outs.append(m.enhance(low_d, 6, generator=torch.Generator(device=dev).manual_seed(5), sampler="ddim"))
            assert torch.equal(torch.cuda.get_rng_state(dev), state)
        assert torch.equal(outs[0], outs[1])
        g = torch.Generator(device=dev).manual_seed(5)
        drawn = torch.empty(1, 2, 3, 64, 64, device=dev).normal_(generator=g)
        assert torch.equal(m.enhance(low_d, 6, noise=drawn, sampler="ddim"), outs[0])
        # loops past graph_max_steps run as plain launches: same bits, no new entry
        entries = cache_entries(m, 2, dev)
        native.check(native.lib().llie_tune(b"graph_max_steps", 5))
        try:
            plain = [m.enhance(low_d, 6, noise=noise, sampler="ddim") for _ in range(3)]
            assert cache_entries(m, 2, dev) == entries
        finally:
            native.check(native.lib().llie_tune(b"graph_max_steps", 0))  # the default
        assert all(torch.equal(o, runs[0]) for o in plain)
        # the LCM default is what it was: the call without `sampler` and the one naming it
        lcm_noise = torch.randn(4, 2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev)
        assert torch.equal(m.enhance(low_d, 4, noise=lcm_noise), m.enhance(low_d, 4, noise=lcm_noise, sampler="lcm"))


def test_long_schedules_run(dev):
    """More steps than the LCM grid allows, and a step count that does not divide T."""
    m = small64(dev, "v_prediction")[0]
    low, x_init = inputs(1, 64, 64, seed=79)
    with compute_dtype(m, "fp16"):
        for n in (1, 7, 60):
            out = m.enhance(low.to(dev), n, noise=x_init[None].to(dev), return_intermediate=True, sampler="ddim")
            assert len(out.intermediate) == n and bool(torch.isfinite(out.enhanced).all())
    with pytest.raises(ValueError, match="999"):
        small64(dev)[0].enhance(low.to(dev), 1000, sampler="ddim")  # epsilon prediction cannot start at alpha-bar 0
    with pytest.raises(ValueError):
        m.enhance(low.to(dev), 1001, sampler="ddim")


def test_c_entry_refuses_mixed_and_clamped_schedules(dev):
    m = small64(dev)[0]
    low, x_init = inputs(2, 64, 64, seed=80)
    low_d, noise = low.to(dev).contiguous(), x_init[None].to(dev).contiguous()
    ts, coefs = m.ddim_schedule(4)
    h, ws, nbytes = m.unet._prepare(2, dev, enhance_steps=8)
    t_dev = torch.tensor(ts, dtype=torch.long).repeat_interleave(2).to(dev)
    out = torch.empty(2, 3, 64, 64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(cs):
        arr = (native.StepCoef * 4)(*cs)
        return native.lib().llie_enhance(h.h, low_d.data_ptr(), noise.data_ptr(), t_dev.data_ptr(), arr, 4, out.data_ptr(), None, None,
                                         2, ws.data_ptr(), nbytes, st)

    assert run(coefs) == 0
    good = out.clone()
    m.scheduler.set_timesteps(4)
    lcm = m.scheduler.step_coefficients(m.scheduler._timestep_list[-1])  # the LCM loop's last step reads no noise either
    assert run(coefs[:3] + [lcm]) == native.ERR_ARG and "LCM or all DDIM" in native.last_error()
    c = coefs[1]
    clamped = native.StepCoef(c.sqrt_alpha_t, c.sqrt_beta_t, c.sqrt_alpha_prev, c.sqrt_beta_prev, 0, 0, 1, 1)
    assert run([coefs[0], clamped] + coefs[2:]) == native.ERR_ARG
    assert run(coefs) == 0 and torch.equal(out, good)
    assert torch.equal(good, m.enhance(low_d, 4, noise=noise, sampler="ddim"))


# ------------------------------------------------------------------ 5. frame mode
def test_frame_mode(dev):
    m = small64(dev)[0]
    low, x_init = inputs(2, 64, 64, seed=81)
    a = m.enhance(low.to(dev), 4, noise=x_init[None].to(dev), return_intermediate=True, sampler="ddim")
    b = m.enhance_frame(low.to(dev), 4, noise=x_init[None].to(dev), return_intermediate=True, sampler="ddim")
    assert torch.equal(a.enhanced, b.enhanced) and all(torch.equal(x, y) for x, y in zip(a.intermediate, b.intermediate))
    low, x_init, ref = reference(dev, "epsilon", 64, 96, 4)
    out = m.enhance_frame(low.to(dev), 4, noise=x_init[None].to(dev), return_intermediate=True, sampler="ddim")
    assert tuple(out.enhanced.shape) == (2, 3, 64, 96)
    worst = max(np.abs(out.intermediate[i].cpu().numpy().astype(np.float64) - r).max() / np.abs(r).max()
                for i, r in enumerate(ref["intermediate"]))
    print(f"frame 64 x 96: worst max-abs / max|ref| over the steps {worst:.3e} (bar {LOOP_BAR:.1e})")
    assert worst <= LOOP_BAR
    img = torch.from_numpy((np.random.default_rng(5).random((70, 90, 3)) * 90).astype(np.uint8)).to(dev)
    canvas = torch.randn(1, 3, 72, 96, generator=torch.Generator().manual_seed(6))
    u8 = M.enhance_frame_u8(m, img, 5, noise=canvas, sampler="ddim")
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (70, 90, 3)
    assert torch.equal(u8, M.enhance_frame_u8(m, img, 5, noise=canvas, sampler="ddim"))


# ------------------------------------------------------------------ 6. tiles
def test_tile_sync_step_bit_exact(dev):
    h, w, s, v = 96, 80, 64, 8
    rng = np.random.default_rng(31)
    eps = rng.uniform(-4, 4, (4, 3, s, s)).astype(F)
    x = rng.standard_normal((3, h, w), dtype=F)
    eps_d, x_d = torch.from_numpy(eps).to(dev), torch.from_numpy(x).to(dev)
    for vpred in (0, 1):
        for last in (0, 1):
            c = native.StepCoef(0.8, 0.6, 0.9, 0.43, last, vpred, 0, 1)
            want = T.sync_step_array(eps, (h, w), v, x, None, c)
            got = M.sync_step_device(eps_d, (h, w), v, x_d, None, c)  # no noise on any step
            assert np.array_equal(got.cpu().numpy(), want), (vpred, last)
            inplace = x_d.clone()
            img = torch.zeros(h, w, 3, dtype=torch.uint8, device=dev)
            M.sync_step_device(eps_d, (h, w), v, inplace, None, c, out=inplace, image=img)
            assert np.array_equal(inplace.cpu().numpy(), want)
            assert np.array_equal(img.cpu().numpy(), T.canvas_store_array(want, (h, w)))
    with pytest.raises(ValueError):
        M.sync_step_device(eps_d, (h, w), v, x_d, None, native.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 1, 1))


@pytest.mark.parametrize("sync", ["none", "latents"])
def test_enhance_tiled(dev, sync):
    m = small64(dev)[0]
    h, w, v = 96, 80, 8
    img_np = (np.random.default_rng(32).random((h, w, 3)) * 90).astype(np.uint8)
    img = torch.from_numpy(img_np).to(dev)
    canvas = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(33))
    a = M.enhance_tiled(m, img, 4, overlap=v, tile_batch=3, noise=canvas, sync=sync, sampler="ddim")
    assert a.dtype == torch.uint8 and tuple(a.shape) == (h, w, 3) and float(a.float().std()) > 0
    assert torch.equal(a, M.enhance_tiled(m, img, 4, overlap=v, tile_batch=3, noise=canvas, sync=sync, sampler="ddim"))
    for seed in (1, 2):  # a generator seeds the canvas, which is all the noise there is
        torch.manual_seed(seed)
        b = M.enhance_tiled(m, img, 4, overlap=v, generator=torch.Generator(device=dev).manual_seed(9), sync=sync, sampler="ddim")
        first = b if seed == 1 else first
    assert torch.equal(b, first)
    with pytest.raises(ValueError):
        M.enhance_tiled(m, img, 4, overlap=v, noise=torch.randn(4, 3, h, w), sync=sync, sampler="ddim")  # the LCM loop's canvas
    if sync == "latents":  # the device loop is the host mirror on the engine's own denoiser, bit for bit
        ts, coefs = m.ddim_schedule(4)

        def eps_fn(lat, low, t):
            tt = torch.full((lat.shape[0],), t, dtype=torch.long, device=dev)
            return m.unet.forward_split(torch.from_numpy(lat).to(dev), torch.from_numpy(low).to(dev), tt, uniform_t=True).cpu().numpy()

        want, want_x = T.enhance_tiled_sync_array(eps_fn, img_np, 64, v, coefs, ts, canvas.numpy(), sampler="ddim")
        got, x = M.enhance_tiled(m, img, 4, overlap=v, noise=canvas, sync=sync, return_canvas=True, sampler="ddim")
        assert np.array_equal(x.cpu().numpy(), want_x) and np.array_equal(got.cpu().numpy(), want) and torch.equal(got, a)
    else:  # the composition of the parts: gather, `enhance(sampler="ddim")` per tile, blend
        low = T.gather_tiles_array(img_np, 64, v)
        draws = torch.stack([canvas[:, :, oy:oy + 64, ox:ox + 64] for oy in T.tile_origins(h, 64, v) for ox in T.tile_origins(w, 64, v)], dim=1)
        tiles = m.enhance(torch.from_numpy(low).to(dev), 4, noise=draws.to(dev), sampler="ddim").cpu().numpy()
        assert np.array_equal(a.cpu().numpy(), T.blend_tiles_array(tiles, (h, w), v))


# ------------------------------------------------------------------ 7. evaluation and the trainer
def pair_store(dev, n=2):
    rng = np.random.default_rng(41)
    high = [rng.integers(0, 256, size=(72, 80, 3), dtype=np.uint8) for _ in range(n)]
    return M.DeviceFrameStore([f // 5 for f in high], high, device=dev, names=[f"p{i}.png" for i in range(n)])


def test_evaluate(dev):
    m = small64(dev)[0]
    store = pair_store(dev)
    loader = M.DevicePairLoader(store, 2, 64, "val")
    torch.manual_seed(1)
    a = M.evaluate(m, loader, sampler="ddim", num_inference_steps=10)
    torch.manual_seed(2)
    b = M.evaluate(m, loader, sampler="ddim", num_inference_steps=10)
    assert a["n"] == 2 and np.isfinite([a["psnr"], a["ssim"], a["mse"], a["loss"]]).all()
    assert a == b
    assert a["psnr"] != M.evaluate(m, loader, num_inference_steps=4)["psnr"]
    # the recipe of the docstring: one entry of noise per batch
    g = torch.Generator(device=dev).manual_seed(0)
    batch = next(iter(loader))
    noise = torch.randn(1, 2, 3, 64, 64, generator=g, device=dev)
    want = M.image_metrics(m.enhance(batch["low_light"], 10, noise=noise, sampler="ddim"), batch["normal_light"], data_range=(-1.0, 1.0))
    assert abs(a["per_image"]["psnr"][0] - float(want.psnr[0])) <= 1e-9
    for mode, kw in (("tiled", {"overlap": 8}), ("tiled", {"overlap": 8, "sync": "latents"}), ("frame", {})):
        r1 = M.evaluate_full_resolution(m, store, num_inference_steps=5, mode=mode, sampler="ddim", **kw)
        r2 = M.evaluate_full_resolution(m, store, num_inference_steps=5, mode=mode, sampler="ddim", **kw)
        assert r1 == r2 and np.isfinite([r1["psnr"], r1["ssim"]]).all()


def test_trainer_validation(dev, tmp_path):
    torch.manual_seed(0)
    model = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4).to(dev)
    store = pair_store(dev, 4)
    cfg = M.TrainingConfig(image_size=64, batch_size=2, epochs=1, use_amp=False, use_ema=False, scheduler_type="cosine", warmup_epochs=0, log_interval=0, save_interval=100,
                           sample_interval=100, seed=3, progress=False, output_dir=str(tmp_path / "out"),
                           checkpoint_dir=str(tmp_path / "ckpt"))
    trainer = M.LowLightTrainer(model, M.DevicePairLoader(store, 2, 64, "train", 3), M.DevicePairLoader(store, 2, 64, "val", 3), cfg,
                                val_sampler="ddim", val_steps=10)
    torch.manual_seed(1)
    loss = trainer.validate()
    first = dict(trainer.last_validation)
    torch.manual_seed(2)
    assert trainer.validate() == loss and trainer.last_validation == first
    assert first == M.evaluate(model, trainer.val_loader, num_inference_steps=10, seed=3, sampler="ddim")
    assert np.isfinite([first["psnr"], first["ssim"]]).all()
    sheet = trainer.generate_samples(0)
    assert sheet.exists()
    once = sheet.read_bytes()
    assert trainer.generate_samples(0).read_bytes() == once
