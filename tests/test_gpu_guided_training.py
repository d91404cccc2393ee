"""Training with condition dropout on the MI355X: TrainStep(cond_dropout=p) against a plain TrainStep on a condition zeroed by
hand, the untouched default, the masked condition gradient, the autograd route, and one LowLightTrainer epoch against its draw
recipe written out.  small at image size 64, fp32 and bf16 engines; every comparison is on the bits, because the dropped-out
condition is the same tensor either way and the steps run the same kernels on it."""
import copy
import importlib

import numpy as np
import pytest
import torch

from conftest import synth_input

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
TR = importlib.import_module("cv-diffusion-model_amd.trainer")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def build(dev, cd, seed=3):
    torch.manual_seed(seed)
    return M.LowLightDiffusion(unet_variant="small", image_size=64, compute_dtype=cd).to(dev).train()


def batch(dev, b=3):
    low = synth_input("guided:tlow", (b, 3, 64, 64), -1.0, -0.2).to(dev)
    normal = synth_input("guided:tnormal", (b, 3, 64, 64), -1.0, 1.0).to(dev)
    g = torch.Generator().manual_seed(9)
    t = torch.randint(0, 1000, (b,), generator=g).to(dev)
    noise = torch.randn(b, 3, 64, 64, generator=g).to(dev)
    return low, normal, t, noise


def step_for(model, **kw):
    opt = M.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    return M.TrainStep(model, opt, loss_type="mse", **kw)


U = [0.7, 0.2, 0.5]  # at p = 0.5: kept, dropped, kept (u == p)


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_step_equals_a_plain_step_on_a_zeroed_condition(dev, cd):
    a = build(dev, cd)
    b = copy.deepcopy(a)
    low, normal, t, noise = batch(dev)
    u = torch.tensor(U, device=dev)
    step_a, step_b = step_for(a, cond_dropout=0.5), step_for(b)
    zeroed = low.clone()
    zeroed[1] = 0.0
    state = torch.cuda.get_rng_state(dev)
    la = step_a(low, normal, timesteps=t, noise=noise, cond_u=u)
    assert torch.equal(torch.cuda.get_rng_state(dev), state)  # everything was supplied: no draw
    lb = step_b(zeroed, normal, timesteps=t, noise=noise)
    assert torch.equal(la, lb), (la.item(), lb.item())
    assert torch.equal(step_a._flat, step_b._flat)
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    assert torch.equal(step_a._cond, zeroed) and float(low[1].abs().min()) > 0  # the caller's tensor is left alone
    # a window: the same micro-batches through accumulate / apply
    la2 = step_a.accumulate(low, normal, timesteps=t, noise=noise, cond_u=u)
    lb2 = step_b.accumulate(zeroed, normal, timesteps=t, noise=noise)
    assert torch.equal(la2, lb2) and torch.equal(step_a._flat, step_b._flat)
    assert torch.equal(step_a.apply(), step_b.apply())
    # p = 1 drops every row whatever u is; cond_u of another shape is refused
    step_c, step_d = step_for(copy.deepcopy(a), cond_dropout=1.0), step_for(copy.deepcopy(a))
    assert torch.equal(step_c(low, normal, timesteps=t, noise=noise, cond_u=u), step_d(torch.zeros_like(low), normal, timesteps=t, noise=noise))
    assert torch.equal(step_c._flat, step_d._flat)
    with pytest.raises(ValueError, match="cond_u"):
        step_a(low, normal, timesteps=t, noise=noise, cond_u=u[:2])
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="cond_dropout"):
            step_for(a, cond_dropout=bad)


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_the_uniforms_are_the_third_draw(dev, cd):
    """Without cond_u the step draws torch.rand(b) from the global device generator after timesteps and noise."""
    a = build(dev, cd)
    b = copy.deepcopy(a)
    low, normal, _, _ = batch(dev)
    step_a, step_b = step_for(a, cond_dropout=0.5), step_for(b, cond_dropout=0.5)
    torch.manual_seed(77)
    la = step_a(low, normal)
    after = torch.cuda.get_rng_state(dev)
    torch.manual_seed(77)
    t = torch.randint(0, 1000, (3,), device=dev)
    noise = torch.randn_like(normal)
    u = torch.rand(3, device=dev)
    assert torch.equal(torch.cuda.get_rng_state(dev), after)
    lb = step_b(low, normal, timesteps=t, noise=noise, cond_u=u)
    assert torch.equal(la, lb) and torch.equal(step_a._flat, step_b._flat)


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_zero_dropout_is_the_step_without_the_keyword(dev, cd):
    a = build(dev, cd)
    b = copy.deepcopy(a)
    low, normal, _, _ = batch(dev)
    step_a, step_b = step_for(a, cond_dropout=0.0), step_for(b)
    torch.manual_seed(5)
    la = step_a(low, normal)
    state_a = torch.cuda.get_rng_state(dev)
    torch.manual_seed(5)
    lb = step_b(low, normal)
    assert torch.equal(torch.cuda.get_rng_state(dev), state_a)  # no third draw at p == 0
    assert torch.equal(la, lb) and torch.equal(step_a._flat, step_b._flat)
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    assert step_a._cond is None  # the kernel did not run


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_condition_gradient_is_masked(dev, cd):
    a = build(dev, cd)
    b = copy.deepcopy(a)
    low, normal, t, noise = batch(dev)
    u = torch.tensor(U, device=dev)
    zeroed = low.clone()
    zeroed[1] = 0.0
    step_a, step_b = step_for(a, cond_dropout=0.5, cond_grad=True), step_for(b, cond_grad=True)
    la = step_a(low, normal, timesteps=t, noise=noise, cond_u=u)
    lb = step_b(zeroed, normal, timesteps=t, noise=noise)
    assert torch.equal(la, lb) and torch.equal(step_a._flat, step_b._flat)
    ga, gb = step_a.cond_grad, step_b.cond_grad
    assert ga.shape == low.shape
    assert np.array_equal(ga[1].cpu().numpy().view(np.uint32), np.zeros((3, 64, 64), dtype=np.uint32))  # dropped: exactly +0
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[2], gb[2])  # kept rows: the undropped step's
    assert float(gb[1].abs().max()) > 0 and float(ga[0].abs().max()) > 0  # the mask, not the network, made the zeros


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_autograd_route_gives_the_step_gradients(dev, cd):
    """compute_loss(..., cond_dropout=p) + backward() against TrainStep(cond_dropout=p), to the standard of
    test_train_step_matches_the_autograd_path: the same draws from the global generator, the same loss and parameter
    gradients, bit for bit; and the gradient of a low_light that requires one is masked."""
    a = build(dev, cd)
    b = copy.deepcopy(a)
    low, normal, _, _ = batch(dev)
    step_b = step_for(b, cond_dropout=0.5, cond_grad=True)
    low_a = low.clone().requires_grad_(True)
    torch.manual_seed(100)
    la = a.compute_loss(low_a, normal, loss_type="mse", cond_dropout=0.5)
    la.backward()
    state = torch.cuda.get_rng_state(dev)
    torch.manual_seed(100)
    lb = step_b(low, normal)
    assert torch.equal(torch.cuda.get_rng_state(dev), state)
    assert torch.equal(la.detach(), lb), (la.item(), lb.item())
    for p, off, q in zip(a.parameters(), step_b._offsets, b.parameters()):
        assert torch.equal(step_b._flat[off:off + q.numel()].view_as(q), p.grad)
    assert torch.equal(low_a.grad, step_b.cond_grad)
    torch.manual_seed(100)
    torch.randint(0, 1000, (3,), device=dev), torch.randn_like(normal)
    dropped = torch.rand(3, device=dev) < 0.5
    for i in range(3):
        assert bool((low_a.grad[i] == 0).all()) == bool(dropped[i])
    # forward with supplied uniforms: the dict is forward's, the prediction is the one on the zeroed condition
    t = torch.tensor([10, 500, 900], device=dev)
    noise = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        got = a.forward(low, normal, timesteps=t, noise=noise, cond_dropout=0.5, cond_u=torch.tensor(U, device=dev))["noise_pred"]
        zeroed = low.clone()
        zeroed[1] = 0.0
        assert torch.equal(got, a.forward(zeroed, normal, timesteps=t, noise=noise)["noise_pred"])
        assert torch.equal(a.forward(low, normal, timesteps=t, noise=noise, cond_dropout=0.0)["noise_pred"],
                           a.forward(low, normal, timesteps=t, noise=noise)["noise_pred"])


def pair_store(dev, n=4):
    rng = np.random.default_rng(41)
    high = [rng.integers(0, 256, size=(72, 80, 3), dtype=np.uint8) for _ in range(n)]
    return M.DeviceFrameStore([f // 5 for f in high], high, device=dev, names=[f"p{i}.png" for i in range(n)])


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_trainer_epoch_follows_its_draw_recipe(dev, cd, tmp_path):
    """One LowLightTrainer epoch of two batches with cond_dropout=0.5 against the recipe of train_epoch's docstring written out
    over a second trainer without dropout whose batches are zeroed by hand."""
    store = pair_store(dev)

    def trainer(p, tag):
        torch.manual_seed(0)
        model = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4).to(dev)
        cfg = M.TrainingConfig(image_size=64, batch_size=2, epochs=1, use_amp=False, use_ema=False, scheduler_type="cosine",
                               warmup_epochs=0, log_interval=0, save_interval=100, sample_interval=100, seed=3, progress=False,
                               compute_dtype=cd, output_dir=str(tmp_path / f"out{tag}"), checkpoint_dir=str(tmp_path / f"ckpt{tag}"))
        return M.LowLightTrainer(model, M.DevicePairLoader(store, 2, 64, "train", 3), None, cfg, **p)

    ta, tb = trainer({"cond_dropout": 0.5}, "a"), trainer({}, "b")
    assert ta.step.cond_dropout == 0.5 and tb.step.cond_dropout == 0.0
    state = torch.cuda.get_rng_state(dev)
    mean_a = ta.train_epoch()
    assert torch.equal(torch.cuda.get_rng_state(dev), state)  # the global generator is neither read nor advanced
    tb.model.train()
    tb.train_loader.set_epoch(0)
    g = torch.Generator(device=dev).manual_seed(TR.train_draw_seed(3, 0))
    losses, dropped = [], 0
    for b in tb.train_loader:
        low, normal = b["low_light"], b["normal_light"]
        n = low.shape[0]
        t = torch.randint(0, 1000, (n,), generator=g, device=dev)
        noise = torch.randn(n, 3, 64, 64, generator=g, device=dev)
        u = torch.rand(n, generator=g, device=dev)
        low = low.clone()
        low[u < 0.5] = 0.0
        dropped += int((u < 0.5).sum())
        losses.append(tb.step(low, normal, timesteps=t, noise=noise))
        tb.optimizer._opt_called = True
        tb.scheduler.step()
    assert len(losses) == 2
    assert mean_a == sum(float(v) for v in torch.stack(losses).cpu().tolist()) / 2
    for x, y in zip(ta.model.parameters(), tb.model.parameters()):
        assert torch.equal(x, y)
    print(f"{cd}: {dropped} of 4 conditions dropped")
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="cond_dropout"):
            trainer({"cond_dropout": bad}, "c")
    with pytest.raises(ValueError, match="guidance_scale"):
        trainer({"val_guidance_scale": float("inf")}, "d")
