"""GPU tests of gradient accumulation: llie_grad_accumulate, TrainStep / DistillStep windows
(accumulate / apply / discard) and LowLightTrainer(accumulate=k).  The model is `small` at image_size = 64 throughout.

  1  the kernel equals its NumPy twin bit for bit: every n at which it takes another path, both alignments, guard words
  2  a window is its written-out composition (train forward, loss, backward, twin-accumulate on the host, step_flat), bit for bit
  3  acc / sum b against float64-checked CPU autograd, at the bars a single step is held to
  4  the grad scaler: a window with a non-finite micro-batch is skipped; a clean fp16 window is its composition
  5  the state machine and what is refused; a window makes no host read
  6  DistillStep windows
  7  the trainer: accumulate=2 over 3 batches is the written-out loop; resume; accumulate=1 is the trainer without the keyword
"""
import importlib

import numpy as np
import pytest
import torch

from test_gpu_train_rect import (KINK_MARGIN_2BYTE, _assert_same_state, _config, _frames, _inputs, _model, _new_model,
                                 _oracle_step, _pair, _reference, _state_of, _weights, cosine)
from test_gpu_distill import _distill
from test_gpu_distill import _inputs as _distill_inputs

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")
T = importlib.import_module("cv-diffusion-model_amd.training")
P = importlib.import_module("cv-diffusion-model_amd.pipeline")
U = importlib.import_module("cv-diffusion-model_amd.unet")

CHUNK = 4096  # kOptChunk (csrc/kernels.h): elements per workgroup, 256 threads of four floats, four passes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1: the kernel
def _launch(acc, grad, weight, first, dev):
    with torch.cuda.device(dev):
        N.check(N.lib().llie_grad_accumulate(acc.data_ptr(), grad.data_ptr(), acc.numel(), float(weight), int(first),
                                             torch.cuda.current_stream(dev).cuda_stream), "grad_accumulate")


def _same_as_twin(got, want):
    """Bit-equal where the twin is a number; NaN exactly where the twin is NaN (a NaN's sign and payload are the machine's)."""
    got = got.cpu().numpy()
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


GUARD = 4  # floats on either side of acc; 4 keeps acc 16-byte aligned at offset 0
SIZES = [1, 3, 4, 5, 1023, 4097,
         2 * CHUNK + 1024 + 7]  # past two full workgroups: a third block, a second pass of its four-float loop, a scalar tail


@pytest.mark.parametrize("acc_off,grad_off", [(0, 0), (1, 1), (0, 1), (1, 0)])
def test_kernel_equals_the_twin_bit_for_bit(dev, acc_off, grad_off):
    """first = 1 over a NaN-poisoned accumulator, then first = 0 on top of it, for every n and weight; pointers offset by one
    float take the single-element path; the guard words on both sides of acc keep their bits."""
    rng = np.random.default_rng(acc_off * 2 + grad_off)
    sentinel = np.float32(-12345.678)
    for n in SIZES:
        g1, g2 = (rng.standard_normal(n).astype(np.float32) * np.float32(3) for _ in range(2))
        for weight in (1, 2, 3, 5):
            buf = torch.full((GUARD + acc_off + n + GUARD,), float(sentinel), device=dev)
            acc = buf[GUARD + acc_off:GUARD + acc_off + n]
            acc.fill_(float("nan"))
            assert acc.data_ptr() % 16 == 4 * acc_off
            grads = []
            for g in (g1, g2):
                t = torch.empty(grad_off + n, device=dev)[grad_off:]
                t.copy_(torch.from_numpy(g))
                assert t.data_ptr() % 16 == 4 * grad_off
                grads.append(t)
            _launch(acc, grads[0], weight, 1, dev)
            want = T.grad_accumulate_array(None, g1, weight, True)
            assert np.isfinite(want).all() and _same_as_twin(acc, want), (n, weight, "first")
            _launch(acc, grads[1], weight + 1, 0, dev)
            want = T.grad_accumulate_array(want, g2, weight + 1, False)
            assert _same_as_twin(acc, want), (n, weight, "second")
            lo, hi = buf[:GUARD + acc_off].cpu().numpy(), buf[GUARD + acc_off + n:].cpu().numpy()
            assert (lo.view(np.uint32) == sentinel.view(np.uint32)).all() and (hi.view(np.uint32) == sentinel.view(np.uint32)).all(), (n, weight)
            assert torch.equal(_bits(grads[1]), _bits(torch.from_numpy(g2).to(dev)))  # grad is read only


@pytest.mark.parametrize("off", [0, 1])
def test_kernel_propagates_inf_and_nan(dev, off):
    """An inf in grad gives inf; an inf followed by -inf gives NaN; the elements around them are untouched by it."""
    n = CHUNK + 9
    g = np.ones(n, dtype=np.float32)
    g[[0, 5, n - 1]] = [np.inf, -np.inf, np.inf]
    grad = torch.empty(off + n, device=dev)[off:]
    acc = torch.full((off + n,), float("nan"), device=dev)[off:]
    grad.copy_(torch.from_numpy(g))
    _launch(acc, grad, 2.0, 1, dev)
    want = T.grad_accumulate_array(None, g, 2.0, True)
    assert _same_as_twin(acc, want)
    assert acc[0].item() == float("inf") and acc[5].item() == -float("inf") and acc[1].item() == 2.0
    grad.copy_(torch.from_numpy(-g))
    _launch(acc, grad, 3.0, 0, dev)
    want = T.grad_accumulate_array(want, -g, 3.0, False)
    assert _same_as_twin(acc, want)
    got = acc.cpu().numpy()
    assert np.isnan(got[[0, 5, n - 1]]).all() and np.isfinite(np.delete(got, [0, 5, n - 1])).all() and got[1] == -1.0


def test_kernel_past_two_gib(dev):
    """Byte offsets past 2^31 (n = 2^29 + one workgroup + 5): the head and the tail against the twin, the whole range
    against torch's separately rounded `acc + weight * grad`."""
    n = 2 ** 29 + CHUNK + 5
    gen = torch.Generator(device=dev).manual_seed(1)
    grad = torch.randn(n, generator=gen, device=dev)
    acc = torch.full((n,), float("nan"), device=dev)
    _launch(acc, grad, 3.0, 1, dev)
    assert torch.equal(_bits(acc), _bits(grad * 3.0))
    before = acc.clone()
    _launch(acc, grad, 5.0, 0, dev)
    for sl in (slice(0, 70), slice(n - 4200, n)):
        want = T.grad_accumulate_array(before[sl].cpu().numpy(), grad[sl].cpu().numpy(), 5.0, False)
        assert _same_as_twin(acc[sl], want)
    prod = grad * 5.0
    prod += before
    assert torch.equal(_bits(acc), _bits(prod))


# ------------------------------------------------------------------ 2: a window is its written-out composition
def _to(dev, batch):
    return tuple(v.to(dev) for v in batch)


def _offsets(model, opt):
    unet = model.unet
    h = unet._handle(U.resolve_compute_dtype(unet.compute_dtype))
    offs = h.grad_offsets()
    return h, [offs[i] for i in T._engine_order(unet, opt, "test")]


def _hand_micro(model, h, batch, dev, x0=(0.0, 0.0), scale=None):
    """One micro-batch by hand: llie_unet_train_forward_hw -> base_loss_and_grad (-> the x0 term, -> times the loss scale) ->
    llie_unet_backward; returns (loss, the flat gradient buffer copied back)."""
    low, normal, noise, t = batch
    b, _, hh, ww = low.shape
    L = N.lib()
    nbytes = h.train_workspace_bytes(b, hh, ww)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    flat = torch.empty(h.grad_numel(), dtype=torch.float32, device=dev)
    noisy = model.scheduler.add_noise(normal, noise, t).float().contiguous()
    cond, t = low.float().contiguous(), t.to(dtype=torch.long).contiguous()
    eps = torch.empty(b, 3, hh, ww, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), torch.no_grad():
        st = torch.cuda.current_stream(dev).cuda_stream
        N.check(L.llie_unet_train_forward_hw(h.h, noisy.data_ptr(), cond.data_ptr(), t.data_ptr(), eps.data_ptr(), b, hh, ww,
                                             ws.data_ptr(), nbytes, st), "train_forward_hw")
        loss, d_eps = P.base_loss_and_grad(eps, noise, "mse")
        if x0 != (0.0, 0.0):
            d_eps = d_eps.contiguous()
            loss = loss + P.x0_loss_device(model.scheduler, eps, noisy, normal, t, False, x0[0], x0[1], d_eps)
        if scale is not None:
            d_eps = d_eps * scale
        N.check(L.llie_unet_backward(h.h, d_eps.data_ptr(), flat.data_ptr(), b, ws.data_ptr(), nbytes, st), "backward")
    return loss, flat.cpu().numpy()


def _written_out_window(model, opt, micro, dev, x0=(0.0, 0.0), scaler=None):
    """The definition: acc = sum b_i g_i with the host twin, one step_flat(acc, offsets, 1 / sum b); the window loss in the
    documented order of fp32 operations."""
    h, offsets = _offsets(model, opt)
    acc, num, total = None, None, 0
    for batch in micro:
        b = batch[0].shape[0]
        loss, flat = _hand_micro(model, h, batch, dev, x0, None if scaler is None else scaler._device_scale(dev))
        acc = T.grad_accumulate_array(acc, flat, float(b), acc is None)
        term = loss * float(b)
        num = term if num is None else num + term
        total += b
    opt.step_flat(torch.from_numpy(acc).to(dev), offsets, grad_scale=1.0 / total, grad_scaler=scaler)
    return num / float(total)


def _assert_same_run(a, opt_a, b, opt_b, what):
    bad = [k for (k, x), y in zip(a.named_parameters(), b.parameters()) if not torch.equal(x, y)]
    assert not bad, f"{what}: {len(bad)} parameters differ, e.g. {bad[:4]}"
    assert torch.equal(opt_a._m, opt_b._m) and torch.equal(opt_a._v, opt_b._v), f"{what}: moments"
    assert torch.equal(opt_a._ema, opt_b._ema), f"{what}: EMA shadows"
    assert torch.equal(_bits(opt_a.grad_norm()), _bits(opt_b.grad_norm())), (what, opt_a.grad_norm().item(), opt_b.grad_norm().item())


def _clones(dev, cd):
    """Two equal models (seeded random weights) at compute dtype `cd`, a FusedAdamW each with clipping and EMA on."""
    a, b, opt_a, opt_b = _pair(dev)
    a.compute_dtype = b.compute_dtype = cd
    return a, b, opt_a, opt_b


WINDOWS = {
    "fp32-1+3": (None, [(64, 64, 1), (64, 64, 3)], (0.0, 0.0)),
    "bf16-mixed": ("bf16", [(64, 64, 2), (64, 96, 1)], (0.0, 0.0)),
    "fp32-x0": (None, [(64, 64, 1), (64, 64, 3)], (0.5, 0.25)),
}


@pytest.mark.parametrize("case", list(WINDOWS))
def test_window_is_its_written_out_composition(dev, case):
    """accumulate x k, apply on one clone; on the other each micro-batch by hand, the twin on the host, one step_flat:
    parameters, both moments, EMA shadows, grad_norm() and the window loss are equal bit for bit."""
    cd, shapes, x0 = WINDOWS[case]
    a, b, opt_a, opt_b = _clones(dev, cd)
    start = [p.detach().clone() for p in a.parameters()]
    micro = [_to(dev, _inputs(hh, ww, n, seed=31 + i)) for i, (hh, ww, n) in enumerate(shapes)]
    step = M.TrainStep(a, opt_a, x0_ssim_weight=x0[0], x0_l1_weight=x0[1])
    assert step.window_images == 0
    seen = 0
    for low, normal, noise, t in micro:
        loss_i = step.accumulate(low, normal, timesteps=t, noise=noise)
        seen += low.shape[0]
        assert step.window_images == seen and loss_i.dim() == 0 and loss_i.device == low.device
    loss_a = step.apply()
    assert step.window_images == 0
    loss_b = _written_out_window(b, opt_b, micro, dev, x0)
    print(f"{case}: window loss {loss_a.item():.7f}, gradient norm {opt_a.grad_norm().item():.6f}")
    assert torch.isfinite(loss_a) and torch.equal(_bits(loss_a), _bits(loss_b)), (loss_a.item(), loss_b.item())
    _assert_same_run(a, opt_a, b, opt_b, case)
    assert any(not torch.equal(p, q) for p, q in zip(a.parameters(), start))  # the step moved the parameters


@pytest.mark.parametrize("cd", [None, "bf16"])
def test_a_window_of_one_power_of_two_batch_is_the_plain_step(dev, cd):
    """b = 2: acc = 2 g and grad_scale = 1 / 2 are exact, so accumulate + apply gives the bits of __call__."""
    a, b, opt_a, opt_b = _clones(dev, cd)
    low, normal, noise, t = _to(dev, _inputs(64, 96, 2, seed=5))
    wa, wb = M.TrainStep(a, opt_a), M.TrainStep(b, opt_b)
    la_micro = wa.accumulate(low, normal, timesteps=t, noise=noise)
    la = wa.apply()
    lb = wb(low, normal, timesteps=t, noise=noise)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(la_micro), _bits(lb))
    _assert_same_run(a, opt_a, b, opt_b, "window of one b = 2")
    # after an applied window a plain step gives the bits of the clone that never opened one
    low, normal, noise, t = _to(dev, _inputs(64, 64, 3, seed=6))
    assert torch.equal(_bits(wa(low, normal, timesteps=t, noise=noise)), _bits(wb(low, normal, timesteps=t, noise=noise)))
    _assert_same_run(a, opt_a, b, opt_b, "plain step after a window")


# ------------------------------------------------------------------ 3: against CPU autograd
FIRST_2BYTE = {(64, 64, 2): 4, (64, 96, 1): 14, (64, 64, 4): 0}  # first attempt that keeps KINK_MARGIN_2BYTE (oracle alone)
_REFS = {}


def _truth(hh, ww, batch, two_byte):
    """(inputs, gradients of the batch's mean loss) from CPU autograd over the oracle, at inputs that keep the SE squeezes off
    the ReLU6 kinks: test_gpu_train_rect._reference and its rule, with the first passing attempt of these shapes."""
    if not two_byte:
        inputs, _, _, grads = _reference("small", hh, ww, batch)
        return inputs, grads
    key = (hh, ww, batch)
    if key not in _REFS:
        sd, spec = _weights("small")
        first = FIRST_2BYTE[key]
        for attempt in range(first, first + 16):
            inputs = _inputs(hh, ww, batch, seed=hh * 7 + ww + batch + 1000 * attempt)
            _, _, grads, (_, margin_small) = _oracle_step(sd, spec, *inputs)
            if margin_small >= KINK_MARGIN_2BYTE:
                break
        assert margin_small >= KINK_MARGIN_2BYTE, margin_small
        _REFS[key] = (inputs, grads)
    return _REFS[key]


def _window_gradients(dev, cd, micro):
    """accumulate every micro-batch (lr = 0: the weights stay), read acc / sum b per parameter, discard."""
    m = _model("small", dev, cd)
    step = M.TrainStep(m, M.FusedAdamW(m.parameters(), lr=0.0, weight_decay=0.0))
    for low, normal, noise, t in micro:
        step.accumulate(*_to(dev, (low, normal)), timesteps=t.to(dev), noise=noise.to(dev))
    total = step.window_images
    got = {k: (step._acc[off:off + p.numel()].view_as(p) / total).cpu() for (k, p), off in zip(m.named_parameters(), step._offsets)}
    step.discard()
    return m, step, got


def _judge(got, want, two_byte, what):
    bad, worst_l2, worst_cs = {}, 0.0, 1.0
    for k, ref in want.items():
        a, b = got[k].double(), ref.double()
        assert torch.isfinite(a).all(), k
        l2, cs = ((a - b).norm() / b.norm().clamp_min(1e-30)).item(), cosine(a, b)
        worst_l2, worst_cs = max(worst_l2, l2), min(worst_cs, cs)
        if not (cs >= 0.98 if two_byte else (l2 < 2e-2 and cs > 0.9995)):
            bad[k] = (l2, cs)
    print(f"{what}: worst relative L2 {worst_l2:.3e}, worst cosine {worst_cs:.6f}")
    assert not bad, f"{what}: {len(bad)} tensors off: {dict(list(bad.items())[:8])}"


@pytest.mark.parametrize("cd,split", [(None, (1, 3)), (None, (2, 2)), ("bf16", (2, 2))])
def test_equal_shape_window_against_autograd_of_the_concatenated_batch(dev, cd, split):
    """acc / 4 of a window over the rows of a batch of 4 at 64 x 64 against CPU autograd on the whole batch: fp32 relative
    L2 < 2e-2 and cosine > 0.9995, bf16 cosine >= 0.98 (the bars of test_unet_backward_rect_vs_autograd / _half_engines).
    fp32 also prints the worst relative L2 against the engine's one-shot gradient of the concatenated batch: the reassociation
    of fp32 sums and nothing else (no bar of its own)."""
    inputs, want = _truth(64, 64, 4, cd is not None)
    cuts = [0, split[0], 4]
    micro = [tuple(v[lo:hi] for v in inputs) for lo, hi in zip(cuts, cuts[1:])]
    m, step, got = _window_gradients(dev, cd, micro)
    _judge(got, want, cd is not None, f"{cd or 'fp32'} {split[0]}+{split[1]} at 64x64")
    if cd is None:
        low, normal, noise, t = _to(dev, inputs)
        step(low, normal, timesteps=t, noise=noise)
        worst = 0.0
        for (k, p), off in zip(m.named_parameters(), step._offsets):
            one = step._flat[off:off + p.numel()].double().cpu()
            worst = max(worst, ((got[k].double().flatten() - one).norm() / one.norm().clamp_min(1e-30)).item())
        print(f"fp32 {split[0]}+{split[1]}: worst relative L2 of acc / 4 against the one-shot gradient of the batch of 4: {worst:.3e}")


@pytest.mark.parametrize("cd", [None, "bf16"])
def test_mixed_window_against_the_weighted_mean_of_autograd_gradients(dev, cd):
    """2 images at 64 x 64 plus 1 at 64 x 96: acc / 3 against the b-weighted float64 mean of the per-micro-batch CPU autograd
    gradients, at the same bars."""
    parts = [_truth(64, 64, 2, cd is not None), _truth(64, 96, 1, cd is not None)]
    weights = [2, 1]
    want = {k: sum(w * g[k].double() for w, (_, g) in zip(weights, parts)) / 3.0 for k in parts[0][1]}
    _, _, got = _window_gradients(dev, cd, [inputs for inputs, _ in parts])
    _judge(got, want, cd is not None, f"{cd or 'fp32'} 2 at 64x64 + 1 at 64x96")


# ------------------------------------------------------------------ 4: the grad scaler (fp16)
SCALE = 2.0 ** 10  # what the fp16 tests of a single step run under


def test_fp16_window_with_a_bad_micro_batch_is_skipped(dev):
    """An inf in the second micro-batch's noise: acc is non-finite, apply skips (parameters and moments unchanged, the scale
    halved, last_step_skipped()); the next clean window steps."""
    a, _, opt, _ = _clones(dev, "fp16")
    scaler = M.FusedGradScaler(init_scale=SCALE)
    step = M.TrainStep(a, opt, grad_scaler=scaler)
    clean = [_to(dev, _inputs(64, 64, 2, seed=41)), _to(dev, _inputs(64, 64, 1, seed=42))]
    low, normal, noise, t = clean[1]
    noise = noise.clone()
    noise[0, 1, 7, 9] = float("inf")
    before = ([p.detach().clone() for p in a.parameters()], opt._m.clone(), opt._v.clone())
    step.accumulate(clean[0][0], clean[0][1], timesteps=clean[0][3], noise=clean[0][2])
    assert torch.isfinite(step._acc).all()
    step.accumulate(low, normal, timesteps=t, noise=noise)
    assert not torch.isfinite(step._acc).all()
    step.apply()
    assert opt.last_step_skipped() and scaler.get_scale() == SCALE / 2
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), before[0]))
    assert torch.equal(opt._m, before[1]) and torch.equal(opt._v, before[2])
    for low, normal, noise, t in clean:
        step.accumulate(low, normal, timesteps=t, noise=noise)
    loss = step.apply()
    assert not opt.last_step_skipped() and torch.isfinite(loss) and scaler.get_scale() == SCALE / 2
    assert any(not torch.equal(p, q) for p, q in zip(a.parameters(), before[0]))
    assert opt.state_dict()["state"][0]["step"].item() == 1


def test_clean_fp16_window_is_its_written_out_composition(dev):
    a, b, opt_a, opt_b = _clones(dev, "fp16")
    sc_a, sc_b = M.FusedGradScaler(init_scale=SCALE), M.FusedGradScaler(init_scale=SCALE)
    micro = [_to(dev, _inputs(64, 64, 2, seed=51)), _to(dev, _inputs(64, 96, 1, seed=52))]
    start = [p.detach().clone() for p in a.parameters()]
    step = M.TrainStep(a, opt_a, grad_scaler=sc_a)
    for low, normal, noise, t in micro:
        step.accumulate(low, normal, timesteps=t, noise=noise)
    loss_a = step.apply()
    loss_b = _written_out_window(b, opt_b, micro, dev, scaler=sc_b)
    assert not opt_a.last_step_skipped() and not opt_b.last_step_skipped()
    assert torch.isfinite(loss_a) and torch.equal(_bits(loss_a), _bits(loss_b))
    _assert_same_run(a, opt_a, b, opt_b, "fp16 window")
    assert sc_a.get_scale() == sc_b.get_scale() == SCALE and sc_a._get_growth_tracker() == sc_b._get_growth_tracker() == 1
    assert any(not torch.equal(p, q) for p, q in zip(a.parameters(), start))


# ------------------------------------------------------------------ 5: the state machine and what is refused
def test_state_machine_and_refusals(dev):
    a, b, opt_a, opt_b = _clones(dev, None)
    b1, b2, b3 = (_to(dev, _inputs(hh, ww, n, seed=60 + n)) for hh, ww, n in ((64, 64, 2), (64, 96, 1), (64, 64, 3)))

    def acc(step, batch):
        low, normal, noise, t = batch
        return step.accumulate(low, normal, timesteps=t, noise=noise)

    step = M.TrainStep(a, opt_a)
    with pytest.raises(RuntimeError, match="no micro-batch"):
        step.apply()
    step.discard()  # closing no window is not an error
    acc(step, b1)
    with pytest.raises(RuntimeError, match="window is open"):
        step(b1[0], b1[1], timesteps=b1[3], noise=b1[2])
    assert step.window_images == 2
    # discard, then a fresh window: the bits of a fresh step object (the stale accumulator is not read)
    step.discard()
    assert step.window_images == 0
    with pytest.raises(RuntimeError, match="no micro-batch"):
        step.apply()
    step._acc.fill_(float("nan"))
    acc(step, b2)
    # a refused shape raises before the accumulator is touched and leaves the open window as it was
    held = step._acc.clone()
    bad = torch.zeros(1, 3, 60, 96, device=dev)
    with pytest.raises(ValueError, match="multiples of 8 and at least 64"):
        step.accumulate(bad, bad)
    assert step.window_images == 1 and torch.equal(_bits(step._acc), _bits(held))
    acc(step, b3)
    la = step.apply()
    fresh = M.TrainStep(b, opt_b)
    acc(fresh, b2)
    acc(fresh, b3)
    lb = fresh.apply()
    assert torch.equal(_bits(la), _bits(lb))
    _assert_same_run(a, opt_a, b, opt_b, "discard, then a fresh window")
    # a discarded window leaves a plain step as on the clone that never opened one
    acc(step, b1)
    step.discard()
    la = step(b3[0], b3[1], timesteps=b3[3], noise=b3[2])
    lb = fresh(b3[0], b3[1], timesteps=b3[3], noise=b3[2])
    assert torch.equal(_bits(la), _bits(lb))
    _assert_same_run(a, opt_a, b, opt_b, "plain step after a discarded window")
    # cond_grad is out of scope inside windows
    with_dx = M.TrainStep(a, opt_a, cond_grad=True)
    with pytest.raises(ValueError, match="cond_grad"):
        acc(with_dx, b1)
    assert with_dx.window_images == 0


@pytest.mark.parametrize("cd", [None, "fp16"])
def test_a_window_does_not_synchronise(dev, cd):
    """After a first window (engine context, workspace, the accumulator, the optimiser's tables, the scaler's state) a whole
    window of two shapes enqueues and returns: no host read in accumulate, apply or discard, with a grad scaler too."""
    a, _, opt, _ = _clones(dev, cd)
    step = M.TrainStep(a, opt, grad_scaler=M.FusedGradScaler(init_scale=SCALE) if cd == "fp16" else None)
    micro = [_to(dev, _inputs(64, 64, 2, seed=71)), _to(dev, _inputs(64, 96, 1, seed=72))]

    def window(close):
        for low, normal, noise, t in micro:
            step.accumulate(low, normal, timesteps=t, noise=noise)
        return close()

    window(step.apply)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = window(step.apply)
        window(step.discard)
        assert step.window_images == 0
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(loss)


# ------------------------------------------------------------------ 6: DistillStep
def test_distill_window_is_its_written_out_composition(dev):
    """bf16, a window of 1 + 1: against consistency_distillation_loss -> backward per micro-batch (the autograd path DistillStep
    equals bit for bit), the twin on the host, one step_flat(acc, offsets, 1 / 2) and one update_ema."""
    low, normal = (x.to(dev) for x in _distill_inputs(64))
    a, b = _distill(dev, cd="bf16"), _distill(dev, cd="bf16")
    kw = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    opt_a, opt_b = M.FusedAdamW(a.student.parameters(), **kw), M.FusedAdamW(b.student.parameters(), **kw)
    gen = torch.Generator().manual_seed(17)
    noise = torch.randn(2, 3, 64, 64, generator=gen).to(dev)
    idx = torch.randint(0, 37, (2,), generator=gen)
    step = M.DistillStep(a, opt_a, ema_decay=0.95)
    with pytest.raises(RuntimeError, match="no micro-batch"):
        step.apply()
    losses = [step.accumulate(low[i:i + 1], normal[i:i + 1], noise=noise[i:i + 1], idx=idx[i:i + 1]) for i in range(2)]
    assert step.window_images == 2
    with pytest.raises(RuntimeError, match="window is open"):
        step(low, normal, noise=noise, idx=idx)
    loss_a = step.apply()

    unet = b.student.unet
    h = unet._handle(U.resolve_compute_dtype(unet.compute_dtype))
    offs = h.grad_offsets()
    offsets = [offs[i] for i in T._engine_order(unet, opt_b, "test")]
    acc, num = None, None
    for i in range(2):
        b.student.zero_grad(set_to_none=True)
        lb = b.consistency_distillation_loss(low[i:i + 1], normal[i:i + 1], noise=noise[i:i + 1], idx=idx[i:i + 1])
        lb.backward()
        assert torch.equal(_bits(lb.detach()), _bits(losses[i])), i
        flat = np.zeros(h.grad_numel(), dtype=np.float32)
        for p, off in zip(b.student.parameters(), offsets):
            flat[off:off + p.numel()] = p.grad.detach().reshape(-1).cpu().numpy()
        acc = T.grad_accumulate_array(acc, flat, 1.0, acc is None)
        term = lb.detach() * 1.0
        num = term if num is None else num + term
    opt_b.step_flat(torch.from_numpy(acc).to(dev), offsets, grad_scale=1.0 / 2)
    b.update_ema(0.95)
    loss_b = num / 2.0
    assert torch.isfinite(loss_a) and torch.equal(_bits(loss_a), _bits(loss_b))
    for (k, pa), pb in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(pa, pb), k
    assert torch.equal(opt_a._m, opt_b._m) and torch.equal(opt_a._v, opt_b._v)
    assert torch.equal(_bits(opt_a.grad_norm()), _bits(opt_b.grad_norm()))
    fresh = _distill(dev, cd="bf16")
    assert any(not torch.equal(x, y) for x, y in zip(a.student.parameters(), fresh.student.parameters()))
    assert any(not torch.equal(x, y) for x, y in zip(a.ema_student.parameters(), fresh.ema_student.parameters()))


# ------------------------------------------------------------------ 7: the trainer
B, SEED = 2, 3


@pytest.fixture(scope="module")
def store(dev):
    return M.DeviceFrameStore(*_frames(6, 11), device=dev, names=[f"t{i}.png" for i in range(6)])


def _trainer(dev, store, cfg, **kw):
    return M.LowLightTrainer(_new_model(dev), M.DevicePairLoader(store, B, 64, "train", SEED), None, cfg, **kw)


def test_trainer_with_accumulate_is_the_written_out_loop_and_resumes(dev, store, tmp_path):
    """accumulate=2 over a loader of 3 batches, 2 epochs: windows 2 + 1 per epoch, 4 optimiser steps.  Equal, bit for bit in
    model, optimiser and EMA state, to the loop written out here (the draw recipe of train_epoch, accumulate / apply, a
    CosineAnnealingLR built for 2 steps per epoch); a resume from the epoch-0 checkpoint with the same keyword gives the
    uninterrupted run's bits."""
    from torch.optim.lr_scheduler import CosineAnnealingLR
    assert T.accumulation_windows(3, 2) == [2, 1]
    model = _new_model(dev)
    model.compute_dtype = "fp32"
    model.train()
    loader = M.DevicePairLoader(store, B, 64, "train", SEED)
    assert len(loader) == 3
    opt = M.FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9999)
    sched = CosineAnnealingLR(opt, T_max=2 * 2, eta_min=1e-6)
    step = M.TrainStep(model, opt, loss_type="mse")
    want_losses = []
    for epoch in range(2):
        loader.set_epoch(epoch)
        g = torch.Generator(device=dev).manual_seed((SEED * 1000003 + epoch * 8191 + 54321) % (2 ** 63 - 1))
        batches = iter(loader)
        losses = []
        for length in T.accumulation_windows(len(loader), 2):
            for _ in range(length):
                batch = next(batches)
                b = batch["low_light"].shape[0]
                t = torch.randint(0, 1000, (b,), generator=g, device=dev)
                noise = torch.randn(b, 3, 64, 64, generator=g, device=dev)
                losses.append(step.accumulate(batch["low_light"], batch["normal_light"], timesteps=t, noise=noise))
            step.apply()
            opt._opt_called = True
            sched.step()
        want_losses.append(sum(v.item() for v in losses) / 3)
    want = _state_of(model, opt)

    common = dict(epochs=2, save_interval=1, sample_interval=100)
    tr = _trainer(dev, store, _config(tmp_path / "a", **common), accumulate=2)
    history = tr.train()
    print("trainer", [h["train_loss"] for h in history], "written out", want_losses)
    assert [h["train_loss"] for h in history] == want_losses
    assert tr.global_step == 4 and tr.accumulate == 2 and tr.step.window_images == 0
    _assert_same_state(_state_of(tr.model, tr.optimizer), want, "trainer against the written-out loop")
    assert "accumulate" not in tr.checkpoint()["config"]

    resumed = _trainer(dev, store, _config(tmp_path / "b", resume_from=str(tmp_path / "a" / "ckpt" / "checkpoint_epoch_0.pt"), **common),
                       accumulate=2)
    assert resumed.epoch == 1 and resumed.global_step == 2
    (log,) = resumed.train()
    assert log["train_loss"] == want_losses[1] and resumed.global_step == 4
    _assert_same_state(_state_of(resumed.model, resumed.optimizer), want, "resumed against the uninterrupted run")


def test_trainer_accumulate_one_is_the_trainer_without_the_keyword(dev, store, tmp_path):
    common = dict(epochs=1, sample_interval=100)
    plain = _trainer(dev, store, _config(tmp_path / "a", **common))
    one = _trainer(dev, store, _config(tmp_path / "b", **common), accumulate=1)
    hp, ho = plain.train(), one.train()
    assert hp == ho and plain.global_step == one.global_step == 3
    _assert_same_state(_state_of(one.model, one.optimizer), _state_of(plain.model, plain.optimizer), "accumulate=1")
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="accumulate"):
            _trainer(dev, store, _config(tmp_path / "c", **common), accumulate=bad)
