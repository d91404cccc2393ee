"""LowLightDistiller and scripts/distill.py on the MI355X.

The setup of tests/test_gpu_trainer.py: small@64, B = 2, 6 training and 4 validation pairs of seeded random 72 x 80 frames
(3 batches per epoch), 2 epochs; the teacher is built after torch.manual_seed(1), the student after torch.manual_seed(0).  Both
are v-prediction networks unless said, so the draws include the terminal idx.

Every comparison is exact: DistillStep promises bitwise-reproducible gradients, so a distiller run equals the loop written out
here, and a resumed run the straight one, bit for bit."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR

from conftest import ROOT

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
D = importlib.import_module("cv-diffusion-model_amd.distiller")

S, B, SEED = 64, 2, 3
STEPS_PER_EPOCH = 3
V = "v_prediction"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def frames(n, seed, hw=(72, 80)):
    rng = np.random.default_rng(seed)
    high = [rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) for _ in range(n)]
    return [f // 5 for f in high], high


@pytest.fixture(scope="module")
def stores(dev):
    return (M.DeviceFrameStore(*frames(6, 11), device=dev, names=[f"t{i}.png" for i in range(6)]),
            M.DeviceFrameStore(*frames(4, 12), device=dev, names=[f"v{i}.png" for i in range(4)]))


def scheduler(ptype):
    return M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type=ptype, num_inference_steps=4,
                          rescale_betas_zero_snr=True)


def network(seed, ptype=V):
    torch.manual_seed(seed)
    return M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4, scheduler=scheduler(ptype))


def new_distill(dev, teacher=V, student=V):
    return M.LowLightLCMDistillation(network(1, teacher), network(0, student)).to(dev)


def config(tmp, **kw):
    base = dict(image_size=S, batch_size=B, epochs=2, use_amp=False, scheduler_type="cosine", warmup_epochs=0, log_interval=0,
                save_interval=100, sample_interval=100, seed=SEED, progress=False, output_dir=str(tmp / "out"),
                checkpoint_dir=str(tmp / "ckpt"))
    base.update(kw)
    return M.TrainingConfig(**base)


def new_distiller(dev, stores, cfg, val_batch=None, crop=S, **kw):
    train = M.DevicePairLoader(stores[0], B, crop, "train", SEED)
    val = M.DevicePairLoader(stores[1], val_batch, crop, "val", SEED) if val_batch else None
    return M.LowLightDistiller(new_distill(dev), train, val, cfg, **kw)


def state_of(distill, opt, scaler=None):
    """Everything a step changes, as clones: the student, both moments, the EMA student, the LR and the scaler's state."""
    ps = list(distill.student.parameters())
    st = {"student": [p.detach().clone() for p in ps], "exp_avg": [opt.state[p]["exp_avg"].clone() for p in ps],
          "exp_avg_sq": [opt.state[p]["exp_avg_sq"].clone() for p in ps], "lr": opt.param_groups[0]["lr"],
          "ema_student": [p.detach().clone() for p in distill.ema_student.parameters()],
          "teacher": [p.detach().clone() for p in distill.teacher.parameters()]}
    if scaler is not None:
        st["scaler"] = scaler.state_dict()
    return st


def assert_same_state(got, want, what):
    assert set(got) == set(want), what
    for key in want:
        if isinstance(want[key], list):
            bad = [i for i, (a, b) in enumerate(zip(got[key], want[key])) if not torch.equal(a, b)]
            assert not bad and len(got[key]) == len(want[key]), f"{what}: {key} differs in tensors {bad[:5]} ({len(bad)} of {len(want[key])})"
        else:
            assert got[key] == want[key], f"{what}: {key} {got[key]!r} != {want[key]!r}"


# ------------------------------------------------------------------ 1: the distiller is the loop it claims to be
@pytest.fixture(scope="module")
def written_out(dev, stores):
    """Two epochs of the loop LowLightDistiller's docstring gives, written out."""
    distill = new_distill(dev)
    for m in (distill.teacher, distill.student, distill.ema_student):
        m.compute_dtype = "fp32"
    loader = M.DevicePairLoader(stores[0], B, S, "train", SEED)
    assert len(loader) == STEPS_PER_EPOCH
    opt = M.FusedAdamW(distill.student.parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    sched = CosineAnnealingLR(opt, T_max=STEPS_PER_EPOCH * 2, eta_min=1e-6)
    step = M.DistillStep(distill, opt, ema_decay=0.95)
    hi = 50 - 50 // 4  # a v student: the terminal idx is drawn
    epoch_losses = []
    for epoch in range(2):
        loader.set_epoch(epoch)
        g = torch.Generator(device=dev).manual_seed((SEED * 1000003 + epoch * 8191 + 76543) % (2 ** 63 - 1))
        losses = []
        for batch in loader:
            b = batch["low_light"].shape[0]
            noise = torch.randn(b, 3, S, S, generator=g, device=dev)
            idx = torch.randint(0, hi, (b,), generator=g, device=dev)
            losses.append(step(batch["low_light"], batch["normal_light"], 4, noise=noise, idx=idx))
            opt._opt_called = True
            sched.step()
        total = 0.0
        for v in losses:
            total += v.item()
        epoch_losses.append(total / len(loader))
    return state_of(distill, opt), epoch_losses


def test_distiller_is_the_written_out_loop(dev, stores, written_out, tmp_path, recwarn):
    want, want_losses = written_out
    ds = new_distiller(dev, stores, config(tmp_path))
    assert ds.scaler is None and ds.scheduler.T_max == 6 and ds.optimizer.ema_decay is None
    assert (ds.skip_terminal, ds.idx_range, ds.num_inference_steps, ds.ema_decay) == (False, 38, 4, 0.95)
    assert all(m.compute_dtype == "fp32" for m in (ds.distill.teacher, ds.distill.student, ds.distill.ema_student))
    teacher_before = [p.detach().clone() for p in ds.distill.teacher.parameters()]
    history = ds.train()
    assert not [w for w in recwarn.list if "lr_scheduler.step()" in str(w.message)]
    print("epoch losses", [h["train_loss"] for h in history], "written out", want_losses)
    assert [h["train_loss"] for h in history] == want_losses and all(np.isfinite(v) for v in want_losses)
    assert [h["epoch"] for h in history] == [0, 1] and all(h["psnr"] is None and "val_loss" not in h for h in history)
    assert history[-1]["lr"] == want["lr"] and ds.global_step == 6 and ds.epoch == 1
    assert_same_state(state_of(ds.distill, ds.optimizer), want, "distiller against the written-out loop")
    assert all(torch.equal(a, b) for a, b in zip(ds.distill.teacher.parameters(), teacher_before))
    assert any(not torch.equal(a, b) for a, b in zip(ds.distill.student.parameters(), ds.distill.ema_student.parameters()))
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["final_model.pt"]


def test_skip_terminal_default_follows_the_student(dev, stores, tmp_path):
    train = M.DevicePairLoader(stores[0], B, S, "train", SEED)
    eps = M.LowLightDistiller(new_distill(dev, V, "epsilon"), train, None, config(tmp_path))
    assert (eps.skip_terminal, eps.idx_range) == (True, 37)
    assert np.isfinite(eps.train_epoch())  # no draw reaches alpha-bar 0
    both = M.LowLightDistiller(new_distill(dev, "epsilon", V), train, None, config(tmp_path), skip_terminal=True, num_inference_steps=8)
    assert (both.skip_terminal, both.idx_range, both.num_inference_steps) == (True, 43, 8)


# ------------------------------------------------------------------ 2: validation and sampling change nothing
def test_validation_and_sampling_are_side_effect_free(dev, stores, written_out, tmp_path, monkeypatch):
    want, want_losses = written_out
    ds = new_distiller(dev, stores, config(tmp_path, sample_interval=1), val_batch=B)
    modes = []
    validate = ds.validate
    monkeypatch.setattr(ds, "validate", lambda: (validate(), modes.append((ds.distill.student.training, ds.distill.ema_student.training,
                                                                          ds.distill.teacher.training)))[0])
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    history = ds.train()
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(dev), dev_rng)
    assert modes == [(True, False, False)] * 2
    assert [h["train_loss"] for h in history] == want_losses
    assert_same_state(state_of(ds.distill, ds.optimizer), want, "with validation and samples against the written-out loop")
    for h in history:
        assert np.isfinite(h["psnr"]) and 0 < h["ssim"] < 1
    assert ds.best_psnr == max(h["psnr"] for h in history)
    assert ds.train_loader.epoch == 2  # the loop's own count: the sample sheet's peek at a loader is not an epoch
    assert ds.validate() == history[-1]["psnr"]
    assert sorted(os.listdir(tmp_path / "out")) == ["samples_epoch_0.png", "samples_epoch_1.png"]
    ds.val_loader.set_epoch(5)
    ds.generate_samples(8)
    assert ds.val_loader.epoch == 5
    ds.val_loader = None
    ds.train_loader.set_epoch(7)
    ds.generate_samples(9)
    assert ds.train_loader.epoch == 7 and (tmp_path / "out" / "samples_epoch_9.png").exists()
    assert_same_state(state_of(ds.distill, ds.optimizer), want, "after one more sample sheet")


# ------------------------------------------------------------------ 3: resume; files and layout
def run_straight_and_resumed(dev, stores, tmp, **kw):
    """Two epochs straight, and the first of the two scheduled epochs -> final_model.pt -> a new distiller with resume_from -> the
    second.  Both legs are built with the 2-epoch configuration (the LR schedule is a function of it)."""
    common = dict(epochs=2, save_interval=1, sample_interval=1, **kw)
    straight = new_distiller(dev, stores, config(tmp / "a", **common), val_batch=4)
    straight_history = straight.train()
    first = new_distiller(dev, stores, config(tmp / "b", **common), val_batch=4)
    first.config.epochs = 1
    first_history = first.train()
    resumed = new_distiller(dev, stores, config(tmp / "c", resume_from=str(tmp / "b" / "ckpt" / "final_model.pt"), **common), val_batch=4)
    assert resumed.epoch == 1 and resumed.global_step == 3
    resumed_history = resumed.train()
    return straight, straight_history, resumed, first_history + resumed_history


def check_resume(straight, straight_history, resumed, resumed_history):
    print("straight", straight_history)
    print("resumed ", resumed_history)
    assert json.dumps(resumed_history) == json.dumps(straight_history)  # as text: a NaN loss equals itself
    assert (resumed.epoch, resumed.global_step, resumed.best_psnr) == (straight.epoch, straight.global_step, straight.best_psnr) \
        and straight.global_step == 6
    assert resumed.scheduler.state_dict() == straight.scheduler.state_dict()
    assert resumed.optimizer.state_dict()["state"][0]["step"] == straight.optimizer.state_dict()["state"][0]["step"]
    assert_same_state(state_of(resumed.distill, resumed.optimizer, resumed.scaler),
                      state_of(straight.distill, straight.optimizer, straight.scaler), "resumed against straight")


@pytest.fixture(scope="module")
def fp32_runs(dev, stores, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("distill_fp32")
    return (tmp,) + run_straight_and_resumed(dev, stores, tmp)


def test_resume_fp32(fp32_runs):
    check_resume(*fp32_runs[1:])


def test_resume_fp16_with_grad_scaler(dev, stores, tmp_path):
    straight, sh, resumed, rh = run_straight_and_resumed(dev, stores, tmp_path, use_amp=True)
    assert straight.scaler is not None and straight.distill.student.compute_dtype == "fp16"
    assert straight.distill.teacher.compute_dtype == "fp16" and straight.distill.ema_student.compute_dtype == "fp16"
    steps = int(straight.optimizer.state_dict()["state"][0]["step"])
    print("fp16: updates taken", steps, "of 6, scaler", straight.scaler.state_dict())
    assert 0 <= steps <= 6
    check_resume(straight, sh, resumed, rh)
    assert "scaler_state_dict" in straight.checkpoint()


def test_files_and_checkpoint_layout(dev, stores, fp32_runs, tmp_path):
    tmp, straight, history = fp32_runs[0], fp32_runs[1], fp32_runs[2]
    ckpt_dir, out_dir = tmp / "a" / "ckpt", tmp / "a" / "out"
    assert sorted(os.listdir(ckpt_dir)) == ["best_model.pt", "checkpoint_epoch_0.pt", "checkpoint_epoch_1.pt", "final_model.pt"]
    assert sorted(os.listdir(out_dir)) == ["samples_epoch_0.png", "samples_epoch_1.png"]
    want_entry = {"num_ddim_timesteps": 50, "num_inference_steps": 4, "ema_decay": 0.95, "teacher_prediction": V,
                  "student_prediction": V, "skip_terminal": False}
    for name, epoch in (("checkpoint_epoch_0.pt", 0), ("best_model.pt", None), ("final_model.pt", 1)):
        ckpt = torch.load(ckpt_dir / name, map_location="cpu", weights_only=True)
        assert set(ckpt) == set(D.DISTILL_CHECKPOINT_KEYS), name  # fp32: no scaler; the teacher is not stored
        assert ckpt["distill"] == want_entry and ckpt["config"] == straight.config.__dict__
        assert not any(k.startswith("teacher") for k in ckpt["model_state_dict"])
        if epoch is not None:
            assert ckpt["epoch"] == epoch and ckpt["global_step"] == 3 * (epoch + 1)
        else:
            best = max(range(2), key=lambda e: (history[e]["psnr"], -e))
            assert ckpt["epoch"] == best and ckpt["best_psnr"] == history[best]["psnr"] == straight.best_psnr
    # model_state_dict is the EMA student: what the other scripts read is the deployable network
    fresh = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4, compute_dtype="fp32", scheduler=scheduler(V))
    meta = M.load_checkpoint(fresh, str(ckpt_dir / "final_model.pt"))
    assert meta["epoch"] == 1 and meta["global_step"] == 6
    fresh = fresh.to(dev).eval()
    ema = straight.distill.ema_student
    for (k, a), b in zip(fresh.state_dict().items(), ema.state_dict().values()):
        assert torch.equal(a, b), k
    assert all(torch.equal(v.cpu(), w.cpu()) for v, w in zip(ckpt["student_state_dict"].values(), straight.distill.student.state_dict().values()))
    g = torch.Generator(device=dev).manual_seed(5)
    low = torch.rand(2, 3, S, S, generator=g, device=dev) * 0.6 - 1.0
    noise = torch.randn(4, 2, 3, S, S, generator=g, device=dev)
    out = fresh.enhance(low, 4, noise=noise)
    assert torch.isfinite(out).all() and torch.equal(out, ema.enhance(low, 4, noise=noise))

    # a file written by another distillation is refused, naming the field; so is a trainer-style file
    resume = str(ckpt_dir / "final_model.pt")
    for kw, field in ((dict(ema_decay=0.9), "ema_decay"), (dict(num_inference_steps=8), "num_inference_steps"),
                      (dict(skip_terminal=True), "skip_terminal")):
        with pytest.raises(ValueError, match=field):
            new_distiller(dev, stores, config(tmp_path, resume_from=resume), **kw)
    train = M.DevicePairLoader(stores[0], B, S, "train", SEED)
    with pytest.raises(ValueError, match="student_prediction"):
        M.LowLightDistiller(new_distill(dev, V, "epsilon"), train, None, config(tmp_path, resume_from=resume), skip_terminal=False)
    with pytest.raises(ValueError, match="num_ddim_timesteps"):
        M.LowLightDistiller(M.LowLightLCMDistillation(network(1), network(0), num_ddim_timesteps=40).to(dev), train, None,
                            config(tmp_path, resume_from=resume))
    del ckpt["distill"]
    torch.save(ckpt, tmp_path / "plain.pt")
    with pytest.raises(ValueError, match="not a LowLightDistiller checkpoint"):
        new_distiller(dev, stores, config(tmp_path, resume_from=str(tmp_path / "plain.pt")))


# ------------------------------------------------------------------ 4: a rectangular crop; windows
def test_a_rectangular_epoch(dev, tmp_path):
    """crop_size = (64, 96), from 72 x 104 frames (the 72 x 80 ones are too narrow for it)."""
    wide = (M.DeviceFrameStore(*frames(6, 13, (72, 104)), device=dev), M.DeviceFrameStore(*frames(4, 14, (72, 104)), device=dev))
    ds = new_distiller(dev, wide, config(tmp_path, epochs=1, sample_interval=1), val_batch=B, crop=(64, 96), crop_size=(64, 96))
    history = ds.train()
    assert np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["psnr"])
    from PIL import Image
    with Image.open(tmp_path / "out" / "samples_epoch_0.png") as im:
        assert (im.height, im.width) == (3 * 66 + 2, 2 * 98 + 2)
    with pytest.raises(ValueError, match="multiples of 8 and at least 64"):
        new_distiller(dev, wide, config(tmp_path), crop=(60, 96), crop_size=(60, 96))


def test_accumulate_two_takes_two_steps_per_epoch(dev, stores, tmp_path):
    ds = new_distiller(dev, stores, config(tmp_path, epochs=1), accumulate=2)
    assert ds.scheduler.T_max == 2
    history = ds.train()
    assert ds.global_step == 2 and ds.step.window_images == 0 and np.isfinite(history[0]["train_loss"])


# ------------------------------------------------------------------ 5: the scripts
def test_distill_script_then_inference(dev, tmp_path):
    from PIL import Image
    for root, (low, high) in (("train", frames(4, 21)), ("val", frames(2, 22))):
        for sub, imgs in (("low", low), ("high", high)):
            os.makedirs(tmp_path / root / sub)
            for i, f in enumerate(imgs):
                Image.fromarray(f).save(tmp_path / root / sub / f"{i}.png")
    torch.save({"model_state_dict": network(1).state_dict()}, tmp_path / "teacher.pt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "distill.py"), "--teacher", str(tmp_path / "teacher.pt"),
                        "--init_student", str(tmp_path / "teacher.pt"), "--teacher_prediction", V, "--student_prediction", V,
                        "--data_dir", str(tmp_path / "train"), "--val_dir", str(tmp_path / "val"), "--image_size", "64", "--batch_size", "2",
                        "--epochs", "1", "--seed", "3", "--checkpoint_dir", str(tmp_path / "ckpt"), "--output_dir", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    logs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(logs) == 1 and logs[0]["epoch"] == 0 and np.isfinite(logs[0]["train_loss"]) and np.isfinite(logs[0]["psnr"])
    assert set(logs[0]) == {"epoch", "train_loss", "lr", "psnr", "ssim"}
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["best_model.pt", "final_model.pt"]
    assert (tmp_path / "out" / "samples_epoch_0.png").exists()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "inference.py"), "--checkpoint", str(tmp_path / "ckpt" / "final_model.pt"),
                        "--prediction", V, "--image_size", "64", "--input", str(tmp_path / "val" / "low" / "0.png"),
                        "--output", str(tmp_path / "enhanced.png")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with Image.open(tmp_path / "enhanced.png") as im:
        assert (im.height, im.width) == (72, 80)
