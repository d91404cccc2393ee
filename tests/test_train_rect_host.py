"""Training at a frame's own H x W, the parts that need no GPU: the shape rule (llie_train_shape_ok), the dry run of the
training step at rectangular frames (llie_train_workspace_bytes replays the forward and backward launch sequences without
launching), the CPU oracle's autograd pinned to the reference's own vectors (tests/golden/train_small_rect.npz,
tools/make_golden_train_rect.py), and the Python surface (keywords, the command line)."""
import importlib
import inspect
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import scheduler_ref as S
from conftest import ROOT, synth_input

M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")

RECT = [(64, 96), (96, 64), (72, 104), (64, 128), (128, 64)]


def _handle(variant="small", size=64, dtype=N.LLIE_F32, **kw):
    m = M.LowLightDiffusion(unet_variant=variant, image_size=size, **kw)
    return N.Handle(m.unet._make_cfg(dtype))


# ------------------------------------------------------------------ the shape rule
@pytest.mark.parametrize("size", [64, 256])
def test_train_shape_ok(size):
    h = _handle(size=size)
    L = N.lib()
    for hh, ww in ((64, 96), (400, 600)):
        assert L.llie_train_shape_ok(h.h, 8, hh, ww) == 0, (hh, ww)
        h.train_shape_ok(8, hh, ww)
    for hh, ww in ((60, 96), (64, 100), (56, 96), (96, 56)):
        assert L.llie_train_shape_ok(h.h, 8, hh, ww) == N.ERR_SHAPE, (hh, ww)
        with pytest.raises(ValueError, match="multiples of 8 and at least 64"):
            h.train_shape_ok(8, hh, ww)
    # the element cap: small stores 384 channels at full resolution, so 2^31 - 1 elements are 5 592 405 pixels
    assert L.llie_train_shape_ok(h.h, 1, 2048, 2728) == 0          # 5 586 944 pixels
    assert L.llie_train_shape_ok(h.h, 1, 2048, 2736) == N.ERR_SHAPE  # 5 603 328
    assert L.llie_train_shape_ok(h.h, 8, 1080, 1920) == N.ERR_SHAPE  # eight full-HD frames
    with pytest.raises(ValueError, match="element cap"):
        h.train_shape_ok(8, 1080, 1920)
    assert L.llie_train_shape_ok(h.h, 0, 64, 96) == N.ERR_ARG
    # never wider than the frame rule of inference
    for b, hh, ww in ((1, 2048, 2728), (1, 2048, 2736), (3, 1080, 1920), (2, 1080, 1920), (70000, 64, 64)):
        if L.llie_train_shape_ok(h.h, b, hh, ww) == 0:
            assert L.llie_frame_shape_ok(h.h, b, hh, ww) == 0


def test_train_shape_rule_at_the_cap():
    """The rule multiplies the rows the weight-gradient GEMM walks -- every image padded to whole 64-row chunks -- by the widest
    channel count.  H and W are multiples of 8, so H x W is a multiple of 64 and the padding adds nothing at full resolution:
    for `small` (384 channels, wider than the up-sampled tensor's 64 and the packed copies' 32) the training rule and the frame
    rule refuse the same frames, and the boundary sits where batch x H x W x 384 crosses 2^31 - 1."""
    h = _handle()
    L = N.lib()
    cap = 2 ** 31 - 1
    for hh, ww in ((72, 72), (72, 104), (64, 96)):
        assert (hh * ww) % 64 == 0
        b = cap // (hh * ww * 384)
        assert L.llie_train_shape_ok(h.h, b, hh, ww) == 0 and L.llie_train_shape_ok(h.h, b + 1, hh, ww) == N.ERR_SHAPE
        assert L.llie_frame_shape_ok(h.h, b, hh, ww) == 0 and L.llie_frame_shape_ok(h.h, b + 1, hh, ww) == N.ERR_SHAPE


@pytest.mark.parametrize("variant", ["tiny", "base"])
def test_unpinned_variants_stay_refused(variant):
    h = _handle(variant, allow_unpinned_groupnorm=True)
    assert N.lib().llie_train_shape_ok(h.h, 1, 64, 96) == N.ERR_CONFIG
    with pytest.raises(ValueError, match="inference-only"):
        h.train_shape_ok(1, 64, 96)
    with pytest.raises(ValueError, match="inference-only"):
        h.train_workspace_bytes(1, 64, 96)


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("variant,size", [("small", 64), ("small", 72), ("small", 256), ("large", 64)])
def test_zero_zero_is_image_size(variant, size):
    for dtype in (N.LLIE_F32, N.LLIE_F16, N.LLIE_BF16):
        h = _handle(variant, size, dtype)
        for b in (1, 2, 3):
            assert h.train_workspace_bytes(b) == h.train_workspace_bytes(b, 0, 0) == h.train_workspace_bytes(b, size, size) > 0
    h = _handle(variant, size)
    L = N.lib()
    assert L.llie_train_workspace_bytes(h.h, 2, 64, 0) == N.ERR_ARG and L.llie_train_workspace_bytes(h.h, 2, 0, 64) == N.ERR_ARG


@pytest.mark.parametrize("variant", ["small", "large"])
def test_training_plan_at_rectangular_frames(variant):
    for dtype in (N.LLIE_F32, N.LLIE_F16, N.LLIE_BF16):
        h = _handle(variant, 64, dtype)
        for hh, ww in RECT + [(400, 600)]:
            for b in (1, 2, 3):
                assert h.train_workspace_bytes(b, hh, ww) > 0, (hh, ww, b)
    h = _handle(variant, 64)
    sq64, sq128 = h.train_workspace_bytes(2, 64, 64), h.train_workspace_bytes(2, 128, 128)
    # a frame's plan lies between those of the squares that enclose it, and does not depend on image_size (the module tree of
    # `small` is the same at 64 and 256 but for where attention sits, so only compare like with like)
    for hh, ww in RECT:
        w = h.train_workspace_bytes(2, hh, ww)
        assert sq64 <= w <= sq128 * 1.05, (hh, ww, w)
    # H x W and W x H hold the same tensors; tile counts may differ by the ragged strips, not by more than a few per cent
    for hh, ww in ((64, 96), (64, 128)):
        a, b = h.train_workspace_bytes(2, hh, ww), h.train_workspace_bytes(2, ww, hh)
        assert abs(a - b) <= 0.05 * a
    with pytest.raises(ValueError, match="multiples of 8 and at least 64"):
        h.train_workspace_bytes(2, 60, 96)
    with pytest.raises(ValueError, match="multiples of 8 and at least 64"):
        h.train_workspace_bytes(2, 64, 100)


# ------------------------------------------------------------------ the oracle against the reference's own vectors
@pytest.mark.parametrize("hh,ww", [(64, 96), (72, 104)])
def test_oracle_autograd_vs_reference_golden_rect(golden, hh, ww):
    """PyTorch autograd over the CPU oracle built at image_size = 64 and fed hh x ww, against the reference model's own step:
    loss to 1e-5, every gradient norm to 5e-3 relative.  This is what lets the GPU tests use the oracle's autograd as the
    reference at shapes the golden file does not hold."""
    g = golden("train_small_rect.npz")
    pre = f"{hh}x{ww}:"
    spec = oracle.make_spec("small", 64)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    tag = f"train{hh}x{ww}"
    low = synth_input(tag + ".low", (2, 3, hh, ww), -1.0, -0.4)
    normal = synth_input(tag + ".normal", (2, 3, hh, ww), -1, 1)
    noise = synth_input(tag + ".noise", (2, 3, hh, ww), -2, 2)
    t = torch.from_numpy(g[pre + "timesteps"])
    assert t[0] != t[1]
    tab = S.LCMTables.build(rescale_betas_zero_snr=True)
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pred = oracle.unet_forward(sdg, spec, torch.cat([S.add_noise(tab, normal, noise, t), low], 1), t)
    assert tuple(pred.shape) == (2, 3, hh, ww)
    loss = F.mse_loss(pred, noise)
    loss.backward()
    assert abs(loss.item() - float(g[pre + "loss"])) < 1e-5, (loss.item(), float(g[pre + "loss"]))
    keys = [str(k) for k in g["keys"]]
    assert len(keys) == len(sd)
    norms = np.array([sdg[k].grad.double().norm().item() for k in keys])
    rel = np.abs(norms - g[pre + "grad_norms"]) / np.maximum(g[pre + "grad_norms"], 1e-12)
    assert rel.max() < 5e-3, (keys[int(rel.argmax())], rel.max())
    full = [n for n in g.files if n.startswith(pre + "grad:")]
    assert len(full) >= 10
    for name in full:
        ref = torch.from_numpy(g[name]).double()
        got = sdg[name[len(pre) + len("grad:"):]].grad.double()
        assert ((got - ref).norm() / ref.norm()).item() < 5e-3, name


# ------------------------------------------------------------------ the Python surface
def test_keywords_exist_and_default_to_the_square():
    assert inspect.signature(M.EfficientUNet.forward_split).parameters["frame"].default is False
    assert inspect.signature(M.LowLightDiffusion.forward).parameters["frame"].default is False
    for fn in (M.LowLightTrainer.__init__, M.train_model):
        p = inspect.signature(fn).parameters["crop_size"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "crop_size" not in M.TrainingConfig.__dataclass_fields__  # a keyword, like the x0 weights: not stored in checkpoints
    for name in ("llie_train_shape_ok", "llie_unet_train_forward_hw", "llie_aug_pair_u8_hw", "llie_aug_synth_u8_hw"):
        assert name in N.EXPORTS and getattr(N.lib(), name)


def test_forward_refuses_other_shapes_without_the_keyword():
    """What the square entry refused before it still refuses (before any device is asked for); with frame=True the shape goes
    to the engine's rule, which needs a device to run but not to refuse a channel split."""
    m = M.LowLightDiffusion(unet_variant="small", image_size=64)
    z = torch.zeros(1, 3, 64, 96)
    with pytest.raises(ValueError, match="frame=True"):
        m.unet.forward_split(z, z, torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError, match="one size"):
        m.unet.forward_split(z, torch.zeros(1, 3, 96, 64), torch.zeros(1, dtype=torch.long), frame=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.unet.forward_split(z, z, torch.zeros(1, dtype=torch.long), frame=True)


def test_train_script_takes_both_crop_flags_or_neither(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        T = importlib.import_module("train")
    finally:
        sys.path.pop(0)
    args = T.parse_args([])
    assert T.crop_size_from_args(args) == {"crop_size": None}
    args = T.parse_args(["--crop_height", "400", "--crop_width", "600"])
    assert T.crop_size_from_args(args) == {"crop_size": (400, 600)}
    assert not hasattr(T.config_from_args(args), "crop_size")
    for argv in (["--crop_height", "400"], ["--crop_width", "600"]):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert "both or neither" in capsys.readouterr().err
