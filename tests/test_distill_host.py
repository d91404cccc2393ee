"""Consistency distillation (LowLightLCMDistillation / DistillStep) without a GPU: exports, the module's structure against
the reference's (tests/golden/distill_small64.npz, tools/make_golden_distill.py), the timestep-pair rule and the refusal of
CPU tensors."""
import copy
import importlib

import numpy as np
import pytest
import torch

M = importlib.import_module("cv-diffusion-model_amd")


def _distill(teacher="small", student="small", size=64, **kw):
    t = M.LowLightDiffusion(unet_variant=teacher, image_size=size, num_inference_steps=4)
    s = M.LowLightDiffusion(unet_variant=student, image_size=size, num_inference_steps=4)
    return M.LowLightLCMDistillation(t, s, **kw)


def test_classes_are_exported():
    assert "LowLightLCMDistillation" in M.__all__ and "DistillStep" in M.__all__
    assert issubclass(M.LowLightLCMDistillation, torch.nn.Module)
    assert callable(M.DistillStep)


def test_state_dict_keys_match_reference(golden):
    g = golden("distill_small64.npz")
    d = _distill()
    assert list(d.state_dict().keys()) == [str(k) for k in g["state_keys"]]
    assert [k for k, _ in d.student.named_parameters()] == [str(k) for k in g["keys"]]
    assert d.num_ddim_timesteps == 50 and d.guidance_scale_range == (3.0, 15.0)


def test_ema_student_is_an_independent_copy():
    d = _distill()
    pairs = list(zip(d.student.parameters(), d.ema_student.parameters()))
    assert len(pairs) == 381
    for a, b in pairs:
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    with torch.no_grad():
        pairs[0][0].add_(1.0)
    assert not torch.equal(pairs[0][0], pairs[0][1])
    assert d.ema_student.unet._handles == {} and d.ema_student.unet is not d.student.unet
    assert not d.ema_student.training and not any(p.requires_grad for p in d.ema_student.parameters())
    assert d.student.training and all(p.requires_grad for p in d.student.parameters())


def test_teacher_is_frozen():
    d = _distill()
    assert not d.teacher.training
    assert not any(p.requires_grad for p in d.teacher.parameters())


def test_teacher_variant_may_differ_but_size_may_not():
    d = _distill(teacher="large", student="small")
    assert d.teacher.unet.config.base_channels == 64 and d.student.unet.config.base_channels == 32
    with pytest.raises(ValueError, match="image_size"):
        M.LowLightLCMDistillation(M.LowLightDiffusion(image_size=64), M.LowLightDiffusion(image_size=72))


@pytest.mark.parametrize("steps", [4, 6, 8])
def test_timestep_pairs(golden, steps):
    d = _distill()
    c, k = 1000 // 50, 50 // steps
    idx = torch.arange(0, 50 - k)
    t, t_next = d.timestep_pairs(idx, steps)
    assert torch.equal(t, idx * c + c - 1) and torch.equal(t_next, (idx + k) * c + c - 1)
    assert int(t_next.max()) == 999 and int(t.min()) == 19      # the last idx reaches the zero-SNR end of the table
    assert bool((t_next > t).all())                              # t_next is the noisier timestep, as written
    g = golden("distill_small64.npz")
    for case in ("seeded", "inf"):
        gi = torch.from_numpy(g[f"{case}/idx"])
        t, t_next = d.timestep_pairs(gi, 4)
        assert torch.equal(t, gi * 20 + 19) and torch.equal(t_next, (gi + 12) * 20 + 19)
    assert torch.equal(d.timestep_pairs(torch.from_numpy(g["inf/idx"]), 4)[1], torch.tensor([999, 259]))


def test_cpu_tensors_are_refused():
    d = _distill()
    low = torch.zeros(2, 3, 64, 64)
    with pytest.raises(RuntimeError, match="HIP device.*no CPU fallback"):
        d.consistency_distillation_loss(low, low)
    with pytest.raises(RuntimeError, match="HIP device.*no CPU fallback"):
        d.update_ema()


def test_deepcopy_of_the_module_copies_everything():
    d = _distill()
    d2 = copy.deepcopy(d)
    for (k, a), (k2, b) in zip(d.state_dict().items(), d2.state_dict().items()):
        assert k == k2 and torch.equal(a, b) and a.data_ptr() != b.data_ptr()


def test_golden_inf_case_is_recorded_as_inf(golden):
    """The fixture documents the reference quirk: idx = 37 -> t_next = 999 -> loss +inf with finite gradients."""
    g = golden("distill_small64.npz")
    assert np.isposinf(g["inf/loss"]) and np.isfinite(g["inf/grad_norms"]).all()
    assert np.isfinite(g["seeded/loss"]) and g["seeded/grad_norms"].shape == (381,)
