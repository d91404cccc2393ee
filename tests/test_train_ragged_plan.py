"""Training at image sizes that are not a multiple of 64: the dry run of the training step
(llie_train_workspace_bytes replays the forward and backward launch sequences without launching) plans every size
inference accepts for the pinned variants, and the refusals that remain are still there.  No GPU needed."""
import importlib

import pytest

M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")


def _plan(variant, size, batch, dtype, **kw):
    m = M.LowLightDiffusion(unet_variant=variant, image_size=size, **kw)
    return N.Handle(m.unet._make_cfg(dtype)).train_workspace_bytes(batch)


@pytest.mark.parametrize("variant,size", [("small", 72), ("small", 96), ("small", 104), ("small", 200), ("small", 224),
                                          ("large", 72), ("large", 200)])
def test_training_plan_at_sizes_off_the_multiples_of_64(variant, size):
    for dtype in (N.LLIE_F32, N.LLIE_F16, N.LLIE_BF16):
        for batch in (1, 2, 3):
            assert _plan(variant, size, batch, dtype) > 0
    # the padded partial buffers keep the plan between those of its neighbours on the 64 grid
    lo, hi = size // 64 * 64 or 64, (size + 63) // 64 * 64
    w = _plan(variant, size, 2, N.LLIE_F32)
    assert _plan(variant, lo, 2, N.LLIE_F32) <= w <= _plan(variant, hi, 2, N.LLIE_F32) * 1.05


@pytest.mark.parametrize("size", [60, 100, 32])
def test_sizes_inference_refuses_are_refused_for_training_too(size):
    with pytest.raises(ValueError):
        M.LowLightDiffusion(unet_variant="small", image_size=size)


@pytest.mark.parametrize("variant", ["tiny", "base"])
def test_unpinned_variants_stay_inference_only(variant):
    for size in (64, 72):
        with pytest.raises(ValueError, match="inference-only"):
            _plan(variant, size, 1, N.LLIE_F32, allow_unpinned_groupnorm=True)
