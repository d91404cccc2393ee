"""The UNet inference cases of tests/test_gpu_workspace_poison.py reach every form of the inverted-residual block.

Those cases run a 2-byte `small` engine at the frames and under the knob sets of tests/poison_refs.py.  A form none of them reaches
would keep its arena traffic and its zeroed totals out of the poison tests without anybody noticing, so the union of
llie_irb_forms / llie_irb_wide_gram over the cases must contain every form (0 unfused, 1 recompute, 2 project, 3 wide) and at least
one block in the wide Gram form.  Host only: the rule of engine.h (irb_path) needs no GPU."""
import importlib

import pytest

from poison_refs import FORM_NAMES, FRAMES, KNOB_SETS, irb_forms, knobs, unet_module

N = importlib.import_module("cv-diffusion-model_amd._native")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_inference_cases_reach_every_block_form(dtype):
    m = unet_module("small")
    h = N.Handle(m._make_cfg(N.dtype_code(dtype)))
    try:
        seen, wide_gram = {}, []
        for settings in KNOB_SETS:
            with knobs(settings):
                for H, W in FRAMES:
                    for cin, hid, cout, bh, bw, form, wg in irb_forms(h, H, W):
                        seen.setdefault(form, (settings, (H, W), (cin, hid, cout, bh, bw)))
                        if wg:
                            assert form == 3
                            wide_gram.append((settings, (H, W), (cin, hid, cout, bh, bw)))
        for form, where in sorted(seen.items()):
            print(f"{dtype}: form {form} ({FORM_NAMES[form]}) first reached by knobs {where[0]} at frame {where[1]}, block {where[2]}")
        print(f"{dtype}: wide Gram blocks: {wide_gram}")
        assert sorted(seen) == [0, 1, 2, 3], f"forms left out: {sorted(set(FORM_NAMES) - set(seen))}"
        assert wide_gram, "no case takes the wide Gram form"
        # the knobs are the defaults again: the default frame takes no wide Gram block (maps below 4096 pixels)
        assert not any(r[6] for r in irb_forms(h, 64, 64))
    finally:
        h.close()


def test_fp32_engine_is_unfused_everywhere():
    """The fp32 cases run one form only, which is why they are not repeated under the knob sets."""
    m = unet_module("small")
    h = N.Handle(m._make_cfg(N.LLIE_F32))
    try:
        for settings in KNOB_SETS:
            with knobs(settings):
                for H, W in FRAMES:
                    assert {r[5] for r in irb_forms(h, H, W)} == {0}, (settings, H, W)
    finally:
        h.close()
