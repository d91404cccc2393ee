"""Byte model of the engine's launch sequence (llie_path_bytes) for the recompute blocks that keep h2 on chip: needs no GPU."""
import importlib

import torch  # noqa: F401  (the library binds to the HIP runtime PyTorch loaded)

M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")

# the recompute blocks of small@256 that take the project form: (Cin, Chid, pixels, how many).  Identity-residual blocks of the
# 32- and 64-channel levels, and the last decoder level's 96 -> 32 block (skip conv, 64 + 32 concatenated channels)
IDENTITY = [(32, 128, 256 * 256, 4), (64, 256, 128 * 128, 3)]
SKIP = [(96, 384, 256 * 256, 1)]
# llie_path_bytes of small@256 fp16 at batch 1 and 32 with every recompute block at 3Cin + 2Chid + Cout
PATH_BYTES_PROJECT_OFF_B1, PATH_BYTES_PROJECT_OFF_B32 = 830513484, 25238348108


def saved_elems(blocks):
    """3Cin + 2Chid + Cout -> 4Cin + Cout: 2 Chid - Cin elements per pixel and block"""
    return sum(n * (2 * chid - cin) * p for cin, chid, p, n in blocks)


def test_path_bytes_charges_project_form_blocks_4cin_plus_cout():
    L = N.lib()
    m = M.LowLightDiffusion(unet_variant="small", image_size=256)
    h = N.Handle(m.unet._make_cfg(N.LLIE_F16))
    try:
        got = {}
        for v in (0, 2, 1):
            N.check(L.llie_tune(b"irbx_project", v))
            got[v] = [h.path_bytes(b) for b in (1, 32)]
        for i, b in enumerate((1, 32)):
            assert got[0][i] - got[2][i] == 2 * b * saved_elems(IDENTITY), (b, got)
            assert got[2][i] - got[1][i] == 2 * b * saved_elems(SKIP), (b, got)
        # irbx_project = 0: every recompute block at 3Cin + 2Chid + Cout, the figure from before the project form was charged
        assert got[0] == [PATH_BYTES_PROJECT_OFF_B1, PATH_BYTES_PROJECT_OFF_B32], got[0]
        # the materialised model (h1 written and read) does not look at the knob
        N.check(L.llie_tune(b"irbx_project", 0))
        a0 = h.algorithmic_bytes(32)
        N.check(L.llie_tune(b"irbx_project", 1))
        assert h.algorithmic_bytes(32) == a0
    finally:
        N.check(L.llie_tune(b"irbx_project", 1))
        h.close()


