"""llie_init_conv_dgrad -- the data gradient of the input conv, init_conv_dgrad_kernel (bwd.hip) -- against the float64 reference of
tests/input_grad_refs.py.

Method as tests/test_gpu_boundary_kernels.py: seeded fp32 draws rounded to the storage type; B = 2 and non-square maps; g and both
outputs between canaries, outputs prefilled with NaN and compared entry by entry; every call made twice with equal bits;
llie_last_kernel() asserted.  An entry passes when |out - ref| - slack < BAR_INIT_DGRAD * 2^-24 * abssum; the constant stands in
input_grad_refs.py with the measured worst ratios beside it.  tests/test_input_grad_host.py checks the reference against torch's own
operators and that the bar rejects subtly wrong kernels.

LLIE_FWD_TEST_SEED (default 0) shifts every seed: the bar was measured over seeds 0, 1 and 2.
"""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_grad_refs as G  # noqa: E402
from kernel_refs import NAN, TDT, Guarded, _ratio, _rt, _same  # noqa: E402

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

SEED0 = int(os.environ.get("LLIE_FWD_TEST_SEED", "0"))
TNAME = {0: "float", 1: "_Float16", 2: "__bf16"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _last():
    return N.lib().llie_last_kernel().decode()


def _run(dev, dtype, g, w, split, want0, want1):
    """one call on fresh guarded buffers -> (d_x0 or None, d_x1 or None) on the CPU, canaries of g, outputs and pack checked"""
    L = N.lib()
    B, H, W, C0 = g.shape
    c0, c1 = split
    gd = Guarded((B, H, W, C0), dev, TDT[dtype], 0.0)
    gd.v.copy_(_rt(g, dtype))
    wd = w.to(dev)
    nbytes = int(L.llie_init_conv_pack_bytes(c0 + c1, C0))
    assert nbytes > 0 and nbytes % 16 == 0
    pack = Guarded((nbytes // 4,), dev)
    d0 = Guarded((B, c0, H, W), dev) if want0 else None
    d1 = Guarded((B, c1, H, W), dev) if want1 else None
    N.check(L.llie_init_conv_dgrad(dtype, gd.ptr, C0, wd.data_ptr(), d0.ptr if want0 else None, c0, d1.ptr if want1 else None, c1,
                                   B, H, W, pack.ptr, nbytes, _st()), "init_conv_dgrad")
    torch.cuda.synchronize()
    assert _last() == f"init_conv_dgrad_kernel<{TNAME[dtype]}>", _last()
    pack.cpu("dgrad pack")
    assert torch.equal(gd.cpu("dgrad g").float(), _rt(g, dtype).float()), "g was written"
    return d0.cpu("d_x0") if want0 else None, d1.cpu("d_x1") if want1 else None


DGRAD_PARAMS = [(d, h, w, sp, co) for d in (0, 1, 2) for h, w in G.DGRAD_MAPS for sp in G.DGRAD_SPLITS for co in G.DGRAD_COUT]


@pytest.mark.parametrize("dtype,H,W,split,cout", DGRAD_PARAMS, ids=[f"dt{d}-{h}x{w}-c{s[0]}_{s[1]}-o{c}" for d, h, w, s, c in DGRAD_PARAMS])
def test_init_conv_dgrad_vs_float64(dev, dtype, H, W, split, cout):
    """From the reference's OIHW weights through the engine's own repack, B = 2.  Maps: 16 x 16 (exactly one 16 x 16 tile), 24 x 40
    (partial tiles on the right and bottom edges), 48 x 56 (3 x 4 tiles: tiles with neighbours on all four sides) and 40 x 24;
    channel splits 3 + 3, 4 + 4, 1 + 2 and 3 + 0; C0 32 and 64 (the second 32-channel block restages the patch); with both
    outputs, with d_x0 alone and with d_x1 alone -- a null output's channels are not computed, and the other's bits do not change.
    Measured worst ratio (MI355X, seeds 0..2): 3.04 fp32, 3.00 fp16, 3.15 bf16; bar BAR_INIT_DGRAD = 31."""
    B, (c0, c1) = 2, split
    g, w = G.dgrad_inputs(dtype, B, H, W, split, cout, SEED0)
    ref, ab, sl = G.init_conv_dgrad_ref(dtype, g, w)
    tag = f"{H}x{W}/c{c0}_{c1}/o{cout}/dt{dtype}"
    both = None
    for want0, want1 in ([(True, True), (True, False), (False, True)] if c1 else [(True, False)]):
        a, b = _run(dev, dtype, g, w, split, want0, want1), _run(dev, dtype, g, w, split, want0, want1)
        for x, y, n in zip(a, b, ("d_x0", "d_x1")):
            if x is not None:
                _same(x, y, n)
        if want0:
            _ratio(a[0], ref[:, :c0], ab[:, :c0], sl[:, :c0], G.BAR_INIT_DGRAD, f"init_dgrad/{tag}/x0{'+x1' if want1 else ''}")
        if want1:
            _ratio(a[1], ref[:, c0:], ab[:, c0:], sl[:, c0:], G.BAR_INIT_DGRAD, f"init_dgrad/{tag}/x1{'+x0' if want0 else ''}")
        if both is None:
            both = a
        else:  # one output alone: the bits it has beside the other
            for x, y, n in zip(a, both, ("d_x0 alone", "d_x1 alone")):
                if x is not None and y is not None:
                    _same(x, y, n)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_init_conv_dgrad_batch_independence(dev, dtype):
    """the rows of image 0 at B = 2 are the bits of the B = 1 call (24 x 40, C0 = 64, 3 + 3)"""
    g, w = G.dgrad_inputs(dtype, 2, 24, 40, (3, 3), 64, SEED0)
    a0, a1 = _run(dev, dtype, g, w, (3, 3), True, True)
    b0, b1 = _run(dev, dtype, g[:1].contiguous(), w, (3, 3), True, True)
    _same(a0[:1], b0, "d_x0 of image 0")
    _same(a1[:1], b1, "d_x1 of image 0")


def test_init_conv_dgrad_refusals(dev):
    """A dtype outside 0..2; NULL g, w_oihw or pack; a misaligned or short pack; c0 < 1, c1 < 0, more than 8 input channels; both outputs
    NULL; d_x1 with c1 == 0; H or W off the multiples of 8, batch 0 or above 65535; Cout 0, negative or off the multiples of 32:
    LLIE_ERR_ARG with nothing written and nothing launched."""
    L = N.lib()
    x = torch.full((2 * 16 * 16 * 64,), NAN, device=dev)
    out = torch.full((2 * 8 * 16 * 16,), NAN, device=dev)
    nb = int(L.llie_init_conv_pack_bytes(6, 32))
    pack = torch.full((nb // 4 + 4,), NAN, device=dev)
    p, o, k = x.data_ptr(), out.data_ptr(), pack.data_ptr()

    def call(dtype=1, g=p, co=32, w=p, d0=o, c0=3, d1=o + 4 * 2 * 3 * 256, c1=3, B=2, H=16, W=16, pk=k, n=nb):
        return L.llie_init_conv_dgrad(dtype, g, co, w, d0, c0, d1, c1, B, H, W, pk, n, _st())
    bad = [dict(dtype=3), dict(dtype=-1), dict(g=None), dict(w=None), dict(pk=None), dict(pk=k + 4), dict(n=nb - 16), dict(c0=0), dict(c1=-1),
           dict(c0=5, c1=4), dict(d0=None, d1=None), dict(c1=0), dict(H=12), dict(W=20), dict(B=0), dict(B=65536), dict(co=0), dict(co=-32),
           dict(co=48)]
    assert call(dtype=0) == 0  # the fp32 kernel's name must still stand after the refused calls, which ask for fp16
    torch.cuda.synchronize()
    before_name = _last()
    assert before_name == "init_conv_dgrad_kernel<float>"
    before = [b.clone() for b in (x, out, pack)]
    for kw in bad:
        assert call(**kw) == N.ERR_ARG, kw
    torch.cuda.synchronize()
    assert _last() == before_name, "a refused call launched a kernel"
    for a, b in zip(before, (x, out, pack)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "a refused call changed a buffer"
    x.zero_()
    assert call() == 0 and call(d1=None) == 0 and call(d0=None) == 0 and call(d1=None, c1=0) == 0
    torch.cuda.synchronize()
    assert _last() == "init_conv_dgrad_kernel<_Float16>"
    assert not torch.isnan(out[:2 * 6 * 256]).any()
