"""llie_guide / llie_guidance_pair / llie_cond_dropout (csrc/guidance.hip) against the NumPy fp32 twins of guidance.py, bit for bit.

The twins perform the kernel's IEEE fp32 operations one by one, so the comparison is on the bits (NaN payloads aside: a NaN must be
a NaN).  Shapes: batch 1 and 3; per_sample 1 and 7 (all tail), 1024 (exactly one workgroup of float4 items), 1025 (one past it: with
one row a float4 body and a scalar tail, with three rows every row unaligned) and 3 * 64 * 64 (the image of the other tests).
Every tensor lives between 0xA5 guard bytes in one allocation, at a 16-byte aligned offset or 4 bytes past one (the 16-byte path
must decline), outputs are prefilled with NaN, and every call is made twice."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
native = importlib.import_module("cv-diffusion-model_amd._native")

F = np.float32
GUARD = 256  # bytes of 0xA5 on either side
SHAPES = [(b, per) for b in (1, 3) for per in (1, 7, 1024, 1025, 3 * 64 * 64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """`n` floats between guard bytes; `shift` = 4 puts them 4 bytes past a 16-byte boundary.  Filled with `values` or NaN."""

    def __init__(self, dev, n, shift=0, values=None):
        self.raw = torch.full((2 * GUARD + 4 * n + 16,), 0xA5, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.first = GUARD + shift
        self.t = self.raw[self.first:self.first + 4 * n].view(torch.float32)
        assert self.t.data_ptr() % 16 == shift
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=F)).reshape(-1)) if values is not None else self.t.fill_(float("nan"))
        self.n = n

    @property
    def ptr(self):
        return self.t.data_ptr()

    def numpy(self):
        return self.t.cpu().numpy()

    def refill(self):
        self.t.fill_(float("nan"))

    def guards_intact(self):
        raw = self.raw.cpu().numpy()
        return bool((raw[:self.first] == 0xA5).all() and (raw[self.first + 4 * self.n:] == 0xA5).all())


def same_bits(got, want):
    got, want = np.asarray(got, dtype=F).reshape(-1), np.asarray(want, dtype=F).reshape(-1)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


def data(b, per, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((b, per)) * 3).astype(F)
    y = (rng.standard_normal((b, per)) * 3).astype(F)
    if per >= 7:  # values whose difference, product or sum rounds, overflows or is not a number
        x[0, :6] = [1e30, -1e30, np.inf, np.nan, 1.0, -0.0]
        y[0, :6] = [-1e30, 1e-30, np.inf, 1.0, 1.0 + 2.0 ** -23, 0.0]
    return x, y


# ------------------------------------------------------------------ llie_guide
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("b,per", SHAPES)
def test_guide(dev, b, per, shift):
    L = native.lib()
    c, u = data(b, per, 100 * b + per)
    gc, gu, go = Guarded(dev, b * per, shift, c), Guarded(dev, b * per, shift, u), Guarded(dev, b * per, shift)
    for w in (0.0, 1.0, 2.5, -1.0):
        want = M.guide_array(c, u, w)
        for _ in range(2):  # twice: the same bits
            go.refill()
            assert L.llie_guide(gc.ptr, gu.ptr, None, w, go.ptr, b, per, st()) == 0
            assert same_bits(go.numpy(), want), (b, per, shift, w)
    rows = np.array([3.0, -0.5, 12.25][:b], dtype=F)
    gw = Guarded(dev, b, 0, rows)
    want = M.guide_array(c, u, rows)
    for _ in range(2):
        go.refill()
        assert L.llie_guide(gc.ptr, gu.ptr, gw.ptr, float("nan"), go.ptr, b, per, st()) == 0  # the scalar is not used
        assert same_bits(go.numpy(), want)
    assert same_bits(gc.numpy(), c) and same_bits(gu.numpy(), u)  # inputs are read only
    # out aliases out_cond; then out_uncond
    assert L.llie_guide(gc.ptr, gu.ptr, None, 2.5, gc.ptr, b, per, st()) == 0
    assert same_bits(gc.numpy(), M.guide_array(c, u, 2.5)) and same_bits(gu.numpy(), u)
    gc.t.copy_(torch.from_numpy(c).reshape(-1))
    assert L.llie_guide(gc.ptr, gu.ptr, gw.ptr, 0.0, gu.ptr, b, per, st()) == 0
    assert same_bits(gu.numpy(), want) and same_bits(gc.numpy(), c)
    assert all(g.guards_intact() for g in (gc, gu, go, gw))


def test_guide_mixed_alignment(dev):
    """One unaligned pointer among aligned ones is enough to decline the 16-byte path; the bits do not change."""
    L = native.lib()
    b, per = 3, 1024
    c, u = data(b, per, 7)
    want = M.guide_array(c, u, 2.5)
    for shifts in ((4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 8, 12)):
        gc, gu, go = Guarded(dev, b * per, shifts[0], c), Guarded(dev, b * per, shifts[1], u), Guarded(dev, b * per, shifts[2])
        assert L.llie_guide(gc.ptr, gu.ptr, None, 2.5, go.ptr, b, per, st()) == 0
        assert same_bits(go.numpy(), want) and go.guards_intact(), shifts


# ------------------------------------------------------------------ llie_guidance_pair
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("b,per", SHAPES)
def test_guidance_pair(dev, b, per, shift):
    L = native.lib()
    lat, cond = data(b, per, 200 * b + per)
    want_lat, want_cond = M.guidance_pair_array(lat, cond)
    gl, gcnd = Guarded(dev, b * per, shift, lat), Guarded(dev, b * per, shift, cond)
    gl2, gc2 = Guarded(dev, 2 * b * per, shift), Guarded(dev, 2 * b * per, shift)
    for _ in range(2):
        gl2.refill(), gc2.refill()
        assert L.llie_guidance_pair(gl.ptr, gcnd.ptr, gl2.ptr, gc2.ptr, b, per, st()) == 0
        assert same_bits(gl2.numpy(), want_lat) and same_bits(gc2.numpy(), want_cond)
        assert np.array_equal(gc2.numpy()[b * per:].view(np.uint32), np.zeros(b * per, dtype=np.uint32))  # positive zeros
    assert same_bits(gl.numpy(), lat) and same_bits(gcnd.numpy(), cond)
    assert all(g.guards_intact() for g in (gl, gcnd, gl2, gc2))


# ------------------------------------------------------------------ llie_cond_dropout
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("b,per", SHAPES)
def test_cond_dropout(dev, b, per, shift):
    L = native.lib()
    x, _ = data(b, per, 300 * b + per)
    u = np.array([0.25, 0.5, 0.75][:b], dtype=F)  # at p = 0.5: dropped (with its inf / NaN), kept (u == p), kept
    gx, gu, go = Guarded(dev, b * per, shift, x), Guarded(dev, b, 0, u), Guarded(dev, b * per, shift)
    for p in (0.0, 0.5, 0.25, 1.0):
        want = M.cond_dropout_array(x, u, p)
        for _ in range(2):
            go.refill()
            assert L.llie_cond_dropout(gx.ptr, gu.ptr, p, go.ptr, b, per, st()) == 0
            got = go.numpy()
            assert same_bits(got, want), (b, per, shift, p)
    dropped = M.cond_dropout_array(x, u, 0.5)
    assert not dropped[0].any() and not np.isnan(dropped[0]).any()  # the row with inf / NaN came out as zeros
    assert same_bits(gx.numpy(), x)
    # in place, as the gradient mask uses it
    assert L.llie_cond_dropout(gx.ptr, gu.ptr, 0.5, gx.ptr, b, per, st()) == 0
    assert same_bits(gx.numpy(), dropped)
    assert all(g.guards_intact() for g in (gx, gu, go))


def test_device_wrappers(dev):
    """guide_device / guidance_pair_device / cond_dropout_device: the same kernels on tensors, with their shape checks."""
    c, u = data(3, 3 * 8 * 8, 9)
    ct, ut = torch.from_numpy(c).to(dev).view(3, 3, 8, 8), torch.from_numpy(u).to(dev).view(3, 3, 8, 8)
    assert same_bits(M.guide_device(ct, ut, 2.5).cpu().numpy(), M.guide_array(c, u, 2.5))
    rows = torch.tensor([1.0, 4.0, -2.0], device=dev)
    assert same_bits(M.guide_device(ct, ut, rows).cpu().numpy(), M.guide_array(c, u, rows.cpu().numpy()))
    lat2, cond2 = M.guidance_pair_device(ct, ut)
    assert same_bits(lat2.cpu().numpy(), np.concatenate([c, c])) and same_bits(cond2[:3].cpu().numpy(), u) and not cond2[3:].any()
    uu = torch.tensor([0.1, 0.9, 0.4], device=dev)
    assert same_bits(M.cond_dropout_device(ct, uu, 0.5).cpu().numpy(), M.cond_dropout_array(c, uu.cpu().numpy(), 0.5))
    with pytest.raises(ValueError):
        M.guide_device(ct, ut[:2], 2.0)
    with pytest.raises(ValueError):
        M.guide_device(ct, ut, float("nan"))
    with pytest.raises(ValueError):
        M.guide_device(ct, ut, rows[:2])
    with pytest.raises(ValueError):
        M.guide_device(ct.half(), ut.half(), 2.0)
    with pytest.raises(ValueError):
        M.cond_dropout_device(ct, uu, 1.5)
    with pytest.raises(ValueError):
        M.cond_dropout_device(ct, uu[:2], 0.5)


# ------------------------------------------------------------------ refusals: before any launch, outputs untouched
def test_refusals_leave_outputs_untouched(dev):
    L = native.lib()
    E = native.ERR_ARG
    b, per = 3, 1025
    c, u = data(b, per, 5)
    gc, gu, go, go2 = Guarded(dev, b * per, 0, c), Guarded(dev, b * per, 0, u), Guarded(dev, b * per), Guarded(dev, 2 * b * per)
    go2b = Guarded(dev, 2 * b * per)
    gw = Guarded(dev, b, 0, np.array([0.2, 0.5, 0.8], dtype=F))
    calls = [
        lambda: L.llie_guide(None, gu.ptr, None, 2.0, go.ptr, b, per, st()),
        lambda: L.llie_guide(gc.ptr, None, None, 2.0, go.ptr, b, per, st()),
        lambda: L.llie_guide(gc.ptr, gu.ptr, None, 2.0, None, b, per, st()),
        lambda: L.llie_guide(gc.ptr, gu.ptr, None, 2.0, go.ptr, 0, per, st()),
        lambda: L.llie_guide(gc.ptr, gu.ptr, None, 2.0, go.ptr, -3, per, st()),
        lambda: L.llie_guide(gc.ptr, gu.ptr, None, 2.0, go.ptr, b, 0, st()),
        lambda: L.llie_guide(gc.ptr, gu.ptr, None, 2.0, go.ptr, b, -1, st()),
        lambda: L.llie_guide(gc.ptr, gu.ptr, None, float("nan"), go.ptr, b, per, st()),
        lambda: L.llie_guide(gc.ptr, gu.ptr, None, float("inf"), go.ptr, b, per, st()),
        lambda: L.llie_guide(gc.ptr, gu.ptr, None, -float("inf"), go.ptr, b, per, st()),
        lambda: L.llie_guidance_pair(None, gu.ptr, go2.ptr, go2b.ptr, b, per, st()),
        lambda: L.llie_guidance_pair(gc.ptr, None, go2.ptr, go2b.ptr, b, per, st()),
        lambda: L.llie_guidance_pair(gc.ptr, gu.ptr, None, go2b.ptr, b, per, st()),
        lambda: L.llie_guidance_pair(gc.ptr, gu.ptr, go2.ptr, None, b, per, st()),
        lambda: L.llie_guidance_pair(gc.ptr, gu.ptr, go2.ptr, go2b.ptr, 0, per, st()),
        lambda: L.llie_guidance_pair(gc.ptr, gu.ptr, go2.ptr, go2b.ptr, b, 0, st()),
        lambda: L.llie_cond_dropout(None, gw.ptr, 0.5, go.ptr, b, per, st()),
        lambda: L.llie_cond_dropout(gc.ptr, None, 0.5, go.ptr, b, per, st()),
        lambda: L.llie_cond_dropout(gc.ptr, gw.ptr, 0.5, None, b, per, st()),
        lambda: L.llie_cond_dropout(gc.ptr, gw.ptr, 0.5, go.ptr, 0, per, st()),
        lambda: L.llie_cond_dropout(gc.ptr, gw.ptr, 0.5, go.ptr, b, 0, st()),
        lambda: L.llie_cond_dropout(gc.ptr, gw.ptr, -0.01, go.ptr, b, per, st()),
        lambda: L.llie_cond_dropout(gc.ptr, gw.ptr, 1.01, go.ptr, b, per, st()),
        lambda: L.llie_cond_dropout(gc.ptr, gw.ptr, float("nan"), go.ptr, b, per, st()),
        lambda: L.llie_cond_dropout(gc.ptr, gw.ptr, float("inf"), go.ptr, b, per, st()),
    ]
    for i, call in enumerate(calls):
        assert call() == E, i
    torch.cuda.synchronize()
    for g in (go, go2, go2b):
        assert np.isnan(g.numpy()).all() and g.guards_intact()  # still the NaN prefill: nothing was launched
    assert same_bits(gc.numpy(), c) and same_bits(gu.numpy(), u)
    with pytest.raises(ValueError):
        native.check(calls[7](), "guide")
