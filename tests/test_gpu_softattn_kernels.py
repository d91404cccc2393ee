"""The fused softmax-attention kernels (csrc/softattn.hip) through llie_softattn / llie_softattn_backward against the float64
restatement of tests/softattn_refs.py, in every dtype.

Method (tests/test_gpu_forward_kernels.py, tests/test_gpu_backward_kernels.py): inputs are drawn in fp32 with a seeded generator
and rounded to T; an entry passes when |out - ref| - slack < BAR * 2^-24 * abssum (softattn_refs.py says which terms abssum and
slack hold; the BAR_* constants stand there with the measured worst ratios).  Outputs are prefilled with NaN and no entry is
excluded; out, lse and dqkv carry one extra entry that must stay NaN, between canaries; every call is made twice and must give
the same bits; llie_last_kernel() must name the kernel and its template argument; a batch of three must give the bits of its
images run alone.

Shapes: N = 1 / 25 (under one block), 64 (exactly one), 72 / 81 (ragged second block; second half-block absent or one key),
200 (two query tiles and four key blocks, both tails ragged: 128 + 72 and 3 x 64 + 8), 1024 (the bottleneck of small@256);
heads 1 / 4 / 8, B 1 / 3.  Families: softattn_refs.make_qkv.

LLIE_SOFTATTN_TEST_SEED (default 0) shifts every seed: the bars were measured over seeds 0, 1 and 2.
"""
import importlib
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softattn_refs as S  # noqa: E402
from kernel_refs import TDT, Guarded, _ratio, _rt, _same  # noqa: E402

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

SEED0 = int(os.environ.get("LLIE_SOFTATTN_TEST_SEED", "0"))
TNAME = {0: "float", 1: "_Float16", 2: "__bf16"}
# (N, heads, B, family)
CASES = [(1, 1, 1, "gauss"), (25, 4, 3, "gauss"), (64, 1, 1, "rising"), (64, 8, 3, "hot"), (72, 8, 1, "falling"), (72, 1, 3, "gauss"),
         (81, 4, 3, "hot"), (81, 1, 1, "rising"), (200, 4, 3, "gauss"), (200, 1, 1, "rising"), (200, 8, 1, "hot"),
         (200, 4, 1, "falling"), (1024, 1, 1, "gauss"), (1024, 1, 1, "rising"), (1024, 1, 1, "hot")]
PARAMS = [(n, h, b, f, d) for n, h, b, f in CASES for d in (0, 1, 2)]
IDS = [f"n{n}-h{h}-b{b}-{f}-dt{d}" for n, h, b, f, d in PARAMS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 1000003 + 7919 * SEED0)


def _last():
    return N.lib().llie_last_kernel().decode()


def _tail_untouched(t, n, what):
    assert torch.isnan(t.reshape(-1)[n:].float()).all(), f"{what}: written past its last entry"
    return t.reshape(-1)[:n]


def run_forward(dev, qkv, heads, dtype, want_lse=True):
    """-> (out [B][N][inner] of T, lse [B][heads][N] or None) on the CPU, guards checked"""
    B, n, _ = qkv.shape
    inner = 32 * heads
    qd = qkv.to(dev)
    out = Guarded((B * n + 1, inner), dev, TDT[dtype])
    lse = Guarded((B * heads * n + 1,), dev) if want_lse else None
    N.check(N.lib().llie_softattn(dtype, qd.data_ptr(), out.ptr, lse.ptr if lse else None, B, n, heads, _st()), "softattn")
    assert _last() == f"softattn_fwd_kernel<{TNAME[dtype]}>"
    torch.cuda.synchronize()
    o = _tail_untouched(out.cpu("softattn out"), B * n * inner, "out").view(B, n, inner)
    ls = _tail_untouched(lse.cpu("softattn lse"), B * heads * n, "lse").view(B, heads, n) if lse else None
    return o, ls


def run_backward(dev, qkv, out, dout, lse, heads, dtype):
    B, n, _ = qkv.shape
    L = N.lib()
    nf = int(L.llie_softattn_bwd_floats(B, n, heads))
    assert nf == B * heads * n
    ins = [t.to(dev) for t in (qkv, out, dout, lse)]
    dqkv = Guarded((B * n + 1, 96 * heads), dev, TDT[dtype])
    scr = Guarded((nf,), dev)
    N.check(L.llie_softattn_backward(dtype, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), dqkv.ptr, scr.ptr,
                                     nf, B, n, heads, _st()), "softattn_backward")
    assert _last() == f"softattn_bwd_kv_kernel<{TNAME[dtype]}>"
    torch.cuda.synchronize()
    scr.cpu("softattn_backward scratch")
    return _tail_untouched(dqkv.cpu("softattn dqkv"), B * n * 96 * heads, "dqkv").view(B, n, 96 * heads)


def forward_ratios(dev, n, heads, B, family, dtype, bars=True):
    qkv = S.make_qkv(family, B, n, heads, dtype, _gen("softattn", n, heads, B, family, dtype))
    a, b = run_forward(dev, qkv, heads, dtype), run_forward(dev, qkv, heads, dtype)
    _same(a[0], b[0], "out")
    _same(a[1], b[1], "lse")
    nolse, none = run_forward(dev, qkv, heads, dtype, want_lse=False)   # inference: no lse pointer, same out
    assert none is None
    _same(a[0], nolse, "out without lse")
    if B > 1:   # an image's bits do not depend on the batch it is in
        for i in range(B):
            o1, l1 = run_forward(dev, qkv[i:i + 1].contiguous(), heads, dtype)
            _same(a[0][i:i + 1], o1, f"image {i} alone")
            _same(a[1][i:i + 1], l1, f"lse of image {i} alone")
    r = S.softattn_ref(qkv, heads, dtype)
    tag = f"n{n}/h{heads}/b{B}/{family}/dt{dtype}"
    return (_ratio(a[0], r["out"], r["out_abssum"], r["out_slack"], S.BAR_SOFTATTN_OUT if bars else None, f"softattn_out/{tag}"),
            _ratio(a[1], r["lse"], r["lse_abssum"], r["lse_slack"], S.BAR_SOFTATTN_LSE if bars else None, f"softattn_lse/{tag}"))


def backward_ratio(dev, n, heads, B, family, dtype, bars=True):
    g = _gen("softattn_bwd", n, heads, B, family, dtype)
    qkv = S.make_qkv(family, B, n, heads, dtype, g)
    dout = _rt(torch.randn(B, n, 32 * heads, generator=g), dtype)
    r = S.softattn_ref(qkv, heads, dtype)
    out, lse = _rt(r["out"], dtype), r["lse"].float()   # what a forward pass would have stored
    a, b = (run_backward(dev, qkv, out, dout, lse, heads, dtype) for _ in range(2))
    _same(a, b, "dqkv")
    if B > 1:
        for i in range(B):
            s = slice(i, i + 1)
            one = run_backward(dev, qkv[s].contiguous(), out[s].contiguous(), dout[s].contiguous(), lse[s].contiguous(), heads, dtype)
            _same(a[s], one, f"dqkv of image {i} alone")
    ref = S.softattn_bwd_ref(qkv, out, dout, lse, heads, dtype)
    return _ratio(a, ref["dqkv"], ref["abssum"], ref["slack"], S.BAR_SOFTATTN_DQKV if bars else None,
                  f"softattn_dqkv/n{n}/h{heads}/b{B}/{family}/dt{dtype}")


@pytest.mark.parametrize("n,heads,B,family,dtype", PARAMS, ids=IDS)
def test_softattn_forward_vs_float64(dev, n, heads, B, family, dtype):
    """out and lse per entry (bars and measured ratios: softattn_refs.py), twice with equal bits, with and without lse, batch rows
    equal to the images alone, nothing written past the last query."""
    forward_ratios(dev, n, heads, B, family, dtype)


@pytest.mark.parametrize("n,heads,B,family,dtype", PARAMS, ids=IDS)
def test_softattn_backward_vs_float64(dev, n, heads, B, family, dtype):
    """dq | dk | dv per entry given out (T) and lse (fp32) as a forward pass stores them; same checks as the forward test."""
    backward_ratio(dev, n, heads, B, family, dtype)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_forward_then_backward_on_the_kernels_own_outputs(dev, dtype):
    """The pair as training runs it: the backward kernels fed the forward kernel's own out and lse (N = 200, heads 4, B = 2)."""
    g = _gen("softattn_pair", dtype)
    qkv = S.make_qkv("gauss", 2, 200, 4, dtype, g)
    dout = _rt(torch.randn(2, 200, 128, generator=g), dtype)
    out, lse = run_forward(dev, qkv, 4, dtype)
    dq = run_backward(dev, qkv, out, dout, lse, 4, dtype)
    ref = S.softattn_bwd_ref(qkv, out, dout, lse, 4, dtype)
    _ratio(dq, ref["dqkv"], ref["abssum"], ref["slack"], S.BAR_SOFTATTN_DQKV, f"softattn_pair/dt{dtype}")
