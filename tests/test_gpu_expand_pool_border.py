"""expand_pool's border bookkeeping (irbx.hip, expand_scan<POOL>): the scan classifies every 16-pixel group as interior or as
touching the first / last image row or column, and only edge groups enter the code that feeds the eight border sums.  The shapes
are chosen for that classification -- one, two, three and four column groups per image row, 32-pixel blocks that straddle two image
rows, workgroups that start in the middle of an image -- at all three widths and with two input segments, fp16 and bf16.

  * exact:  operands for which every intermediate value of the kernel is an integer, so that the totals equal the definition
            (depthwise 3x3 with zero padding, summed over the image) bit for bit; one pixel booked under a wrong border class
            changes the integer.  The construction itself is checked on the host, without a GPU.
  * random: the rule of test_gpu_expand_scan.test_expand_pool_totals at these shapes.
"""
import importlib

import pytest
import torch

from test_gpu_expand_dw_project import block_inputs, front64, run_pool

N = importlib.import_module("cv-diffusion-model_amd._native")

DTYPES = [(1, torch.float16), (2, torch.bfloat16)]
SHAPES = [(32, 8, 16, 2, 0),      # one column group: a group is both first and last column
          (32, 8, 32, 1, 0),      # two column groups: no interior group anywhere
          (32, 8, 64, 2, 0),      # blocks made of two interior groups in rows 1..6, edge blocks around them
          (32, 24, 48, 1, 0),     # three column groups: a block straddles two image rows and mixes an edge group with an
                                  # interior one; workgroups start in the middle of the image
          (64, 16, 32, 2, 0),     # second width
          (96, 16, 32, 2, 64)]    # third width, two input segments (64 + 32)
FIX = float(2 ** 24)              # fixed-point scale of the totals


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def exact_inputs(cin, H, W, B, tdt, seed):
    """Operands in the layout of block_inputs for which the kernel computes with integers only.
    x in {-1, 0, 1, 2} and both affines t -> 2^20 t - 2^19 (a scale of 2^20 around the threshold 1/2; norm2's shift is handed
    over undivided, so it is six times that): clamp01 sends every integer to 0 or 1, whatever the rounding of shift / 6.  With
    W1 in {-1, 0, 1} the accumulators are integers of at most Cin, a' = [acc >= 1], and the nine sums count pixels.  The
    depthwise weights are multiples of 1/2 without zero, so 6 w is one of -6, -3, 3, 6 in T and every tap counts."""
    g = torch.Generator().manual_seed(seed)
    chid = 4 * cin
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
    t = {}
    t["x"] = ri(-1, 2, B, H, W, cin).to(tdt)
    t["s1"] = torch.full((B, cin), 2.0 ** 20)
    t["b1"] = torch.full((B, cin), -2.0 ** 19)
    t["w1"] = ri(-1, 1, chid, cin).to(tdt)
    t["s2"] = torch.full((B, chid), 2.0 ** 20)
    t["b2"] = torch.full((B, chid), -6 * 2.0 ** 19)
    half = torch.tensor([-1.0, -0.5, 0.5, 1.0])
    t["wd"] = half[ri(0, 3, 9, chid)]
    return t


_exact = {}


def exact_case(cin, H, W, B, tdt):
    """operands and the float64 totals from the definition, computed once per (shape, dtype)"""
    key = (cin, H, W, B, tdt)
    if key not in _exact:
        t = exact_inputs(cin, H, W, B, tdt, 7 * cin + 3 * H + W)
        _exact[key] = (t, front64(t, tdt, round_weights=True).sum((2, 3)))     # [B][Chid]
    return _exact[key]


_random = {}


def random_case(cin, H, W, B, tdt):
    key = (cin, H, W, B, tdt)
    if key not in _random:
        t = block_inputs(cin, H, W, B, tdt, 500 * cin + 7 * H + W)
        _random[key] = (t, front64(t, tdt, round_weights=True).sum((2, 3)))
    return _random[key]


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,H,W,B,split", SHAPES)
def test_exact_operands_and_reference_on_the_host(tdt, cin, H, W, B, split):
    """No GPU.  What the exact test relies on: the operands survive the rounding to T, every accumulator is an integer, a' is 0
    or 1 with both values well represented, and the float64 reference from the definition (conv2d with zero padding, summed) is
    an integer below 2^24 that equals the nine-sum restatement (whole image minus a border row / column plus the corner they
    share, per tap) evaluated in int64 -- an independent route to the same number."""
    t, ref = exact_case(cin, H, W, B, tdt)
    for k in ("x", "w1"):
        assert torch.equal(t[k].double(), t[k].double().round())
    w6 = (6 * t["wd"]).to(tdt).double()
    assert torch.equal(w6, 6 * t["wd"].double()) and torch.equal(w6, w6.round()) and (w6 != 0).all()
    ap = (t["x"].double() * t["s1"].double()[:, None, None, :] + t["b1"].double()[:, None, None, :]).clamp(0, 1)
    assert torch.equal(ap, (t["x"].double() >= 1).double())
    acc = ap @ t["w1"].double().t()
    assert torch.equal(acc, acc.round())
    # fp32, as the kernel applies norm2: the shift is divided by six with a rounded 1/6
    sh = (t["b2"] * torch.tensor(1.0 / 6.0, dtype=torch.float32))[:, None, None, :]
    a32 = torch.addcmul(sh, acc.float(), t["s2"][:, None, None, :]).clamp(0, 1)
    a = (acc >= 1).to(torch.int64)                                               # [B][H][W][Chid]
    assert torch.equal(a32.double(), a.double())
    assert 0.2 < a.double().mean().item() < 0.8
    S = a.sum((1, 2))
    r0, rh, c0, cw = a[:, 0].sum(1), a[:, -1].sum(1), a[:, :, 0].sum(1), a[:, :, -1].sum(1)
    k00, k0w, kh0, khw = a[:, 0, 0], a[:, 0, -1], a[:, -1, 0], a[:, -1, -1]
    tot = torch.zeros_like(S)
    for tap in range(9):     # tap (ky, kx) reads pixel p + (ky - 1, kx - 1): p itself must leave the far border out
        ky, kx = divmod(tap, 3)
        st = S.clone()
        st -= r0 if ky == 2 else 0
        st -= rh if ky == 0 else 0
        st -= c0 if kx == 2 else 0
        st -= cw if kx == 0 else 0
        st += {(2, 2): k00, (2, 0): k0w, (0, 2): kh0, (0, 0): khw}.get((ky, kx), 0)
        tot += w6[tap].to(torch.int64)[None, :] * st
    assert torch.equal(ref, ref.round()) and ref.abs().max().item() < 2 ** 24
    assert torch.equal(ref.to(torch.int64), tot)
    assert (tot != 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("cin,H,W,B,split", SHAPES)
def test_expand_pool_border_classes_exact(dev, dtype, tdt, cin, H, W, B, split):
    """a' in {0, 1}, integer weights: every fp32 operation of the kernel is exact, so pool_tot / 2^24 must EQUAL the float64 total
    of the definition.  Two runs are bit-equal and an image alone gives its row of the batch."""
    L = N.lib()
    t, ref = exact_case(cin, H, W, B, tdt)
    got = run_pool(L, dtype, t, dev, split)
    exp = (ref * FIX).to(torch.int64)
    bad = (got != exp).nonzero()
    msg = f"{bad.shape[0]} of {exp.numel()} totals differ; first (image, channel) {bad[:4].tolist()}, " \
          f"got / 2^24 {[got[i, c].item() / FIX for i, c in bad[:4].tolist()]}, expected {[ref[i, c].item() for i, c in bad[:4].tolist()]}"
    print(f"|total|max {ref.abs().max().item():.0f}, totals that differ: {bad.shape[0]}")
    assert bad.shape[0] == 0, msg
    assert torch.equal(got, run_pool(L, dtype, t, dev, split))
    for i in range(B if B > 1 else 0):
        assert torch.equal(got[i:i + 1], run_pool(L, dtype, t, dev, split, i, i + 1)), i


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("cin,H,W,B,split", SHAPES)
def test_expand_pool_border_classes_random(dev, dtype, tdt, cin, H, W, B, split):
    """The rule of test_expand_pool_totals: the totals are at most twice as far from the float64 restatement as expand_dw's own on
    the same inputs (same rounding points, another summation order), two runs are bit-equal, and an image alone gives the bits of
    its row in the batch."""
    L = N.lib()
    t, ref = random_case(cin, H, W, B, tdt)
    new = run_pool(L, dtype, t, dev, split)
    old = run_pool(L, dtype, t, dev, split, project=False)
    err_new = (new.double() / FIX - ref).abs().max().item()
    err_old = (old.double() / FIX - ref).abs().max().item()
    msg = f"max |total - float64|: expand_pool {err_new:.3e}, expand_dw {err_old:.3e}, |ref|max {ref.abs().max().item():.3e}"
    print(msg)
    assert err_new <= 2 * err_old, msg
    assert torch.equal(new, run_pool(L, dtype, t, dev, split))
    for i in range(B if B > 1 else 0):
        assert torch.equal(new[i:i + 1], run_pool(L, dtype, t, dev, split, i, i + 1)), i
