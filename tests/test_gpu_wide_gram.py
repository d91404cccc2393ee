"""The wide Gram form of the 192 -> 64 decoder block (knob "wide_gram"): norm2's tables from the Gram matrix of the activated block
input (gram.hip: gram_wide / gram_group_finalize), the expand GEMM that stores the ACTIVATED h1 and adds the SE pool totals itself
(pwx.hip: pw_expand_act) and dwconv3x3_project reading that tensor as it is (irbx.hip: PREACT).  The 384 -> 128 block does not
take the form (its Gram was not built), so there is one layer here: 128 + 64 -> 768 -> 64.

Maps: 8 x 16 (one 128-pixel tile: every 16-pixel run is on a border, the first row is also the last tile row), 16 x 32 and 24 x 48
(an interior, nine 128-pixel tiles per image: a ragged count for the Gram's workgroups).  B = 3, fp16 and bf16.

  * Gram: operands whose a' are multiples of 1/4 in [0, 1] with per-image, per-channel tables: G and m EQUAL the float64 reference;
    an image alone gives its row of the batch; a rerun gives the same bits.
  * group finalize: against a float64 evaluation of the same G (per channel, from the definition), a well- and an ill-conditioned
    case (|mean| >> sigma), and against what the slab path (pw_expand + gn_finalize) makes of the same input.  Bound: twice the
    slab path's own distance from float64, measured on these inputs in the same test.
  * activating expand: integer-exact operands give h1a and the pool totals of the float64 definition bit for bit, guards intact;
    on random operands h1a is at most as far from float64 as T(h1) activated afterwards (one rounding less).
  * pre-activated project: y and its slab equal dwconv3x3_project's on the stored h1 bit for bit when h1a is exactly the activation of
    that h1 (the two kernels then stage the same tile).
  * one block through the engine at knob 2 / 0, and small@64: PSNR, batch invariance, eager = capture = replay.
"""
import ctypes
import importlib
import math
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")
U = importlib.import_module("cv-diffusion-model_amd.unet")
oracle = importlib.import_module("oracle")

DTYPES = [(1, torch.float16), (2, torch.bfloat16)]
MAPS = [(8, 16), (16, 32), (24, 48)]
B, C0, C1, K, CHID, COUT, GROUPS = 3, 128, 64, 192, 768, 64, 32
CG = CHID // GROUPS
FIX = float(2 ** 24)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def block_map():
    L = N.lib()
    out = []
    for q in range(21):
        bi, bj = ctypes.c_int(), ctypes.c_int()
        N.check(L.llie_gram_wide_block(q, ctypes.byref(bi), ctypes.byref(bj)))
        out.append((bi.value, bj.value))
    return out


def full_gram(gblk):
    """[b][21 * 1024 + 192] as the kernels keep it -> (G [b][192][192], m [b][192]) float64"""
    g = gblk.double()
    G = torch.full((g.shape[0], K, K), float("nan"), dtype=torch.float64)
    for q, (bi, bj) in enumerate(block_map()):
        blk = g[:, q * 1024:(q + 1) * 1024].view(-1, 32, 32)
        G[:, 32 * bi:32 * bi + 32, 32 * bj:32 * bj + 32] = blk
        G[:, 32 * bj:32 * bj + 32, 32 * bi:32 * bi + 32] = blk.transpose(1, 2)
    assert torch.isfinite(G).all(), "the 21 blocks do not cover G"
    return G, g[:, 21 * 1024:]


def run_gram(dev, dtype, x, sc, sh, b0=0, b1=B):
    L = N.lib()
    nb, P = b1 - b0, x.shape[1]
    x0 = x[b0:b1, :, :C0].contiguous().to(dev)
    x1 = x[b0:b1, :, C0:].contiguous().to(dev)
    scd, shd = sc[b0:b1].contiguous().to(dev), sh[b0:b1].contiguous().to(dev)
    nf = int(L.llie_gram_wide_floats())
    part = R.Guarded((nb * int(L.llie_gram_wide_part_floats(P)),), dev)
    gblk = R.Guarded((nb, nf), dev)
    N.check(L.llie_gram_wide(dtype, x0.data_ptr(), C0, x1.data_ptr(), C1, scd.data_ptr(), shd.data_ptr(), nb, P, part.ptr, gblk.ptr, _st()), "gram_wide")
    torch.cuda.synchronize()
    part.cpu("partials")
    out = gblk.cpu("G")
    assert torch.isfinite(out).all(), "entries of G left unwritten"
    return out


# ------------------------------------------------------------------ 1. the wide Gram
@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
def test_gram_exact(dev, dtype, tdt, H, W):
    """x in {0, 1, 2, 4}, scale 1/4 or 1/2, shift 0 or 1/4 per (image, channel): a' is a multiple of 1/4 in [0, 1], every product a
    multiple of 1/16 and every sum below 2^11: fp32 is exact, so G and m equal float64."""
    P = H * W
    g = _gen("gram", H, W)
    x = torch.tensor([0.0, 1.0, 2.0, 4.0])[torch.randint(0, 4, (B, P, K), generator=g)].to(tdt)
    sc = torch.tensor([0.25, 0.5])[torch.randint(0, 2, (B, K), generator=g)]
    sh = torch.tensor([0.0, 0.25])[torch.randint(0, 2, (B, K), generator=g)]
    a = (x.double() * sc.double()[:, None, :] + sh.double()[:, None, :]).clamp(0, 1)
    Gref, mref = a.transpose(1, 2) @ a, a.sum(1)
    got = run_gram(dev, dtype, x, sc, sh)
    G, m = full_gram(got)
    assert torch.equal(G, Gref), f"G differs in {(G != Gref).sum().item()} entries"
    assert torch.equal(m, mref)
    assert torch.equal(got, run_gram(dev, dtype, x, sc, sh)), "a rerun gives other bits"
    for i in range(B):
        assert torch.equal(got[i:i + 1], run_gram(dev, dtype, x, sc, sh, i, i + 1)), i


# ------------------------------------------------------------------ 2. the group finalize
def tables_ref64(G, m, w6, gamma, beta, film, post, P):
    """norm2 + FiLM tables in float64 from the definition: per channel s1 = w_c . m, s2 = w_c^T G w_c (w = the T(6 W) rows), summed per
    group of CG channels"""
    s1 = m @ w6.t()                                            # [b][Chid]
    s2 = torch.einsum("ck,bkl,cl->bc", w6, G, w6)
    n = CG * P
    mean = s1.view(-1, GROUPS, CG).sum(2) / n
    var = (s2.view(-1, GROUPS, CG).sum(2) / n - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + 1e-5)
    mean, rstd = mean.repeat_interleave(CG, 1), rstd.repeat_interleave(CG, 1)
    sc = gamma.double() * rstd
    sh = beta.double() - mean * sc
    if film is not None:
        fs, fh = 1 + film[:, :CHID].double(), film[:, CHID:2 * CHID].double()
        sc, sh = sc * fs, sh * fs + fh
    return sc * post, sh * post


def finalize_inputs(kind, H, W, tdt):
    P = H * W
    g = _gen("fin", kind, H, W)
    if kind == "ill":  # a' close to 1/2 everywhere, weights close to one value: h1 is about 290 with a spread of a few units
        x = (0.5 + 0.05 * torch.randn(B, P, K, generator=g)).to(tdt)
        sc1, sh1 = torch.ones(B, K), torch.zeros(B, K)
        w32 = 0.5 + 0.01 * torch.randn(CHID, K, generator=g)
    else:
        x = torch.randn(B, P, K, generator=g).to(tdt)
        sc1, sh1 = (0.5 + torch.rand(B, K, generator=g)) / 6, (1.0 + 2.0 * torch.rand(B, K, generator=g)) / 6
        w32 = torch.randn(CHID, K, generator=g) / math.sqrt(K)
    gamma, beta = torch.rand(CHID, generator=g) + 0.5, 0.5 * torch.randn(CHID, generator=g)
    film = 0.3 * torch.randn(B, 2 * CHID, generator=g)
    return x, sc1, sh1, w32, gamma, beta, film


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("kind", ["random", "ill"])
def test_group_finalize_vs_float64_and_slab_path(dev, dtype, tdt, H, W, kind):
    """Tables of gram_group_finalize from the device's own G against float64 from the definition on that G, and against the
    tables the slab path (pw_expand's statistics of the ROUNDED h1, gn_finalize) produces on the same input.  Error measure: max
    |table - float64| over max |float64| per table.  The Gram route may be at most twice as far from float64 as the slab route
    (whose distance is mostly the rounding of h1 to T, which the Gram does not see); both are printed."""
    L = N.lib()
    P = H * W
    x, sc1, sh1, w32, gamma, beta, film = finalize_inputs(kind, H, W, tdt)
    post = 1.0 / 6.0
    gblk = run_gram(dev, dtype, x, sc1, sh1)
    G, m = full_gram(gblk)
    d = {k: v.to(dev) for k, v in dict(w32=w32, gamma=gamma, beta=beta, film=film, sc1=sc1, sh1=sh1).items()}
    # the slab path first: it packs the weights (T(6 W) in fragment order), which M_g is built from and the reference reads back
    x0, x1 = x[..., :C0].contiguous().to(dev), x[..., C0:].contiguous().to(dev)
    segs = (N.GemmSeg * 2)(N.GemmSeg(x0.data_ptr(), C0, d["sc1"].data_ptr(), d["sh1"].data_ptr(), K, 3),
                           N.GemmSeg(x1.data_ptr(), C1, d["sc1"].data_ptr() + 4 * C0, d["sh1"].data_ptr() + 4 * C0, K, 3))
    wpack = torch.empty(CHID * K, dtype=tdt, device=dev)
    h1 = torch.empty(B, P, CHID, dtype=tdt, device=dev)
    slab = torch.empty(B, P // 128, 2, CHID, device=dev)
    N.check(L.llie_pw_expand(dtype, segs, 2, d["w32"].data_ptr(), wpack.data_ptr(), h1.data_ptr(), slab.data_ptr(), B * P, CHID, P, _st()), "pw_expand")
    n_, k_ = torch.meshgrid(torch.arange(CHID), torch.arange(K), indexing="ij")
    pack_index = ((((n_ >> 5) * (K >> 4) + (k_ >> 4)) * 64 + (n_ & 31) + 32 * ((k_ >> 3) & 1)) << 3) + (k_ & 7)
    w6 = wpack.cpu().double()[pack_index]
    differ = (w6 != (w32 * 6.0).to(tdt).double()).sum().item()
    rsc, rsh = tables_ref64(G, m, w6, gamma, beta, film, post, P)
    mg = torch.full((GROUPS * int(L.llie_gram_wide_floats()),), float("nan"), dtype=torch.float64, device=dev)
    N.check(L.llie_gram_group_weights(dtype, wpack.data_ptr(), mg.data_ptr(), CHID, K, _st()), "gram_group_weights")
    runs, gd = [], gblk.to(dev)
    for _ in range(2):
        sc, sh = R.Guarded((B, CHID), dev), R.Guarded((B, CHID), dev)
        N.check(L.llie_gram_group_finalize(gd.data_ptr(), mg.data_ptr(), K, P, d["gamma"].data_ptr(), d["beta"].data_ptr(), d["film"].data_ptr(),
                                           2 * CHID, 1e-5, post, B, sc.ptr, sh.ptr, _st()), "gram_group_finalize")
        torch.cuda.synchronize()
        runs.append((sc.cpu("scale"), sh.cpu("shift")))
    assert torch.isfinite(mg).all()
    R._same(runs[0][0], runs[1][0], "scale")
    R._same(runs[0][1], runs[1][1], "shift")
    # the slab path's tables
    ssc, ssh = torch.empty(B, CHID, device=dev), torch.empty(B, CHID, device=dev)
    N.check(L.llie_groupnorm_finalize(slab.data_ptr(), P // 128, CHID, None, 0, 0, 32, P, d["gamma"].data_ptr(), d["beta"].data_ptr(), d["film"].data_ptr(),
                                      2 * CHID, 1e-5, post, B, ssc.data_ptr(), ssh.data_ptr(), _st()), "groupnorm_finalize")
    torch.cuda.synchronize()
    rel = lambda got, ref: ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    e_gram = max(rel(runs[0][0], rsc), rel(runs[0][1], rsh))
    e_slab = max(rel(ssc, rsc), rel(ssh, rsh))
    cond = ((rsh / post).abs().max() / (rsc / post).abs().max()).item()
    msg = (f"FINALIZE {kind} {H}x{W} {str(tdt)[6:]}: max rel |table - float64| gram {e_gram:.3e}, slab path {e_slab:.3e} (shift / scale {cond:.1f}; "
           f"packed weights that differ from torch's T(6 w): {differ})")
    print(msg)
    assert e_gram <= 2 * e_slab, msg


# ------------------------------------------------------------------ 3. the activating expand
def depthwise64(a, w9):
    return R.dw_from_padded(R.pad_zero(a), w9)[0]


def run_expand_act(dev, dtype, tdt, x, sc1, sh1, w32, sc2, sh2, wd, H, W, b0=0, b1=B):
    L = N.lib()
    nb, P = b1 - b0, H * W
    d = {k: v[b0:b1].contiguous().to(dev) for k, v in dict(sc1=sc1, sh1=sh1, sc2=sc2, sh2=sh2).items()}
    x0, x1 = x[b0:b1, :, :C0].contiguous().to(dev), x[b0:b1, :, C0:].contiguous().to(dev)
    segs = (N.GemmSeg * 2)(N.GemmSeg(x0.data_ptr(), C0, d["sc1"].data_ptr(), d["sh1"].data_ptr(), K, 3),
                           N.GemmSeg(x1.data_ptr(), C1, d["sc1"].data_ptr() + 4 * C0, d["sh1"].data_ptr() + 4 * C0, K, 3))
    w32d, wdd = w32.to(dev), wd.to(dev)
    wpack = torch.empty(CHID * K, dtype=tdt, device=dev)
    out = R.Guarded((nb, P, CHID), dev, tdt)
    tot = R.Guarded((nb, CHID), dev, torch.int64, fill=0)
    N.check(L.llie_pw_expand_act(dtype, segs, 2, w32d.data_ptr(), wpack.data_ptr(), d["sc2"].data_ptr(), d["sh2"].data_ptr(), wdd.data_ptr(), out.ptr,
                                 tot.ptr, nb * P, CHID, H, W, _st()), "pw_expand_act")
    torch.cuda.synchronize()
    o = out.cpu("h1a")
    assert torch.isfinite(o.float()).all(), "entries of h1a left unwritten"
    return o, tot.cpu("pool totals")


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
def test_expand_act_exact(dev, dtype, tdt, H, W):
    """a' in {0, 1}; rows of W hold eight entries of +-1/2 (6 w = +-3): h1 is an integer of at most 24; scale2 = 1/8, shift2 = 1/2
    or 1/4 per (image, channel): a = clamp01(.) is a multiple of 1/8; depthwise weights are multiples of 1/2 (6 w an integer).
    Everything is exact in fp32, so h1a equals T(a) and pool_tot equals 2^24 x the float64 total, bit for bit."""
    P = H * W
    g = _gen("actx", H, W)
    x = torch.randint(0, 2, (B, P, K), generator=g).to(tdt)
    sc1, sh1 = torch.ones(B, K), torch.zeros(B, K)
    w32 = torch.zeros(CHID, K)
    for r in range(CHID):
        w32[r, torch.randperm(K, generator=g)[:8]] = torch.randint(0, 2, (8,), generator=g).float() - 0.5
    sc2 = torch.full((B, CHID), 0.125)
    sh2 = torch.tensor([0.5, 0.25])[torch.randint(0, 2, (B, CHID), generator=g)]
    wd = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (9, CHID), generator=g)]
    h1 = x.double() @ (6 * w32.double()).t()
    a = (h1 * sc2.double()[:, None, :] + sh2.double()[:, None, :]).clamp(0, 1)
    assert torch.equal(a, a.to(tdt).double()) and 0 < a.mean() < 1
    tot_ref = depthwise64(a.view(B, H, W, CHID), 6 * wd.double()).sum((1, 2))
    got, tot = run_expand_act(dev, dtype, tdt, x, sc1, sh1, w32, sc2, sh2, wd, H, W)
    assert torch.equal(got.double(), a), f"h1a differs in {(got.double() != a).sum().item()} entries"
    bad = (tot != (tot_ref * FIX).to(torch.int64)).nonzero()
    assert bad.shape[0] == 0, f"{bad.shape[0]} totals differ; first (image, channel) {bad[:4].tolist()}"
    got2, tot2 = run_expand_act(dev, dtype, tdt, x, sc1, sh1, w32, sc2, sh2, wd, H, W)
    assert torch.equal(R._bits(got), R._bits(got2)) and torch.equal(tot, tot2)
    for i in range(B):
        gi, ti = run_expand_act(dev, dtype, tdt, x, sc1, sh1, w32, sc2, sh2, wd, H, W, i, i + 1)
        assert torch.equal(R._bits(got[i:i + 1]), R._bits(gi)) and torch.equal(tot[i:i + 1], ti), i


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
def test_expand_act_random(dev, dtype, tdt, H, W):
    """Random operands: max |h1a - float64| is at most that of T(h1) (pw_expand) activated afterwards with the project kernel's
    arithmetic (fp32 FMA, clamp, one rounding to T): the new form rounds once less.  The totals against float64 of the stored h1a, next
    to those dwconv3x3 leaves from that tensor."""
    L = N.lib()
    P = H * W
    x, sc1, sh1, w32, _, _, _ = finalize_inputs("random", H, W, tdt)
    g = _gen("actr", H, W)
    sc2, sh2 = (0.3 + 0.3 * torch.rand(B, CHID, generator=g)) / 6, (2.0 + 2.0 * torch.rand(B, CHID, generator=g)) / 6
    wd = 0.3 * torch.randn(9, CHID, generator=g)
    ap, _ = R.gemm_operand(dtype, x, 3, sc1, sh1)
    w6 = (w32 * 6.0).to(tdt).double()
    aref = (ap @ w6.t() * sc2.double()[:, None, :] + sh2.double()[:, None, :]).clamp(0, 1)
    got, tot = run_expand_act(dev, dtype, tdt, x, sc1, sh1, w32, sc2, sh2, wd, H, W)
    d = {k: v.to(dev) for k, v in dict(sc1=sc1, sh1=sh1, w32=w32).items()}
    x0, x1 = x[..., :C0].contiguous().to(dev), x[..., C0:].contiguous().to(dev)
    segs = (N.GemmSeg * 2)(N.GemmSeg(x0.data_ptr(), C0, d["sc1"].data_ptr(), d["sh1"].data_ptr(), K, 3),
                           N.GemmSeg(x1.data_ptr(), C1, d["sc1"].data_ptr() + 4 * C0, d["sh1"].data_ptr() + 4 * C0, K, 3))
    wpack = torch.empty(CHID * K, dtype=tdt, device=dev)
    h1 = torch.empty(B, P, CHID, dtype=tdt, device=dev)
    slab = torch.empty(B, P // 128, 2, CHID, device=dev)
    N.check(L.llie_pw_expand(dtype, segs, 2, d["w32"].data_ptr(), wpack.data_ptr(), h1.data_ptr(), slab.data_ptr(), B * P, CHID, P, _st()), "pw_expand")
    torch.cuda.synchronize()
    a_old = R._r64(R._f32(h1.cpu().double() * sc2.double()[:, None, :] + sh2.double()[:, None, :]).clamp(0, 1), dtype)
    e_new, e_old = (got.double() - aref).abs().max().item(), (a_old - aref).abs().max().item()
    msg = f"H1A_ERR {H}x{W} {str(tdt)[6:]}: max |a - float64| activating expand {e_new:.3e}, T(h1) activated afterwards {e_old:.3e}"
    print(msg)
    assert 0.05 < aref.mean().item() < 0.95 and e_new <= e_old, msg
    tot_ref = depthwise64(got.double().view(B, H, W, CHID), (6 * wd).to(tdt).double()).sum((1, 2))
    e_tot = (tot.double() / FIX - tot_ref).abs().max().item()
    # the rule of test_pool_totals_random (test_gpu_wide_project.py): at most twice as far from float64 as the totals dwconv3x3 leaves
    # on the same tensor -- here the stored h1a under the identity tables (clamp01(1 a + 0) = a), so both sum the same numbers
    hd, one, zero, wdd = got.to(dev), torch.ones(B, CHID, device=dev), torch.zeros(B, CHID, device=dev), wd.to(dev)
    h2, told = torch.empty_like(hd), torch.zeros(B, CHID, dtype=torch.int64, device=dev)
    N.check(L.llie_dwconv3x3_ex(dtype, hd.data_ptr(), h2.data_ptr(), one.data_ptr(), zero.data_ptr(), wdd.data_ptr(), None, told.data_ptr(), 1, B, H, W,
                                CHID, _st()), "dwconv3x3_ex")
    torch.cuda.synchronize()
    e_old_tot = (told.cpu().double() / FIX - tot_ref).abs().max().item()
    msg = (f"POOL_ERR {H}x{W} {str(tdt)[6:]}: max |total - float64 of the stored h1a| activating expand {e_tot:.3e}, dwconv3x3 {e_old_tot:.3e}, "
           f"|ref|max {tot_ref.abs().max().item():.3e}")
    print(msg)
    assert e_tot <= 2 * e_old_tot, msg


# ------------------------------------------------------------------ 4. the pre-activated project
def _round_once(z):
    """float64 -> fp32 rounded to odd, so that the conversion to fp16 that follows is the only rounding that counts"""
    f = z.float()
    bits = f.view(torch.int32)
    up = (f.double() < z) == (f >= 0)  # the neighbour towards z is the next larger bit pattern
    fix = (f.double() != z) & ((bits & 1) == 0)
    return torch.where(fix, bits + torch.where(up, 1, -1).to(torch.int32), bits).view(torch.float32)


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("kind", ["random", "exact"])
def test_project_preact_equals_project_on_the_stored_h1(dev, dtype, tdt, H, W, kind):
    """h1a := T(clamp01(fma(h1, s, b))), exactly what dwconv3x3_project parks in LDS from the stored h1: both kernels then run the
    same arithmetic: y and the slab are equal bit for bit on integer-exact operands and within one rounding of T on random ones (the
    count of differing entries is printed; with the activation emulated exactly it is expected to be 0)."""
    L = N.lib()
    g = _gen("pre", kind, H, W)
    if kind == "exact":
        h1 = torch.randint(-1, 3, (B, H, W, CHID), generator=g).to(tdt)
        sc, sh = torch.full((B, CHID), 2.0 ** 20), torch.full((B, CHID), -2.0 ** 19)
        wd = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (9, CHID), generator=g)]
        gate = torch.ones(B, CHID)
        xin = torch.randint(-1, 3, (B, H, W, K), generator=g).to(tdt)
        wps = torch.zeros(COUT, CHID + K)
        for r in range(COUT):
            wps[r, torch.randperm(CHID, generator=g)[:8]] = 2.0 * torch.randint(0, 2, (8,), generator=g) - 1.0
            wps[r, CHID + torch.randperm(K, generator=g)[:4]] = 2.0 * torch.randint(0, 2, (4,), generator=g) - 1.0
        wps = wps.to(tdt)
    else:
        h1 = (2.0 * torch.randn(B, H, W, CHID, generator=g)).to(tdt)
        sc, sh = (0.5 + torch.rand(B, CHID, generator=g)) / 6, (1.0 + 2.0 * torch.rand(B, CHID, generator=g)) / 6
        wd = 0.3 * torch.randn(9, CHID, generator=g)
        gate = torch.rand(B, CHID, generator=g)
        xin = torch.randn(B, H, W, K, generator=g).to(tdt)
        wps = (torch.randn(COUT, CHID + K, generator=g) / math.sqrt(CHID + K)).to(tdt)
    # fp16: v_fma_mix rounds the exact FMA once, to T; bf16: an fp32 FMA, then the rounding to T.  z is exact in float64 here
    z = (h1.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]).clamp(0, 1)
    h1a = _round_once(z).to(tdt) if dtype == 1 else R._rt(R._f32(z), dtype)
    d = {k: v.to(dev) for k, v in dict(h1=h1, h1a=h1a, sc=sc, sh=sh, wd=wd, gate=gate, wps=wps).items()}
    x0, x1 = xin[..., :C0].contiguous().to(dev), xin[..., C0:].contiguous().to(dev)
    nt = int(L.llie_irbx_project_tiles(H, W))
    outs = []
    for pre in (False, True, True):
        y, slab = R.Guarded((B, H, W, COUT), dev, tdt), R.Guarded((B, nt, 2, COUT), dev)
        if pre:
            N.check(L.llie_dwconv3x3_project_preact(dtype, d["h1a"].data_ptr(), d["wd"].data_ptr(), d["gate"].data_ptr(), x0.data_ptr(), C0, x1.data_ptr(), C1,
                                                    d["wps"].data_ptr(), CHID + K, COUT, y.ptr, slab.ptr, B, H, W, _st()), "project_preact")
        else:
            N.check(L.llie_dwconv3x3_project(dtype, d["h1"].data_ptr(), d["sc"].data_ptr(), d["sh"].data_ptr(), d["wd"].data_ptr(), d["gate"].data_ptr(),
                                             x0.data_ptr(), C0, x1.data_ptr(), C1, d["wps"].data_ptr(), CHID + K, COUT, y.ptr, slab.ptr, B, H, W, _st()), "project")
        torch.cuda.synchronize()
        outs.append((y.cpu("y"), slab.cpu("slab")))
    assert torch.isfinite(outs[1][0].float()).all() and torch.isfinite(outs[1][1]).all()
    ndiff = (R._bits(outs[0][0]) != R._bits(outs[1][0])).sum().item()
    print(f"PREACT {kind} {H}x{W} {str(tdt)[6:]}: y entries that differ from dwconv3x3_project on the stored h1: {ndiff}")
    if kind == "exact":
        assert ndiff == 0 and torch.equal(outs[0][1], outs[1][1])
    else:  # within one rounding of T; the slab holds fp32 sums of 128 such values and their squares
        ya, yb = outs[0][0].double(), outs[1][0].double()
        assert ((ya - yb).abs() <= R._ulp(ya, dtype)).all()
        assert torch.allclose(outs[0][1], outs[1][1], rtol=2.0 ** -6, atol=128 * R.EPS_T[dtype] * ya.abs().max().item())
    assert torch.equal(R._bits(outs[1][0]), R._bits(outs[2][0])) and torch.equal(outs[1][1], outs[2][1])


def test_launchers_refuse_other_shapes(dev):
    L = N.lib()
    assert L.llie_wide_gram_supported(1, 192, 128, 768, 512) and L.llie_wide_gram_supported(2, 192, 192, 768, 128)
    for a in ((0, 192, 128, 768, 512), (1, 384, 256, 1536, 512), (1, 192, 128, 768, 192), (1, 192, 100, 768, 512), (1, 96, 64, 384, 512)):
        assert not L.llie_wide_gram_supported(*a), a
    z = torch.zeros(4096, device=dev)
    out = torch.full((4096,), float("nan"), device=dev)
    assert L.llie_gram_wide(1, z.data_ptr(), 64, z.data_ptr(), 32, z.data_ptr(), z.data_ptr(), 1, 512, out.data_ptr(), out.data_ptr(), _st()) != 0
    assert L.llie_gram_wide(1, z.data_ptr(), 128, z.data_ptr(), 64, z.data_ptr(), z.data_ptr(), 1, 192, out.data_ptr(), out.data_ptr(), _st()) != 0
    seg = (N.GemmSeg * 1)(N.GemmSeg(z.data_ptr(), 384, z.data_ptr(), z.data_ptr(), 384, 3))
    assert L.llie_pw_expand_act(1, seg, 1, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), out.data_ptr(), out.data_ptr(), 128, 1536, 8, 16, _st()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"


# ------------------------------------------------------------------ 5. one block and the whole network
TDIM = 256


def block_forward(dev, dtype, knob, H, W, nb=3, only=None):
    L = N.lib()
    cfg = U._module_cfg(N.LLIE_IRB, K, COUT, TDIM, split=C0)
    cfg.compute_dtype = N.dtype_code(dtype)
    h = N.Handle(cfg)
    try:
        N.check(L.llie_tune(b"wide_gram", knob))
        g = torch.Generator().manual_seed(19264)
        params = [(0.1 * torch.randn(shape, generator=g)).to(dev) for _, shape in h.params()]
        h.load_all(params, _st())
        x = torch.randn(nb, K, H, W, generator=g).to(dev)
        temb = torch.randn(nb, TDIM, generator=g).to(dev)
        if only is not None:
            x, temb, nb = x[only:only + 1].contiguous(), temb[only:only + 1].contiguous(), 1
        y = torch.empty(nb, COUT, H, W, device=dev)
        nbytes = h.workspace_bytes(nb, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        h.profile_begin(31)
        N.check(L.llie_module_forward(h.h, x.data_ptr(), temb.data_ptr(), y.data_ptr(), nb, H, W, ws.data_ptr(), nbytes, _st()), "forward")
        torch.cuda.synchronize()
        rows = h.profile_dump()
        assert torch.isfinite(y).all()
        return y.cpu(), [name.split("<")[0] for cls, name, _tag, _ms, _b in rows if cls != N.K_SE]
    finally:
        L.llie_tune(b"wide_gram", 1)
        h.close()


@pytest.mark.parametrize("H,W", MAPS)
def test_block_through_the_engine(dev, H, W):
    """Knob 2 (the form at every map size): gn(norm1), the wide Gram, the group finalize, the activating expand, SE, the pre-activated
    project; knob 0 the parent's sequence; knob 1 takes the form from 4096 pixels per image on, so not at these maps.  Against the fp32
    engine on the same parameters (it stands in for float64, as in test_gpu_wide_project.py) the new sequence may err at most twice
    as much as the shipped wide form.  An image alone gives the bits of its row."""
    y2, seq2 = block_forward(dev, "fp16", 2, H, W)
    y0, seq0 = block_forward(dev, "fp16", 0, H, W)
    y1, seq1 = block_forward(dev, "fp16", 1, H, W)
    yr, _ = block_forward(dev, "fp32", 2, H, W)
    assert seq2 == ["gn_finalize_kernel", "gram_wide_kernel", "gram_group_finalize_kernel", "pw_expand_act_kernel", "dwconv3x3_project_kernel"], seq2
    assert seq0 == ["gn_finalize_kernel", "pw_expand_kernel", "gn_finalize_kernel", "dwconv3x3_pool_kernel", "dwconv3x3_project_kernel"], seq0
    assert seq1 == seq0 and torch.equal(y1, y0)
    e2, e0 = (y2 - yr).abs().max().item(), (y0 - yr).abs().max().item()
    msg = f"BLOCK_ERR {H}x{W} fp16: max |y - fp32 engine| wide Gram form {e2:.3e}, shipped wide form {e0:.3e}, |y|max {yr.abs().max().item():.3e}"
    print(msg)
    assert not torch.equal(y2, y0) and e2 <= 2 * e0, msg
    for i in range(3):
        assert torch.equal(y2[i:i + 1], block_forward(dev, "fp16", 2, H, W, only=i)[0]), i


def _psnr01(a, b):
    a = (torch.as_tensor(a).double().clamp(-1, 1) + 1) / 2
    b = (torch.as_tensor(b).double().clamp(-1, 1) + 1) / 2
    mse = ((a - b) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


def test_whole_network_properties(dev):
    """small@64 fp16 (the 192 -> 64 block sits at 32 x 32 there, so the knob is 2 against 0): different kernels ran, PSNR of
    `enhanced` above the house bar of 45 dB, each setting bitwise reproducible over the eager run, the capture and a replay, and
    an image alone gives its row of the batch."""
    spec = oracle.make_spec("small", 64)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    m = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4, compute_dtype="fp16")
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    L = N.lib()
    gen = torch.Generator().manual_seed(11)
    low = (torch.rand(3, 3, 64, 64, generator=gen) * 2 - 1).to(dev)
    noise = torch.randn(4, 3, 3, 64, 64, generator=gen).to(dev)
    try:
        outs = {}
        for v in (0, 2):
            N.check(L.llie_tune(b"wide_gram", v))
            runs = [m.enhance(low, 4, noise=noise).clone() for _ in range(3)]  # eager, capture, replay
            assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), v
            outs[v] = runs[0]
        assert not torch.equal(outs[0], outs[2])
        psnr = _psnr01(outs[0].cpu(), outs[2].cpu())
        print(f"small@64 fp16 enhanced: wide Gram form against the pool pass {psnr:.2f} dB")
        assert psnr > 45.0, psnr
        for i in range(3):
            one = m.enhance(low[i:i + 1], 4, noise=noise[:, i:i + 1]).clone()
            assert torch.equal(one, outs[2][i:i + 1]), i
    finally:
        N.check(L.llie_tune(b"wide_gram", 1))
