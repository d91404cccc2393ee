"""Each forward kernel that has a C ABI entry point, per launch path, against the plain float64 references of tests/kernel_refs.py.

Method (as tests/test_gpu_backward_kernels.py): inputs are drawn in fp32 with a seeded generator and rounded to the storage type;
the reference mirrors the kernel's roundings and nothing else; an entry passes when |out - ref| - slack < BAR * 2^-24 * abssum
(kernel_refs._ratio; the BAR_* constants stand in kernel_refs.py with the measured worst ratios beside them, which each test's
docstring repeats).  Every output is prefilled with NaN, so every entry is compared; every buffer a kernel writes part of (outputs,
statistics slabs and scratch sized by the *_tiles / *_splits helpers) sits between canaries; every call is made twice and must
give the same bits.  Where a launcher records a name, llie_last_kernel() must name the expected kernel and template arguments.
tests/test_forward_refs_host.py checks, without a GPU, that the references agree with torch's own float64 operators and that
these bars reject subtly wrong kernels.

LLIE_FWD_TEST_SEED (default 0) shifts every seed: the bars were measured over seeds 0, 1 and 2.
"""
import importlib
import math
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402
from kernel_refs import NAN, TDT, Guarded, _ratio, _rt, _same, _slab, _split, _ulp  # noqa: E402

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

SEED0 = int(os.environ.get("LLIE_FWD_TEST_SEED", "0"))
DTYPES = [0, 1, 2]
TNAME = {0: "float", 1: "_Float16", 2: "__bf16"}


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


def _ptr(t):
    return t.data_ptr() if t is not None else None


# =============================================================================================
# llie_pw_gemm: every template configuration launch_t (gemm.hip) selects
# segs: (channels, act, affine) with affine 0 = no table, 1 = scale only, 2 = scale and shift, 3 = both with affine_ld > channels
class GemmCase:
    def __init__(self, path, cfg, segs, n, p, dts=DTYPES, B=3):
        self.path, self.cfg, self.segs, self.n, self.p, self.dts, self.B = path, cfg, segs, n, p, dts, B
        self.name = f"{path}-k{'_'.join(str(s[0]) for s in segs)}-n{n}-p{p}"


H2 = [1, 2]
GEMM_CASES = [
    GemmCase("bk128", "128, 128, 2, 2, 128", [(128, 1, 2)], 128, 128, H2),
    GemmCase("bk128", "128, 128, 2, 2, 128", [(128, 3, 2), (128, 3, 3)], 128, 128, H2),
    GemmCase("bk64", "128, 128, 2, 2, 64", [(64, 0, 1)], 128, 128, H2),
    GemmCase("bk64", "128, 64, 2, 2, 64", [(64, 1, 3)], 64, 128, H2),
    GemmCase("bk64", "128, 32, 4, 1, 64", [(64, 0, 0), (128, 1, 2)], 32, 128, H2),
    GemmCase("bk64", "128, 128, 2, 2, 64", [(64, 0, 2), (128, 0, 0)], 128, 128, H2),
    GemmCase("ktail", "128, 128, 2, 2, 64", [(96, 1, 2)], 128, 128, H2),
    GemmCase("ktail", "128, 64, 2, 2, 64", [(32, 0, 0), (64, 1, 3)], 64, 256, H2),
    GemmCase("ktail", "128, 32, 4, 1, 64", [(160, 3, 2), (32, 3, 2), (96, 3, 3)], 96, 128, H2),
    GemmCase("ktail", "128, 64, 2, 2, 64", [(96, 0, 1)], 64, 256, H2),
    GemmCase("bk32", "128, 128, 2, 2, 32", [(32, 1, 2)], 128, 128, H2),
    GemmCase("bk32", "128, 64, 2, 2, 32", [(32, 0, 0), (32, 0, 1)], 64, 128, H2),
    GemmCase("bk32", "128, 32, 4, 1, 32", [(32, 3, 3)], 32, 128, H2),
    GemmCase("bk32f", "128, 128, 2, 2, 32", [(32, 1, 2), (64, 0, 0)], 128, 128, [0]),
    GemmCase("bk32f", "128, 64, 2, 2, 32", [(32, 0, 1), (64, 1, 3)], 64, 128, [0]),
    GemmCase("bk32f", "128, 32, 4, 1, 32", [(32, 0, 2), (64, 0, 3)], 32, 128, [0]),
    GemmCase("bm64", "64, 128, 2, 2, 32", [(64, 1, 2)], 128, 64),
    GemmCase("bm64", "64, 64, 2, 2, 32", [(96, 0, 1)], 64, 192),
    GemmCase("bm64", "64, 32, 2, 1, 32", [(32, 0, 0), (32, 1, 3)], 32, 64),
    GemmCase("bm64", "64, 128, 2, 2, 32", [(128, 0, 2)], 128, 192),
    GemmCase("ragged", "64, 128, 2, 2, 32", [(64, 1, 3)], 128, 25),
    GemmCase("ragged", "64, 64, 2, 2, 32", [(96, 0, 0)], 64, 81),
    GemmCase("ragged", "64, 32, 2, 1, 32", [(32, 0, 1), (64, 1, 2)], 32, 100),
    GemmCase("ragged", "64, 128, 2, 2, 32", [(128, 1, 2), (128, 0, 2)], 128, 324),
]
GEMM_PARAMS = [(c, d, full) for c in GEMM_CASES for d in c.dts for full in (True, False)]


def _gemm_inputs(segs, n, P, B, dtype, key):
    g = _gen("gemm", key, dtype)
    xs, tabs, lds = [], [], []
    for ch, act, aff in segs:
        xs.append(_rt(torch.randn(B, P, ch, generator=g) * 1.5, dtype))
        ld = ch + 24 if aff == 3 else ch
        div = 6.0 if act == 3 else 1.0
        sc = (torch.rand(B, ld, generator=g) + 0.5) / div if aff else None
        sh = (torch.randn(B, ld, generator=g) * 0.7 + (1.0 if act else 0.0)) / div if aff >= 2 else None
        tabs.append((sc, sh))
        lds.append(ld)
    K = sum(s[0] for s in segs)
    w = _rt(torch.randn(n, K, generator=g) / math.sqrt(K), dtype)
    bias = torch.randn(n, generator=g) * 0.3
    res = _rt(torch.randn(B, P, n, generator=g), dtype)
    return xs, tabs, lds, w, bias, res


def _gemm_call(dev, dtype, segs, xd, tabd, lds, wd, bd, rd, n, P, B, stats):
    L = N.lib()
    arr = (N.GemmSeg * len(segs))()
    for i, ((ch, act, aff), x, (sc, sh)) in enumerate(zip(segs, xd, tabd)):
        arr[i] = N.GemmSeg(x.data_ptr(), ch, _ptr(sc), _ptr(sh), lds[i] if aff else 0, act)
    out = Guarded((B, P, n), dev, TDT[dtype])
    rows = int(L.llie_pw_gemm_tile_rows(P))
    nt = (P + rows - 1) // rows
    slab = _slab(dev, B, nt, 2, n) if stats else None
    rc = L.llie_pw_gemm(dtype, arr, len(segs), wd.data_ptr(), _ptr(bd), _ptr(rd), out.ptr, slab.ptr if stats else None, B * P, n, P, _st())
    torch.cuda.synchronize()
    return rc, out, slab, rows, nt


def _gemm_check(case_name, dtype, segs, xs, tabs, w, bias, res, o, slab, rows, nt):
    acts = [s[1] for s in segs]
    cut = [(sc[:, :ch] if sc is not None else None, sh[:, :ch] if sh is not None else None) for (ch, _, _), (sc, sh) in zip(segs, tabs)]
    ref, ab, sl = R.pw_gemm_ref(dtype, xs, acts, cut, w, bias, res)
    _ratio(o, ref, ab, sl, R.BAR_GEMM, f"gemm/{case_name}/dt{dtype}")
    if slab is not None:
        sref, sab, ssl = R.tile_stats_ref(o, rows)
        _ratio(slab, sref, sab, ssl, R.BAR_GEMM_STATS, f"gemm_stats/{case_name}/dt{dtype}")


@pytest.mark.parametrize("case,dtype,full", GEMM_PARAMS, ids=[f"{c.name}-dt{d}-{'full' if f else 'bare'}" for c, d, f in GEMM_PARAMS])
def test_pw_gemm_vs_float64(dev, case, dtype, full):
    """llie_pw_gemm in each configuration of launch_t: BK 128 / 64 / KTAIL / 32 at 128-row tiles, the 64-row tiles (P = 64, 192) and
    the ragged ones (P = 25, 81, 100, 324), BN 128 / 64 / 32, 1-3 segments; once with bias, residual and statistics, once bare.
    Over the cases of a dtype: act 0, 1 and (2-byte) 3; segments without a table, with scale only, with scale and shift, and with
    affine_ld wider than the segment.  (Act 2, SiLU, is refused: test_pw_gemm_refusals.)  The statistics slab is checked entry by
    entry against the sums of the values the kernel stored, which are themselves checked against the reference.
    Measured worst ratio (MI355X, seeds 0..2), output: 5.00 fp32, 0.29 fp16, 0.10 bf16, bar BAR_GEMM = 50; statistics: 1.78 / 1.24 /
    0.96, bar BAR_GEMM_STATS = 18."""
    c = case
    xs, tabs, lds, w, bias, res = _gemm_inputs(c.segs, c.n, c.p, c.B, dtype, c.name)
    d = lambda t: t.to(dev) if t is not None else None  # noqa: E731
    xd, tabd, wd = [d(x) for x in xs], [(d(a), d(b)) for a, b in tabs], d(w)
    bd, rd = (d(bias), d(res)) if full else (None, None)
    runs = []
    for _ in range(2):
        rc, out, slab, rows, nt = _gemm_call(dev, dtype, c.segs, xd, tabd, lds, wd, bd, rd, c.n, c.p, c.B, full)
        N.check(rc, "pw_gemm")
        assert _last() == f"pw_gemm_kernel<{TNAME[dtype]}, {c.cfg}>", _last()
        runs.append((out.cpu("gemm out"), _split(slab.cpu("gemm stats"), c.B, nt, "gemm stats") if full else None))
    _same(runs[0][0], runs[1][0], "out")
    if full:
        _same(runs[0][1], runs[1][1], "stats")
    _gemm_check(c.name + ("/full" if full else "/bare"), dtype, c.segs, xs, tabs, w, bias if full else None, res if full else None,
                runs[0][0], runs[0][1], rows, nt)


@pytest.mark.parametrize("dtype", H2)
def test_pw_gemm_chunk_width_threshold_same_bits(dev, dtype):
    """K = 128, N = 512, P = 128: B = 3 is 12 workgroups (128-wide K chunks), B = 257 is 1028 > kBk128MaxGrid (64-wide).  The
    launcher's claim: the same sequence of 32-wide k-steps, so the same bits.  The large batch repeats three distinct images;
    images 0..2 equal the small launch bit for bit and are checked against the reference, every other image equals its twin."""
    segs, n, P, B = [(128, 1, 2)], 512, 128, 257
    xs, tabs, lds, w, bias, res = _gemm_inputs(segs, n, P, 3, dtype, "threshold")
    idx = torch.arange(B) % 3
    d = lambda t: t.to(dev)  # noqa: E731
    big = lambda t: t[idx].contiguous().to(dev)  # noqa: E731
    rc, o3, s3, rows, nt = _gemm_call(dev, dtype, segs, [d(xs[0])], [(d(tabs[0][0]), d(tabs[0][1]))], lds, d(w), d(bias), d(res), n, P, 3, True)
    N.check(rc, "pw_gemm")
    assert _last() == f"pw_gemm_kernel<{TNAME[dtype]}, 128, 128, 2, 2, 128>", _last()
    rc, ob, sb, _, _ = _gemm_call(dev, dtype, segs, [big(xs[0])], [(big(tabs[0][0]), big(tabs[0][1]))], lds, d(w), d(bias), big(res), n, P, B, True)
    N.check(rc, "pw_gemm")
    assert _last() == f"pw_gemm_kernel<{TNAME[dtype]}, 128, 128, 2, 2, 64>", _last()
    o3c, s3c = o3.cpu(), _split(s3.cpu(), 3, nt, "gemm stats")
    obc, sbc = ob.cpu("gemm out"), _split(sb.cpu("gemm stats"), B, nt, "gemm stats")
    _same(obc[:3], o3c, "B = 257 vs B = 3 (out)")
    _same(sbc[:3], s3c, "B = 257 vs B = 3 (stats)")
    _same(obc, obc[idx], "an image and its twin (out)")
    _same(sbc, sbc[idx], "an image and its twin (stats)")
    _gemm_check("threshold", dtype, segs, xs, tabs, w, bias, res, obc[:3], sbc[:3], rows, nt)


def test_pw_gemm_refusals(dev):
    """Out-of-contract calls are refused and nothing is launched (the NaN-filled output stays NaN): N or a segment not a multiple
    of 32, M % P != 0, act 3 on some segments only, act 3 in fp32, SiLU (act 2: the forward GEMM has no such prologue and used to
    compute it as no activation), an activation or a shift without a scale table, affine_ld < channels."""
    L = N.lib()
    T = torch.float16
    x = torch.zeros(256, 128, dtype=T, device=dev)
    x32 = torch.zeros(256, 128, device=dev)
    t = torch.zeros(2, 128, device=dev)
    w = torch.zeros(128 * 256, dtype=torch.float32, device=dev)
    out = torch.full((256 * 128,), NAN, device=dev)

    def call(dtype=1, segs=((64, 0, True, True, 64),), n=64, M=256, P=128):
        arr = (N.GemmSeg * len(segs))(*[N.GemmSeg((x32 if dtype == 0 else x).data_ptr(), ch, t.data_ptr() if sc else None,
                                                  t.data_ptr() if sh else None, ld, act) for ch, act, sc, sh, ld in segs])
        return L.llie_pw_gemm(dtype, arr, len(segs), w.data_ptr(), None, None, out.data_ptr(), None, M, n, P, _st())
    bad = [dict(n=48), dict(segs=((48, 0, True, True, 48),)), dict(M=200), dict(segs=((64, 3, True, True, 64), (64, 1, True, True, 64))),
           dict(dtype=0, segs=((64, 3, True, True, 64),)), dict(segs=((64, 2, True, True, 64),)), dict(segs=((64, 1, False, False, 0),)),
           dict(segs=((64, 0, False, True, 64),)), dict(segs=((64, 0, True, True, 32),))]
    for kw in bad:
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out.view(torch.float16)[:256 * 64]).any()


# =============================================================================================
# llie_dwconv3x3_ex (dwconv.hip): strip widths, the ragged kernel, flags, pooling outputs, strip heights
DW_MAPS = R.DW_MAPS  # (H, W, TX, ragged); the backward test runs the same maps
DW_FLAGS = {"act": 0, "s6": 1, "noact": 2}


def _dw_params():
    out = []
    for i, (H, W, tx, rg) in enumerate(DW_MAPS):
        for dtype in DTYPES:
            cc = 32 if dtype == 0 else 64
            flags = ["act", "noact"] if dtype == 0 else ["act", "s6", "noact"]
            # every map runs every flag; the channel count and the pooling output rotate so that each (kernel, flag) pair meets one
            # chunk and three, and slab, totals and no pooling
            for j, fl in enumerate(flags):
                C = cc * (3 if (i + j) % 2 else 1)
                pool = ("slab", "totals", "none")[(i + j + dtype) % 3]
                out.append((H, W, tx, rg, dtype, fl, C, pool))
    return out


DW_PARAMS = _dw_params()


def _dw_inputs(B, H, W, C, dtype, fl, key):
    g = _gen("dw", key, dtype, fl)
    x = _rt(torch.randn(B, H, W, C, generator=g) * 2, dtype)
    sc, sh = torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g) + 1.5
    if fl == "s6":
        sc, sh = sc / 6, sh / 6
    w = torch.randn(9, C, generator=g) / 3
    return x, sc, sh, w


def _dw_call(dev, dtype, xd, scd, shd, wd, B, H, W, C, flags, pool, start=0, legacy=False):
    L = N.lib()
    out = Guarded((B, H, W, C), dev, TDT[dtype])
    nt = int(L.llie_dwconv3x3_tiles(H, W))
    slab = _slab(dev, B, nt, C) if pool == "slab" else None
    tot = Guarded((B, C), dev, torch.int64, fill=start) if pool == "totals" else None
    if legacy:
        rc = L.llie_dwconv3x3(dtype, xd.data_ptr(), out.ptr, scd.data_ptr(), shd.data_ptr(), wd.data_ptr(), slab.ptr if slab else None,
                              B, H, W, C, _st())
    else:
        rc = L.llie_dwconv3x3_ex(dtype, xd.data_ptr(), out.ptr, scd.data_ptr(), shd.data_ptr(), wd.data_ptr(), slab.ptr if slab else None,
                                 tot.ptr if tot else None, flags, B, H, W, C, _st())
    torch.cuda.synchronize()
    return rc, out, slab, tot, nt


def _dw_check(tag, dtype, x, sc, sh, w, fl, o, slab, tot, nt, tx, start):
    B, H, W, C = x.shape
    ref, ab, sl = R.dwconv3x3_ref(dtype, x, sc, sh, w, s6=fl == "s6", no_act=fl == "noact")
    _ratio(o, ref, ab, sl, R.BAR_DW, f"dw/{tag}")
    if slab is not None:
        pref, pab, psl = R.strip_pool_ref(o, tx)
        assert pref.shape[1] == nt
        _ratio(slab, pref, pab, psl, R.BAR_DW_POOL, f"dw_pool/{tag}")
    if tot is not None:
        pref, pab, _ = R.strip_pool_ref(o, tx)
        got = (tot - start).double() / 2.0 ** 24
        # every (8-row segment, strip) partial is rounded to a multiple of 2^-24 once
        _ratio(got, pref.sum(1), pab.sum(1), torch.full_like(got, pref.shape[1] * 2.0 ** -25), R.BAR_DW_POOL, f"dw_totals/{tag}")


@pytest.mark.parametrize("H,W,tx,ragged,dtype,fl,C,pool", DW_PARAMS,
                         ids=[f"{h}x{w}-dt{d}-{f}-c{c}-{p}" for h, w, _, _, d, f, c, p in DW_PARAMS])
def test_dwconv3x3_ex_vs_float64(dev, H, W, tx, ragged, dtype, fl, C, pool):
    """llie_dwconv3x3_ex: strip widths 8 / 16 / 32 and the ragged kernel (W or H not a multiple of 8), non-square maps both ways
    round, one channel chunk and three, flags 0 / s6 (2-byte: clamp01 prologue, weights T(6 w)) / no_act, and the three pooling
    outputs: the slab entry by entry ([B][llie_dwconv3x3_tiles][C], 8-row segments x strips), the fixed-point totals / 2^24
    against the float64 sum of the stored output (from a non-zero start too: the kernel adds), or none.  B = 3.
    Measured worst ratio (MI355X, seeds 0..2), output: 2.64 fp32, 1.08 fp16, 0.18 bf16, bar BAR_DW = 26; slab 1.09 / 0.54 / 0 and
    totals 2.10 / 1.63 / 0.93, bar BAR_DW_POOL = 21."""
    L = N.lib()
    B = 3
    x, sc, sh, w = _dw_inputs(B, H, W, C, dtype, fl, (H, W, C, pool))
    xd, scd, shd, wd = (t.to(dev) for t in (x, sc, sh, w))
    assert int(L.llie_dwconv3x3_strip_rows(dtype, B, H, W, C)) == 8
    tag = f"{H}x{W}x{C}/dt{dtype}/{fl}/{pool}"
    start = 0 if (H + W) % 2 else (5 << 24) + 12345
    runs = []
    for _ in range(2):
        rc, out, slab, tot, nt = _dw_call(dev, dtype, xd, scd, shd, wd, B, H, W, C, DW_FLAGS[fl], pool, start)
        N.check(rc, "dwconv3x3_ex")
        assert _last() == ("dwconv3x3_ragged_kernel" if ragged else f"dwconv3x3_kernel<{TNAME[dtype]}, {tx}, 4>"), _last()
        runs.append((out.cpu("dw out"), _split(slab.cpu("dw pool"), B, nt, "dw pool") if slab else None, tot.cpu("dw totals") if tot else None))
    for a, b in zip(runs[0], runs[1]):
        if a is not None:
            _same(a, b, tag)
    _dw_check(tag, dtype, x, sc, sh, w, fl, runs[0][0], runs[0][1], runs[0][2], nt, tx, start)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dwconv3x3_is_ex_with_flags_zero(dev, dtype):
    """llie_dwconv3x3 and llie_dwconv3x3_ex with flags 0 and the same pool slab give the same bits (16 x 48, three chunks)."""
    B, H, W, C = 3, 16, 48, 3 * (32 if dtype == 0 else 64)
    x, sc, sh, w = _dw_inputs(B, H, W, C, dtype, "act", "legacy")
    xd, scd, shd, wd = (t.to(dev) for t in (x, sc, sh, w))
    rc, o1, s1, _, nt = _dw_call(dev, dtype, xd, scd, shd, wd, B, H, W, C, 0, "slab", legacy=True)
    N.check(rc, "dwconv3x3")
    rc, o2, s2, _, _ = _dw_call(dev, dtype, xd, scd, shd, wd, B, H, W, C, 0, "slab")
    N.check(rc, "dwconv3x3_ex")
    s1c, s2c = _split(s1.cpu("dw pool"), B, nt, "dw pool"), _split(s2.cpu("dw pool"), B, nt, "dw pool")
    _same(o1.cpu("dw out"), o2.cpu("dw out"), "out")
    _same(s1c, s2c, "pool")
    _dw_check(f"legacy/dt{dtype}", dtype, x, sc, sh, w, "act", o1.cpu(), s1c, None, nt, 16, 0)


DW_STRIPS = [(h, d) for h in (16, 32, 64) for d in H2]


@pytest.mark.parametrize("H,dtype", DW_STRIPS)
def test_dwconv3x3_strip_heights(dev, H, dtype):
    """Strips of 16, 32 and 64 rows: dw_pick_tyl needs >= 1024 workgroups, so W = 8, C = 64, H = the strip height, B = 1024 made of
    three distinct images repeated.  llie_dwconv3x3_strip_rows must name the height; images 0..2 are checked against the
    reference (output and pool slab, s6 form), every other image must equal its twin bit for bit."""
    L = N.lib()
    B, W, C = 1024, 8, 64
    assert int(L.llie_dwconv3x3_strip_rows(dtype, B, H, W, C)) == H
    x, sc, sh, w = _dw_inputs(3, H, W, C, dtype, "s6", ("strip", H))
    idx = torch.arange(B) % 3
    xd, scd, shd, wd = x[idx].contiguous().to(dev), sc[idx].contiguous().to(dev), sh[idx].contiguous().to(dev), w.to(dev)
    runs = []
    for _ in range(2):
        rc, out, slab, _, nt = _dw_call(dev, dtype, xd, scd, shd, wd, B, H, W, C, 1, "slab")
        N.check(rc, "dwconv3x3_ex")
        assert _last() == f"dwconv3x3_kernel<{TNAME[dtype]}, 8, 4>", _last()
        runs.append((out.cpu("dw out"), _split(slab.cpu("dw pool"), B, nt, "dw pool")))
    _same(runs[0][0], runs[1][0], "out")
    _same(runs[0][1], runs[1][1], "pool")
    o, s = runs[0]
    _same(o, o[idx], "an image and its twin (out)")
    _same(s, s[idx], "an image and its twin (pool)")
    _dw_check(f"strip{H}/dt{dtype}", dtype, x, sc, sh, w, "s6", o[:3], s[:3], None, nt, 8, 0)


def test_dwconv3x3_strip_heights_all_covered():
    """The cases above reach every strip height: 8 (every B = 3 case), 16, 32 and 64."""
    L = N.lib()
    got = {int(L.llie_dwconv3x3_strip_rows(d, 1024, h, 8, 64)) for h, d in DW_STRIPS}
    got |= {int(L.llie_dwconv3x3_strip_rows(p[4], 3, p[0], p[1], p[6])) for p in DW_PARAMS}
    assert got == {8, 16, 32, 64}, got
    assert int(L.llie_dwconv3x3_strip_rows(1, 3, 16, 16, 48)) == N.ERR_ARG and int(L.llie_dwconv3x3_strip_rows(3, 3, 16, 16, 64)) == N.ERR_ARG


def test_dwconv3x3_ex_refusals(dev):
    """s6 with no_act, s6 in fp32, pool with pool_totals, unknown flag bits, C off the chunk size, NULL tensors: LLIE_ERR_ARG before
    any HIP call; the NaN-filled output stays NaN."""
    L = N.lib()
    x = torch.zeros(2 * 8 * 8 * 64, device=dev)
    out = torch.full((2 * 8 * 8 * 64,), NAN, device=dev)
    t = torch.zeros(2 * 9 * 64, device=dev)
    q = torch.zeros(2 * 64, dtype=torch.int64, device=dev)

    def call(dtype=1, pool=None, tot=None, flags=0, C=64, xin=x.data_ptr()):
        return L.llie_dwconv3x3_ex(dtype, xin, out.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), pool, tot, flags, 2, 8, 8, C, _st())
    for kw in (dict(flags=3), dict(dtype=0, flags=1), dict(pool=t.data_ptr(), tot=q.data_ptr()), dict(flags=4), dict(flags=-1), dict(C=32),
               dict(dtype=0, C=48), dict(xin=None), dict(dtype=3)):
        assert call(**kw) == N.ERR_ARG, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"


# =============================================================================================
# llie_conv3x3 (conv.hip: launch_conv_t): 3 modes x {TW 16, TW 8, ragged} x {BN 128, 64, 32}
CONV_MAPS = {  # mode -> output maps (Ho, Wo, TW, ragged)
    0: [(8, 16, 16, False), (16, 32, 16, False), (16, 8, 8, False), (8, 24, 8, False), (9, 13, 8, True), (13, 9, 8, True)],
    1: [(8, 16, 16, False), (16, 32, 16, False), (16, 8, 8, False), (8, 24, 8, False), (18, 26, 8, True), (26, 10, 8, True)],
    2: [(8, 16, 16, False), (16, 32, 16, False), (16, 8, 8, False), (8, 24, 8, False), (9, 13, 8, True), (13, 9, 8, True), (9, 16, 8, True)],
}
CONV_CH = [(32, 64), (64, 32), (96, 32), (128, 128), (32, 96)]


def _conv_cfg(tw, ragged, cout):
    bn = 128 if cout % 128 == 0 else (64 if cout % 64 == 0 else 32)
    wmwn = "2, 2" if bn >= 64 else ("4, 1" if (tw == 16 and not ragged) else "2, 1")
    return f"{tw}, {bn}, {wmwn}"


CONV_PARAMS = [(m, ho, wo, tw, rg, CONV_CH[(i + k) % 5], d) for m in (0, 1, 2) for i, (ho, wo, tw, rg) in enumerate(CONV_MAPS[m])
               for k in (0, 3) for d in DTYPES]


@pytest.mark.parametrize("mode,Ho,Wo,tw,ragged,ch,dtype", CONV_PARAMS,
                         ids=[f"m{m}-{ho}x{wo}-c{c[0]}_{c[1]}-dt{d}" for m, ho, wo, _, _, c, d in CONV_PARAMS])
def test_conv3x3_vs_float64(dev, mode, Ho, Wo, tw, ragged, ch, dtype):
    """llie_conv3x3 in modes 0 (stride 2), 1 (bilinear x2 first; the blended patch is rounded to T before the MFMA, mirrored) and 2
    (stride 1), on 16-wide tiles, 8-wide tiles and ragged maps, all non-square, Cin != Cout, every BN; with bias and statistics and
    without either.  The statistics slab [B][llie_conv3x3_tiles][2][Cout] is checked entry by entry against the stored values.
    Measured worst ratio (MI355X, seeds 0..2), output: 4.87 fp32, 0.50 fp16, 0.19 bf16, bar BAR_CONV = 49; statistics: 1.67 / 1.54 /
    1.15, bar BAR_CONV_STATS = 17."""
    L = N.lib()
    B, (cin, cout) = 2, ch
    Hi, Wi = (2 * Ho, 2 * Wo) if mode == 0 else ((Ho // 2, Wo // 2) if mode == 1 else (Ho, Wo))
    g = _gen("conv", mode, Ho, Wo, ch, dtype)
    x = _rt(torch.randn(B, Hi, Wi, cin, generator=g), dtype)
    w = _rt(torch.randn(9, cout, cin, generator=g) / math.sqrt(9 * cin), dtype)
    bias = torch.randn(cout, generator=g) * 0.3
    xd, wd, bd = x.to(dev), w.to(dev), bias.to(dev)
    nt = int(L.llie_conv3x3_tiles(Ho, Wo))
    tag = f"m{mode}/{Ho}x{Wo}/c{cin}_{cout}/dt{dtype}"
    for full in (True, False):
        runs = []
        for _ in range(2):
            out = Guarded((B, Ho, Wo, cout), dev, TDT[dtype])
            slab = _slab(dev, B, nt, 2, cout) if full else None
            N.check(L.llie_conv3x3(dtype, mode, xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if full else None, out.ptr,
                                   slab.ptr if full else None, B, Hi, Wi, cin, cout, _st()), "conv3x3")
            torch.cuda.synchronize()
            assert _last() == f"conv3x3_kernel<{TNAME[dtype]}, {mode}, {_conv_cfg(tw, ragged, cout)}>", _last()
            runs.append((out.cpu("conv out"), _split(slab.cpu("conv stats"), B, nt, "conv stats") if full else None))
        _same(runs[0][0], runs[1][0], tag)
        ref, ab, sl = R.conv3x3_ref(dtype, x, w, bias if full else None, mode)
        _ratio(runs[0][0], ref, ab, sl, R.BAR_CONV, f"conv/{tag}/{'full' if full else 'bare'}")
        if full:
            s = runs[0][1]
            _same(s, runs[1][1], tag + " stats")
            sref, sab, ssl = R.conv_tile_stats_ref(runs[0][0], tw)
            assert sref.shape[1] == nt
            _ratio(s, sref, sab, ssl, R.BAR_CONV_STATS, f"conv_stats/{tag}")


def test_conv3x3_refusals(dev):
    """Odd Hi / Wi in mode 0, channels that are not a multiple of 32 and modes outside 0..2 are refused; nothing is written."""
    L = N.lib()
    x = torch.zeros(2 * 18 * 18 * 64, dtype=torch.float16, device=dev)
    w = torch.zeros(9 * 64 * 64, dtype=torch.float16, device=dev)
    out = torch.full((2 * 18 * 18 * 64,), NAN, dtype=torch.float16, device=dev)

    def call(mode=0, Hi=16, Wi=16, cin=64, cout=64):
        return L.llie_conv3x3(1, mode, x.data_ptr(), w.data_ptr(), None, out.data_ptr(), None, 2, Hi, Wi, cin, cout, _st())
    for kw in (dict(Hi=17), dict(Wi=9), dict(cin=48), dict(cout=40), dict(mode=2, cin=16), dict(mode=3), dict(mode=-1)):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"


# =============================================================================================
# llie_linattn (small.hip): splits, partial chunks, multi-chunk spans, and the kv scratch the backward pass reads
ATTN_N = {25: 1, 64: 1, 81: 1, 100: 1, 128: 1, 256: 2, 384: 1, 512: 4, 1024: 8, 2048: 8}
ATTN_PARAMS = [(n, h, b, d) for n in ATTN_N for h, b in ((1, 1), (3, 3), (1, 3), (3, 1)) for d in DTYPES]


@pytest.mark.parametrize("n,heads,B,dtype", ATTN_PARAMS, ids=[f"n{n}-h{h}-b{b}-dt{d}" for n, h, b, d in ATTN_PARAMS])
def test_linattn_vs_float64(dev, n, heads, B, dtype):
    """llie_linattn for N with a partial last 64-position chunk (25, 81, 100), one to six chunks per span (384), 1 / 2 / 4 / 8
    splits and spans of 128 and 256 positions.  The output per entry, with |.| propagated through numerator and denominator, and the
    kv scratch [llie_linattn_splits(N)][B][heads][32][33] (column 32 = ksum), every split against the reference over its own
    position range: it is what llie_linattn_backward consumes.
    Measured worst ratio (MI355X, seeds 0..2), output: 2.04 fp32, 0 fp16 (inside the ulp of the stored value), 0.06 bf16, bar BAR_ATTN =
    20; kv: 15.83 / 10.75 / 10.31 (at spans of 256 and 384 positions, summed one after the other; 2.6 at N = 25), bar BAR_ATTN_KV = 160."""
    L = N.lib()
    inner = heads * 32
    ns = int(L.llie_linattn_splits(n))
    assert ns == ATTN_N[n]
    qkv = _rt(torch.randn(B, n, 3 * inner, generator=_gen("attn", n, heads, B, dtype)) * 0.8, dtype)
    qd = qkv.to(dev)
    runs = []
    for _ in range(2):
        kv = Guarded((ns, B, heads, 32, 33), dev)
        out = Guarded((B, n, inner), dev, TDT[dtype])
        N.check(L.llie_linattn(dtype, qd.data_ptr(), kv.ptr, out.ptr, B, n, heads, _st()), "linattn")
        torch.cuda.synchronize()
        runs.append((out.cpu("linattn out"), kv.cpu("linattn kv")))
    _same(runs[0][0], runs[1][0], "out")
    _same(runs[0][1], runs[1][1], "kv")
    ref, ab, kvr, kva = R.linattn_ref(qkv, heads, R.linattn_splits_ranges(n, ns))
    tag = f"n{n}/h{heads}/b{B}/dt{dtype}"
    _ratio(runs[0][1], kvr, kva, _ulp(kvr, 0), R.BAR_ATTN_KV, f"linattn_kv/{tag}")
    _ratio(runs[0][0], ref, ab, _ulp(ref, dtype), R.BAR_ATTN, f"linattn/{tag}")


# =============================================================================================
# llie_groupnorm_finalize (small.hip)
GN_PARAMS = [(c, p, f, ps, 0.0) for c in (32, 96, 256) for p in (81, 128, 1024) for f in ("none", "image", "shared") for ps in (0.0, 1.0 / 6.0)]
GN_PARAMS += [(96, 1024, "image", 0.0, 20.0), (256, 81, "shared", 1.0 / 6.0, 20.0)]
GN_SPLIT = {32: (16, 16), 96: (64, 32), 256: (160, 96)}  # 96: group 21 (channels 63..65) straddles the two slabs


def _gn_slab(y, nt):
    """[B][P][ch] float64 -> fp32 [B][nt][2][ch]: (sum, sum of squares) of nt nearly equal runs of rows"""
    return torch.stack([torch.stack([t.sum(1), (t * t).sum(1)], 1) for t in torch.tensor_split(y, nt, dim=1)], 1).float().contiguous()


@pytest.mark.parametrize("C,P,film,post,offset", GN_PARAMS, ids=[f"c{c}-p{p}-{f}-ps{int(ps > 0)}-m{int(o)}" for c, p, f, ps, o in GN_PARAMS])
def test_groupnorm_finalize_vs_float64(dev, C, P, film, post, offset):
    """llie_groupnorm_finalize with 1, 3 and 8 channels per group, two slabs with different tile counts (2 and 4) as a virtual concat
    (at C = 96 a group straddles them), P = 81 / 128 / 1024, FiLM none / one row per image / one row for all (film_stride 0),
    post_scale 0 and 1/6, and |mean| = 20 sigma (cancellation in E[x^2] - mean^2).  B = 3.  The reference is float64 from the fp32
    slab values as given; scale and shift themselves are compared, each against the absolute sum of its own expression times the
    condition of the variance.  Measured worst ratio (MI355X, seeds 0..2): scale 2.16, shift 3.00; bar BAR_GN = 30."""
    L = N.lib()
    B, (c0, c1) = 3, GN_SPLIT[C]
    g = _gen("gn", C, P, film, post, offset)
    y = torch.randn(B, P, C, generator=g, dtype=torch.float64) * 1.7 + (offset * 1.7 if offset else 0.3)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    s0, s1 = _gn_slab(y[..., :c0], 2), _gn_slab(y[..., c0:], 4)
    rows = B if film == "image" else 1
    fl = torch.randn(rows, 2 * C + 8, generator=g) * 0.3 if film != "none" else None
    stride = (2 * C + 8) if film == "image" else 0
    s0d, s1d, gd, bd = s0.to(dev), s1.to(dev), gamma.to(dev), beta.to(dev)
    fd = fl.to(dev) if fl is not None else None
    runs = []
    for _ in range(2):
        sc, sh = Guarded((B, C), dev), Guarded((B, C), dev)
        N.check(L.llie_groupnorm_finalize(s0d.data_ptr(), 2, c0, s1d.data_ptr(), 4, c1, 32, P, gd.data_ptr(), bd.data_ptr(), _ptr(fd), stride,
                                          1e-5, post, B, sc.ptr, sh.ptr, _st()), "groupnorm_finalize")
        torch.cuda.synchronize()
        runs.append((sc.cpu("gn scale"), sh.cpu("gn shift")))
    _same(runs[0][0], runs[1][0], "scale")
    _same(runs[0][1], runs[1][1], "shift")
    rsc, rsh, asc, ash = R.gn_finalize_ref([s0, s1], 32, P, gamma, beta, fl[:, :2 * C] if fl is not None else None, film == "image", 1e-5, post)
    tag = f"c{C}/p{P}/{film}/ps{post:.2f}/m{offset:.0f}"
    _ratio(runs[0][0], rsc, asc, _ulp(rsc, 0), R.BAR_GN, f"gn_scale/{tag}")
    _ratio(runs[0][1], rsh, ash, _ulp(rsh, 0), R.BAR_GN, f"gn_shift/{tag}")


# =============================================================================================
# llie_se_mlp (small.hip): the narrowest and the widest block of each variant (model.cpp: hid = 4 Cin, or 2 Cin for tiny; Cs = hid / 4;
# the widest block is the first decoder block, Cin = 2 x 8 x base_channels), B = 1 and both sides of kSeMaxB = 4
SE_SHAPES = [(32, 8), (512, 128), (128, 32), (2048, 512), (192, 48), (3072, 768), (256, 64), (4096, 1024)]
SE_PARAMS = [(c, cs, b, d) for c, cs in SE_SHAPES for b in (1, 4, 5) for d in DTYPES]


@pytest.mark.parametrize("C,Cs,B,dtype", SE_PARAMS, ids=[f"c{c}-s{s}-b{b}-dt{d}" for c, s, b, d in SE_PARAMS])
def test_se_mlp_vs_float64(dev, C, Cs, B, dtype):
    """llie_se_mlp: mean, hidden and gate per entry, each stage against the reference fed with the kernel's own previous stage.
    C up to 4096 (rows longer than the prefetched 2048 / 1024 elements), Cs = 8 (shorter than a vector per lane), B = 1, 4, 5.
    Measured worst ratio (MI355X, seeds 0..2): mean 0, hidden 0.62, gate 1.96, alike in every weight type; bar BAR_SE = 20."""
    L = N.lib()
    P = 324
    g = _gen("se", C, Cs, B, dtype)
    sums = torch.randn(B, C, generator=g) * P * 0.5
    w1, w2 = _rt(torch.randn(Cs, C, generator=g) / math.sqrt(C), dtype), _rt(torch.randn(C, Cs, generator=g) / math.sqrt(Cs), dtype)
    b1, b2 = torch.randn(Cs, generator=g) * 2.5 + 2.5, torch.randn(C, generator=g) * 0.5  # hidden on both sides of 0 and of 6
    dd = [t.to(dev) for t in (sums, w1, b1, w2, b2)]
    runs = []
    for _ in range(2):
        mean, hid, gate = Guarded((B, C), dev), Guarded((B, Cs), dev), Guarded((B, C), dev)
        N.check(L.llie_se_mlp(dtype, dd[0].data_ptr(), P, dd[1].data_ptr(), dd[2].data_ptr(), dd[3].data_ptr(), dd[4].data_ptr(), mean.ptr,
                              hid.ptr, gate.ptr, B, C, Cs, _st()), "se_mlp")
        torch.cuda.synchronize()
        runs.append((mean.cpu("se mean"), hid.cpu("se hidden"), gate.cpu("se gate")))
    for a, b, what in zip(runs[0], runs[1], ("mean", "hidden", "gate")):
        _same(a, b, what)
    mk, hk, gk = runs[0]
    (m, ma), (h, ha), (gt, ga) = R.se_mlp_ref(sums, P, w1, b1, w2, b2, mean=mk, hidden=hk)
    tag = f"c{C}/s{Cs}/b{B}/dt{dtype}"
    _ratio(mk, m, ma, _ulp(m, 0), R.BAR_SE, f"se_mean/{tag}")
    _ratio(hk, h, ha, _ulp(h, 0), R.BAR_SE, f"se_hidden/{tag}")
    _ratio(gk, gt, ga, _ulp(gt, 0), R.BAR_SE, f"se_gate/{tag}")
