"""pw_expand, the Gram statistics, their finalize, FiLM and silu_rows, per launch path, against the float64 references of
tests/kernel_refs.py.

Method (as tests/test_gpu_forward_kernels.py): inputs are drawn in fp32 with a seeded generator and rounded to the storage type; the
reference mirrors the kernel's roundings and nothing else; an entry passes when |out - ref| - slack < BAR * 2^-24 * abssum
(kernel_refs._ratio; the BAR_* constants stand in kernel_refs.py with the measured worst ratios beside them).  Every output is
prefilled with NaN and sits between canaries; every call is made twice and must give the same bits; an image (a row) alone gives the
bits it has inside the batch; where a launcher records a name, llie_last_kernel() must name the kernel.
tests/test_forward_refs_host.py checks, without a GPU, that these references agree with torch's float64 operators, that the bars
reject subtly wrong kernels and that the grid values of the case tables follow from the launch rules.

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
from kernel_refs import NAN, TDT, Guarded, _ratio, _same, _slab, _split  # noqa: E402

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

SEED0 = int(os.environ.get("LLIE_FWD_TEST_SEED", "0"))
H2 = [1, 2]
TNAME = {1: "_Float16", 2: "__bf16"}


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


# =============================================================================================
# llie_pw_expand
def _pwx_call(dev, dtype, segs, xd, scd, bid, ld, w32d, wpack, n, P, B):
    """one launch on fresh guarded buffers; w32d None = the pre-packed call.  -> (out [B][P][n], slab [B][P / 128][2][n])"""
    arr = (N.GemmSeg * len(segs))()
    off = 0
    for i, (c, x) in enumerate(zip(segs, xd)):
        arr[i] = N.GemmSeg(x.data_ptr(), c, scd.data_ptr() + off * 4, bid.data_ptr() + off * 4, ld, 3)
        off += c
    out = Guarded((B * P + 1, n), dev, TDT[dtype])
    nt = P // 128
    slab = _slab(dev, B, nt, 2, n)
    N.check(N.lib().llie_pw_expand(dtype, arr, len(segs), w32d.data_ptr() if w32d is not None else None, wpack.ptr, out.ptr, slab.ptr,
                                   B * P, n, P, _st()), "pw_expand")
    torch.cuda.synchronize()
    o = out.cpu("pw_expand out")
    assert torch.isnan(o[B * P:].float()).all(), "pw_expand: wrote past its last row"
    return o[:B * P].view(B, P, n), _split(slab.cpu("pw_expand stats"), B, nt, "pw_expand stats")


PWX_PARAMS = [(c, d) for c in R.PWX_CASES for d in H2]


@pytest.mark.parametrize("case,dtype", PWX_PARAMS, ids=[f"k{'_'.join(map(str, c[0]))}-n{c[1]}-p{c[2]}-b{c[3]}-dt{d}" for c, d in PWX_PARAMS])
def test_pw_expand_vs_float64(dev, case, dtype):
    """llie_pw_expand on every case of kernel_refs.PWX_CASES (the comments there say which launch path a case reaches): nsplit 1
    ([128] -> 64, 576; [512] -> 1088) and 2 ([192] -> 128; [128, 64] -> 1152); channel loops of 18 and 34 weight buffers (N = 576,
    1152, 1088: odd multiples of 64, which the rule cannot split further); three segments (the koff2 branch) at K = 192, 256, 384 and
    512; affine_ld = K + 24 with per-segment offsets ([64, 64] -> 512 and [64, 64, 64] -> 768); the rotating 3-deep prefetch (K = 256,
    384, 512) over one and three segments; the K = 512 form that stores straight from registers; the tile remap on and off.
    The output has one guarded extra row, the slab one guarded extra entry.  The call is made twice, then a third time with w32 =
    NULL on the pack the first call left (equal bits each time); every image alone -- another nsplit, another tile order -- gives the
    bits of its row.  nsplit is asserted through llie_pw_expand_nsplit.  The statistics are judged entry by entry against the sums
    of the values the kernel stored.
    Measured worst ratio (MI355X, seeds 0..2), output: 0.42 fp16, 0.27 bf16, bar BAR_PWX = 4.3; statistics: 1.69 / 1.54, bar
    BAR_PWX_STATS = 17."""
    segs, n, P, B, ldx, (nsplit, _remap, _nit) = case
    L = N.lib()
    K = sum(segs)
    xs, w32, sc, bi = R.pwx_inputs(_gen("pwx", segs, n, P, B, dtype), dtype, segs, n, P, B, ldx)
    assert int(L.llie_pw_expand_nsplit(B * P, n)) == nsplit
    xd, scd, bid, w32d = [x.to(dev) for x in xs], sc.to(dev), bi.to(dev), w32.to(dev)
    wpack = Guarded((n * K,), dev, TDT[dtype])
    name = f"pw_expand_kernel<{TNAME[dtype]}, {K // 16}, 1>"
    runs = []
    for w in (w32d, w32d, None):
        runs.append(_pwx_call(dev, dtype, segs, xd, scd, bid, K + ldx, w, wpack, n, P, B))
        assert _last() == name, _last()
    wpack.cpu("pw_expand pack")
    for (o, s), what in zip(runs[1:], ("second call", "pre-packed call")):
        _same(runs[0][0], o, f"out, {what}")
        _same(runs[0][1], s, f"stats, {what}")
    out, slab = runs[0]
    if B > 1:
        for b in range(B):
            o1, s1 = _pwx_call(dev, dtype, segs, [x[b:b + 1].contiguous() for x in xd], scd[b:b + 1].contiguous(), bid[b:b + 1].contiguous(),
                               K + ldx, None, wpack, n, P, 1)
            _same(out[b:b + 1], o1, f"image {b} alone (out)")
            _same(slab[b:b + 1], s1, f"image {b} alone (stats)")
    what = f"k{'_'.join(map(str, segs))}-n{n}-p{P}/dt{dtype}"
    ref, ab, sl = R.pw_expand_ref(dtype, xs, R.seg_tables(segs, sc, bi), w32)
    _ratio(out, ref, ab, sl, R.BAR_PWX, "pwx/" + what)
    sref, sab, ssl = R.tile_stats_ref(out, 128)
    _ratio(slab, sref, sab, ssl, R.BAR_PWX_STATS, "pwx_stats/" + what)


def test_pw_expand_refusals(dev):
    """Out-of-contract calls are refused before any launch (the NaN-filled output stays NaN, no kernel name is recorded): K outside
    {128, 192, 256, 384, 512}, P % 128, M % P, N % 64, a segment that is no multiple of 64, more than three segments, an activation
    other than 3, fp32, affine_ld < channels, and a null segment list, segment pointer, table, pack, output or slab."""
    L = N.lib()
    x = torch.zeros(256, 256, dtype=torch.float16, device=dev)
    t = torch.zeros(2, 512, device=dev)
    w = torch.zeros(512 * 512, device=dev)
    pack = torch.zeros(512 * 512, dtype=torch.float16, device=dev)
    out = torch.full((256 * 512,), NAN, dtype=torch.float16, device=dev)
    stats = torch.full((2 * 2 * 512,), NAN, device=dev)
    p, tp = x.data_ptr(), t.data_ptr()

    def call(dtype=1, segs=((p, 128, tp, tp, 128, 3),), n=512, M=256, P=128, arr=True, pk=pack.data_ptr(), o=out.data_ptr(), s=stats.data_ptr()):
        a = (N.GemmSeg * len(segs))(*[N.GemmSeg(*sg) for sg in segs]) if arr else None
        return L.llie_pw_expand(dtype, a, len(segs), w.data_ptr(), pk, o, s, M, n, P, _st())
    seg = lambda ch, **kw: (kw.get("ptr", p), ch, kw.get("sc", tp), kw.get("sh", tp), kw.get("ld", ch), kw.get("act", 3))  # noqa: E731
    bad = [dict(segs=(seg(64),)), dict(segs=(seg(320),)), dict(segs=(seg(64), seg(32), seg(32))), dict(segs=(seg(96), seg(96))), dict(P=96, M=192),
           dict(M=320), dict(n=96), dict(segs=(seg(64), seg(64), seg(64), seg(64))), dict(segs=(seg(128, act=1),)), dict(segs=(seg(128, act=0),)),
           dict(dtype=0), dict(dtype=3), dict(segs=(seg(128, ld=64),)), dict(segs=(seg(64), seg(64, ld=0))), dict(arr=False), dict(segs=(seg(128, ptr=None),)),
           dict(segs=(seg(128, sc=None),)), dict(segs=(seg(128, sh=None),)), dict(pk=None), dict(o=None), dict(s=None)]
    before = _last()
    for kw in bad:
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert _last() == before
    assert torch.isnan(out.float()).all() and torch.isnan(stats).all()
    assert call() == 0  # the contract itself is met by the defaults
    torch.cuda.synchronize()
    assert torch.isfinite(out[:256 * 512].float()).all()
    assert L.llie_pw_expand_nsplit(100, 512) < 0 and L.llie_pw_expand_nsplit(256, 96) < 0 and L.llie_pw_expand_nsplit(0, 512) < 0


# =============================================================================================
# llie_gram_stats
def _gram_run(dev, dtype, c0, c1, P, x0, x1, sc, bi):
    """two launches on the same tickets -> gtot [B][K K + K] of the first, after asserting the second one's bits, the guards, the
    tickets and the kernel name"""
    L = N.lib()
    K, B = c0 + c1, x0.shape[0]
    d = [t.contiguous().to(dev) if t is not None else None for t in (x0, x1, sc, bi)]
    pf = int(L.llie_gram_part_floats(K, P))
    tick = torch.zeros(B, dtype=torch.int32, device=dev)
    got = []
    for _ in range(2):
        part, gtot = Guarded((B * pf,), dev), Guarded((B, K * K + K), dev)
        N.check(L.llie_gram_stats(dtype, d[0].data_ptr(), c0, d[1].data_ptr() if c1 else None, c1, d[2].data_ptr(), d[3].data_ptr(), B, P,
                                  part.ptr, gtot.ptr, tick.data_ptr(), _st()), "gram_stats")
        torch.cuda.synchronize()
        assert _last() == "gram_stats_kernel", _last()
        assert int(tick.abs().sum()) == 0, "tickets left non-zero"
        assert torch.isfinite(part.cpu("gram part")).all(), "a partial left unwritten"
        got.append(gtot.cpu("gram totals"))
    _same(got[0], got[1], "gram totals")
    return got[0]


GRAM_PARAMS = [(c, d, f) for c in R.GRAM_CASES for d in H2 for f in ("gauss", "ones")]


@pytest.mark.parametrize("case,dtype,family", GRAM_PARAMS, ids=[f"c{c[0]}_{c[1]}-p{c[2]}-b{c[3]}-dt{d}-{f}" for c, d, f in GRAM_PARAMS])
def test_gram_stats_vs_float64(dev, case, dtype, family):
    """llie_gram_stats with 1, 3, 8, 17, 17, 16 and 16 workgroup partials per image (kernel_refs.GRAM_CASES; nwg is derived from
    llie_gram_part_floats and asserted): the last-ticket sum runs one ragged group (nwg 1, 3, 8), one full group (16), and a full
    group plus a one-partial tail (nwg 17: P = 8704 at K = 96, and P = 17408 = 136 x 128 pixels, the frame-mode shape, at K = 32); K =
    32, 64 and 96, with and without a second input.  `part` and `gtot` are guarded and prefilled with NaN; the launch is repeated
    on the tickets the first one left (zero afterwards, equal bits); every image alone gives its row; G is bitwise symmetric; G
    and m are judged per entry.  Family "ones": the first input's activations are all 1 and the rest 0, so G and m are the exact
    integers P and 0 and a missing or doubled partial shows as an integer difference (asserted with torch.equal).
    Measured worst ratio (MI355X, seeds 0..2), G: 2.39 fp16, 2.94 bf16, bar BAR_GRAM = 30; m: 1.78 / 1.93, bar BAR_GRAM_M = 20."""
    c0, c1, P, B, nwg = case
    K, nf = c0 + c1, (c0 + c1) // 32
    assert int(N.lib().llie_gram_part_floats(K, P)) == nwg * (nf * (nf + 1) // 2 * 1024 + K)
    x0, x1, sc, bi = R.gram_inputs(_gen("gram", case, dtype, family), dtype, c0, c1, P, B, family)
    got = _gram_run(dev, dtype, c0, c1, P, x0, x1, sc, bi)
    if B > 1:
        for b in range(B):
            one = _gram_run(dev, dtype, c0, c1, P, x0[b:b + 1], x1[b:b + 1] if c1 else None, sc[b:b + 1], bi[b:b + 1])
            _same(got[b:b + 1], one, f"image {b} alone")
    G, m = got[:, :K * K].view(B, K, K), got[:, K * K:]
    assert torch.equal(G, G.transpose(1, 2)), "G is not bitwise symmetric"
    what = f"c{c0}_{c1}-p{P}/dt{dtype}/{family}"
    (gr, ga, gs), (mr, ma, ms) = R.gram_ref(dtype, x0, x1, sc, bi)
    if family == "ones":
        assert torch.equal(G.double(), gr) and torch.equal(m.double(), mr), "integer totals differ"
        assert gr[0, 0, 0] == P and mr[0, 0] == P and (c0 == K or gr[0, -1, -1] == 0)
    _ratio(G, gr, ga, gs, R.BAR_GRAM, "gram/" + what)
    _ratio(m, mr, ma, ms, R.BAR_GRAM_M, "gram_m/" + what)


def test_gram_refusals(dev):
    """llie_gram_stats and llie_gram_finalize refuse, before any launch: K outside {32, 64, 96}, P % 512, c0 % 8, fp32, a second
    channel count without its tensor, and null pointers."""
    L = N.lib()
    x = torch.zeros(1024 * 96, dtype=torch.float16, device=dev)
    t = torch.zeros(2 * 96, device=dev)
    part = torch.full((2 * 2 * 6240,), NAN, device=dev)
    gtot = torch.full((2 * (96 * 96 + 96),), NAN, device=dev)
    tick = torch.zeros(2, dtype=torch.int32, device=dev)
    p, tp = x.data_ptr(), t.data_ptr()

    def stats(dtype=1, x0=p, c0=32, x1=None, c1=0, sc=tp, bi=tp, B=2, P=512, pa=part.data_ptr(), g=gtot.data_ptr(), tk=tick.data_ptr()):
        return L.llie_gram_stats(dtype, x0, c0, x1, c1, sc, bi, B, P, pa, g, tk, _st())
    before = _last()
    for kw in (dict(c0=128), dict(c0=16), dict(c0=48), dict(c0=32, c1=96, x1=p), dict(P=640), dict(P=256), dict(P=0), dict(c0=36, c1=28, x1=p), dict(dtype=0),
               dict(dtype=3), dict(c1=32), dict(x0=None), dict(sc=None), dict(bi=None), dict(pa=None), dict(g=None), dict(tk=None), dict(B=0)):
        assert stats(**kw) != 0, kw
    assert L.llie_gram_part_floats(48, 512) < 0 and L.llie_gram_part_floats(32, 640) < 0

    sc_o = torch.full((2 * 384,), NAN, device=dev)

    def fin(dtype=1, g=tp, w=p, K=32, P=512, ga=tp, be=tp, B=2, so=sc_o.data_ptr(), ho=sc_o.data_ptr()):
        return L.llie_gram_finalize(dtype, g, w, K, P, ga, be, None, 0, 1e-5, 0.0, B, so, ho, _st())
    for kw in (dict(K=48), dict(K=128), dict(dtype=0), dict(dtype=3), dict(P=0), dict(B=0), dict(g=None), dict(w=None), dict(ga=None), dict(be=None),
               dict(so=None), dict(ho=None)):
        assert fin(**kw) != 0, kw
    torch.cuda.synchronize()
    assert _last() == before
    assert torch.isnan(part).all() and torch.isnan(gtot).all() and torch.isnan(sc_o).all() and int(tick.abs().sum()) == 0


# =============================================================================================
# llie_gram_finalize
FIN_PARAMS = [(K, hard, d, film, post) for K in (32, 64, 96) for hard in (False, True) for d in H2 for film in (False, True) for post in (0.0, 1.0 / 6.0)]


@pytest.mark.parametrize("K,hard,dtype,film,post", FIN_PARAMS,
                         ids=[f"k{K}-{'hard' if h else 'plain'}-dt{d}-{'film' if f else 'nofilm'}-{'post' if ps else 'nopost'}" for K, h, d, f, ps in FIN_PARAMS])
def test_gram_finalize_vs_float64(dev, K, hard, dtype, film, post):
    """llie_gram_finalize at K = 32, 64, 96 and B = 3, with and without FiLM (rows film_stride = 2 C + 24 apart), post_scale 0 and
    1/6, on the plain and the ill-conditioned family of test_gpu_round4._gram_case.  The reference starts from the same fp32 totals
    the kernel is given, so only the kernel's own arithmetic is judged; scale and shift are judged per entry, between canaries, and
    two calls give equal bits.
    Measured worst ratio (MI355X, seeds 0..2), scale: 2.00 fp16, 1.96 bf16; shift: 1.91 / 1.84; bar BAR_GRAM_FIN = 20."""
    L = N.lib()
    B, P, C = 3, 2048, 4 * K
    g = _gen("gram_fin", K, hard, dtype)
    gtot, w, _ = R.gram_fin_inputs(g, dtype, K, P, B, hard)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    stride = 2 * C + 24
    fl = torch.randn(B, stride, generator=g) * 0.3 if film else None
    d = [t.to(dev) if t is not None else None for t in (gtot, w, gamma, beta, fl)]
    runs = []
    for _ in range(2):
        sc, sh = Guarded((B, C), dev), Guarded((B, C), dev)
        N.check(L.llie_gram_finalize(dtype, d[0].data_ptr(), d[1].data_ptr(), K, P, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr() if film else None,
                                     stride if film else 0, 1e-5, post, B, sc.ptr, sh.ptr, _st()), "gram_finalize")
        torch.cuda.synchronize()
        assert _last() == "gram_finalize_kernel", _last()
        runs.append((sc.cpu("gram_finalize scale"), sh.cpu("gram_finalize shift")))
    _same(runs[0][0], runs[1][0], "scale")
    _same(runs[0][1], runs[1][1], "shift")
    rsc, rsh, asc, ash = R.gram_finalize_ref(dtype, gtot, w, K, P, gamma, beta, fl, stride if film else 0, 1e-5, post)
    what = f"k{K}/{'hard' if hard else 'plain'}/dt{dtype}/film{int(film)}/post{int(post != 0)}"
    _ratio(runs[0][0], rsc, asc, R._ulp(rsc, 0), R.BAR_GRAM_FIN, "gram_fin_scale/" + what)
    _ratio(runs[0][1], rsh, ash, R._ulp(rsh, 0), R.BAR_GRAM_FIN, "gram_fin_shift/" + what)


# =============================================================================================
# llie_film / llie_silu_rows
def _film_call(dev, sd, wd, bd, rows, T, F_):
    out = Guarded((rows, F_), dev)
    N.check(N.lib().llie_film(sd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.ptr, rows, T, F_, _st()), "film")
    torch.cuda.synchronize()
    return out.cpu("film")


FILM_PARAMS = [(rows, T, F_) for T, F_ in ((128, 1000), (512, 6000), (64, 256)) for rows in (1, 3, 4, 5, 8, 9)]


@pytest.mark.parametrize("rows,T,F_", FILM_PARAMS, ids=[f"r{r}-t{t}-f{f}" for r, t, f in FILM_PARAMS])
def test_film_vs_float64(dev, rows, T, F_):
    """llie_film with 1, 3, 4, 5, 8 and 9 rows: film_kernel takes kSeMaxB = 4 rows per pass, so rows 5, 8 and 9 run blockIdx.y > 0,
    with a ragged last pass at 5 and 9; (T, F) = (128, 1000) and (512, 6000) as the forward pass has them (F no multiple of the 16
    outputs of a workgroup at 1000), and (64, 256): the backward pass's call with T = the sinusoidal dimension (backward.cpp: the
    first Linear of the time MLP recomputed).  Output between canaries with NaN prefill, twice with equal bits; row r alone gives the
    bits of row r.
    Measured worst ratio (MI355X, seeds 0..2): 0.86, bar BAR_FILM = 9."""
    g = _gen("film", rows, T, F_)
    st = torch.randn(rows, T, generator=g)
    wf, bf = torch.randn(F_, T, generator=g) / math.sqrt(T), torch.randn(F_, generator=g) * 0.1
    sd, wd, bd = st.to(dev), wf.to(dev), bf.to(dev)
    out = _film_call(dev, sd, wd, bd, rows, T, F_)
    _same(out, _film_call(dev, sd, wd, bd, rows, T, F_), "film")
    if rows > 1:
        for r in range(rows):
            _same(out[r:r + 1], _film_call(dev, sd[r:r + 1].contiguous(), wd, bd, 1, T, F_), f"row {r} alone")
    ref, ab, sl = R.film_ref(st, wf, bf)
    _ratio(out, ref, ab, sl, R.BAR_FILM, f"film/r{rows}-t{T}-f{F_}")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 9 * 512])
def test_silu_rows_vs_float64(dev, n):
    """llie_silu_rows (the companion of llie_film in both passes) below, at and above one workgroup of 256 values, and at rows x T =
    9 x 512; values up to |x| = 12 so that both tails of the sigmoid are reached.  Guarded output, twice with equal bits.
    Judged under BAR_FILM with the evaluation error of siluf as the absolute sum (kernel_refs.silu_ref); measured worst ratio 0.53."""
    L = N.lib()
    x = torch.randn(n, generator=_gen("silu", n)) * 4
    x[0] = 0.0
    xd = x.to(dev)
    outs = []
    for _ in range(2):
        out = Guarded((n,), dev)
        N.check(L.llie_silu_rows(xd.data_ptr(), out.ptr, n, _st()), "silu_rows")
        torch.cuda.synchronize()
        outs.append(out.cpu("silu_rows"))
    _same(outs[0], outs[1], "silu_rows")
    assert outs[0][0] == 0.0
    ref, ab, sl = R.silu_ref(x)
    _ratio(outs[0], ref, ab, sl, R.BAR_FILM, f"silu_rows/n{n}")


def test_film_and_silu_rows_refusals(dev):
    """null pointers and empty shapes are refused before any launch"""
    L = N.lib()
    t = torch.full((64,), NAN, device=dev)
    p = t.data_ptr()
    for a in ((None, p, p, p, 1, 8, 4), (p, None, p, p, 1, 8, 4), (p, p, None, p, 1, 8, 4), (p, p, p, None, 1, 8, 4), (p, p, p, p, 0, 8, 4),
              (p, p, p, p, 1, 0, 4), (p, p, p, p, 1, 8, 0)):
        assert L.llie_film(*a, _st()) == N.ERR_ARG, a
    for a in ((None, p, 8), (p, None, 8), (p, p, 0), (p, p, -3)):
        assert L.llie_silu_rows(*a, _st()) == N.ERR_ARG, a
    torch.cuda.synchronize()
    assert torch.isnan(t).all()
