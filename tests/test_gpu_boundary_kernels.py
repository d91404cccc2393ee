"""The head, tail and boundary kernels -- init_conv, final_conv (with the fused scheduler step), the SE gate from fixed-point totals,
affine_add, the layout converters and pw_gemm's `dot` epilogue -- per launch path against the float64 references of
tests/kernel_refs.py.

Method as tests/test_gpu_forward_kernels.py: seeded fp32 draws rounded to the storage type; B = 2 unless stated and non-square maps,
so a wrong image offset or exchanged H and W show; every output prefilled with NaN and compared entry by entry; every written
buffer between canaries, slabs with one extra guarded entry past the helper's count; every call made twice with equal bits;
llie_last_kernel() asserted.  An entry passes when |out - ref| - slack < BAR * 2^-24 * abssum; the BAR_* constants stand in
kernel_refs.py with the measured worst ratios beside them.  tests/test_forward_refs_host.py checks the references against torch's
own operators and that these bars reject subtly wrong kernels.

LLIE_FWD_TEST_SEED (default 0) shifts every seed: the bars were measured over seeds 0, 1 and 2.
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
import test_gpu_forward_kernels as FK  # noqa: E402  (GEMM_CASES and its input / call helpers)
from kernel_refs import NAN, TDT, Guarded, _ratio, _rt, _same, _slab, _split  # noqa: E402

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

SEED0 = int(os.environ.get("LLIE_FWD_TEST_SEED", "0"))
DTYPES = [0, 1, 2]
H2 = [1, 2]
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


def _pack(dev, nbytes):
    """pack scratch of the two convs: nbytes (a multiple of 16) between canaries, 16-byte aligned, prefilled with NaN"""
    assert nbytes > 0 and nbytes % 16 == 0
    return Guarded((nbytes // 4,), dev)


def _twice(call, names):
    """run `call` twice on fresh buffers; -> the first run's tensors (None where absent), after asserting equal bits"""
    a, b = call(), call()
    for x, y, n in zip(a, b, names):
        if x is not None:
            _same(x, y, n)
    return a


# =============================================================================================
# llie_init_conv (conv_edge.hip): the VALU kernel on 16 x 16 tiles, the MFMA kernel on 8 x 32 tiles
INIT_SPLITS = [(3, 3), (4, 4), (1, 2)]
INIT_MAPS = {0: [(16, 16), (24, 40), (32, 48)], 1: [(8, 32), (24, 40), (16, 72), (32, 128)]}
INIT_PARAMS = [(m, d, h, w, sp, co) for m in (0, 1) for d in (DTYPES if m == 0 else H2) for h, w in INIT_MAPS[m] for sp in INIT_SPLITS
               for co in (32, 64)]


@pytest.mark.parametrize("mfma,dtype,H,W,split,cout", INIT_PARAMS,
                         ids=[f"{'mfma' if m else 'valu'}-dt{d}-{h}x{w}-c{s[0]}_{s[1]}-o{c}" for m, d, h, w, s, c in INIT_PARAMS])
def test_init_conv_vs_float64(dev, mfma, dtype, H, W, split, cout):
    """llie_init_conv from the reference's OIHW weights through the engine's own repack.  VALU kernel (all three types; the 2-byte
    forms are reachable through the launcher alone) at 16 x 16 (one tile), 24 x 40 (partial tiles on both edges) and 32 x 48; MFMA
    kernel at 8 x 32, 24 x 40 (8 valid columns in the edge tile), 16 x 72 and 32 x 128 (16 tiles: xcd_tile_order is a real
    permutation); channel splits 3 + 3, 4 + 4 and 1 + 2; Cout 32 and 64 (the second 32-channel block loads its weights on another
    path); with the statistics slab -- checked entry by entry against the stored values, tiles of 16 x 16 or 8 x 32 -- and without.
    Measured worst ratio (MI355X, seeds 0..2), output: 4.81 fp32, 0.64 fp16, 0.67 bf16, bar BAR_INIT = 49; statistics: 1.29 / 2.54 /
    1.93, bar BAR_INIT_STATS = 26."""
    L = N.lib()
    B, (c0, c1) = 2, split
    g = _gen("init", mfma, dtype, H, W, split, cout)
    x0, x1 = torch.randn(B, c0, H, W, generator=g), torch.randn(B, c1, H, W, generator=g)
    w = torch.randn(cout, c0 + c1, 3, 3, generator=g) / math.sqrt(9 * (c0 + c1))
    bias = torch.randn(cout, generator=g) * 0.3
    x0d, x1d, wd, bd = (t.to(dev) for t in (x0, x1, w, bias))
    nt = int(L.llie_init_conv_tiles(H, W, mfma))
    assert nt == ((H // 8) * ((W + 31) // 32) if mfma else ((H + 15) // 16) * ((W + 15) // 16))
    nbytes = int(L.llie_init_conv_pack_bytes(c0 + c1, cout))
    tag = f"{'mfma' if mfma else 'valu'}/{H}x{W}/c{c0}_{c1}/o{cout}/dt{dtype}"
    ref, ab, sl = R.init_conv_ref(dtype, x0, x1, w, bias, mfma)
    for full in (True, False):
        def call():
            out, pack = Guarded((B, H, W, cout), dev, TDT[dtype]), _pack(dev, nbytes)
            slab = _slab(dev, B, nt, 2, cout) if full else None
            N.check(L.llie_init_conv(dtype, x0d.data_ptr(), c0, x1d.data_ptr(), c1, wd.data_ptr(), bd.data_ptr(), out.ptr,
                                     slab.ptr if full else None, B, H, W, cout, mfma, pack.ptr, nbytes, _st()), "init_conv")
            torch.cuda.synchronize()
            assert _last() == f"init_conv_{'mfma_' if mfma else ''}kernel<{TNAME[dtype]}>", _last()
            pack.cpu("init pack")
            return out.cpu("init out"), _split(slab.cpu("init stats"), B, nt, "init stats") if full else None
        o, s = _twice(call, ("out", "stats"))
        _ratio(o, ref, ab, sl, R.BAR_INIT, f"init/{tag}/{'full' if full else 'bare'}")
        if full:
            sref, sab, ssl = R.conv_tile_stats_ref(o, 32 if mfma else 16, 8 if mfma else 16)
            assert sref.shape[1] == nt
            _ratio(s, sref, sab, ssl, R.BAR_INIT_STATS, f"init_stats/{tag}")


# =============================================================================================
# llie_final_conv (conv_edge.hip): the VALU kernel, the MFMA kernel, and the MFMA kernel's fused scheduler step
FINAL_MAPS = [(16, 16), (24, 40), (64, 64)]
FINAL_PARAMS = [(m, d, h, w, c, co) for m in (0, 1) for d in (DTYPES if m == 0 else H2) for h, w in FINAL_MAPS for c in (32, 64, 96)
                for co in (3, 4)]


def _final_inputs(B, H, W, C, cout, dtype, key):
    g = _gen("final", key, dtype)
    x = _rt(torch.randn(B, H, W, C, generator=g) * 1.5, dtype)
    sc, sh = torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g) * 0.7
    w = torch.randn(cout, C, 3, 3, generator=g) / math.sqrt(9 * C)
    return g, x, sc, sh, w, torch.randn(cout, generator=g) * 0.3


def _final_name(mfma, dtype):
    return f"final_conv_mfma_kernel<{TNAME[dtype]}, 16>" if mfma else f"final_conv_kernel<{TNAME[dtype]}>"


@pytest.mark.parametrize("mfma,dtype,H,W,C,cout", FINAL_PARAMS,
                         ids=[f"{'mfma' if m else 'valu'}-dt{d}-{h}x{w}-c{c}-o{o}" for m, d, h, w, c, o in FINAL_PARAMS])
def test_final_conv_vs_float64(dev, mfma, dtype, H, W, C, cout):
    """llie_final_conv without the step: one, two and three 32-channel chunks (the MFMA kernel re-stages its weights per chunk), Cout
    3 (a zero fourth weight row) and 4, at 16 x 16 (one tile), 24 x 40 (partial tiles on both edges) and 64 x 64 (16 tiles: a real
    xcd_tile_order permutation).  The fp32 NCHW noise prediction is compared entry by entry; the MFMA reference rounds silu(x sc +
    sh) and the weights to T, the VALU one keeps both in fp32.  Measured worst ratio (MI355X, seeds 0..2): 0.75 fp32, 1.98 fp16, 2.15 bf16; bar
    BAR_FINAL = 26."""
    L = N.lib()
    B = 2
    _, x, sc, sh, w, bias = _final_inputs(B, H, W, C, cout, dtype, (mfma, H, W, C, cout))
    dd = [t.to(dev) for t in (x, sc, sh, w, bias)]
    nbytes = int(L.llie_final_conv_pack_bytes(C))

    def call():
        out, pack = Guarded((B, cout, H, W), dev), _pack(dev, nbytes)
        N.check(L.llie_final_conv(dtype, *(t.data_ptr() for t in dd), out.ptr, B, H, W, C, cout, mfma, None, None, None, None, None,
                                  pack.ptr, nbytes, _st()), "final_conv")
        torch.cuda.synchronize()
        assert _last() == _final_name(mfma, dtype), _last()
        pack.cpu("final pack")
        return (out.cpu("final out"),)
    (o,) = _twice(call, ("out",))
    ref, ab, sl = R.final_conv_ref(dtype, x, sc, sh, w, bias, mfma)
    _ratio(o, ref, ab, sl, R.BAR_FINAL, f"final/{'mfma' if mfma else 'valu'}/{H}x{W}/c{C}/o{cout}/dt{dtype}")


STEP_PARAMS = [(d, h, w, k) for d in H2 for h, w in ((24, 40), (64, 64)) for k in range(8)]


@pytest.mark.parametrize("dtype,H,W,k", STEP_PARAMS, ids=[f"dt{d}-{h}x{w}-v{k & 1}c{(k >> 1) & 1}l{k >> 2}" for d, h, w, k in STEP_PARAMS])
def test_final_conv_fused_step_vs_float64(dev, dtype, H, W, k):
    """The LCM step in final_conv_mfma_kernel's epilogue: all eight (v_prediction, clamp_x0, is_last) combinations at 24 x 40 and 64 x
    64, each with `out` and `clamped` given and NULL (four calls), noise NULL when is_last; C and Cout rotate over 32 / 64 / 96 and 3
    / 4.  sa and sap are drawn in [0.2, 1].  prev, clamped and (when given) the noise prediction are compared entry by entry with
    lcm_step_ref on final_conv_ref, whose absolute sum and slack they carry through sb / sa and sap; the noise prediction has the
    same bits with and without the step's outputs.  Measured worst ratio (MI355X, seeds 0..2), fp16 / bf16: prev 2.25 / 1.52, clamped 1.61 /
    1.49, bar BAR_STEP = 23; the noise prediction 2.59 / 2.09, bar BAR_FINAL = 26."""
    L = N.lib()
    B, C, cout = 2, (32, 64, 96)[k % 3], 3 + (k + H // 8) % 2
    vpred, clamp, last = k & 1, (k >> 1) & 1, k >> 2
    g, x, sc, sh, w, bias = _final_inputs(B, H, W, C, cout, dtype, ("step", H, W, k))
    sample, noise = torch.randn(B, cout, H, W, generator=g), torch.randn(B, cout, H, W, generator=g)
    sa, sap = (0.2 + 0.8 * torch.rand(2, generator=g)).tolist()
    coef = (sa, math.sqrt(1 - sa * sa), sap, math.sqrt(1 - sap * sap), last, vpred, clamp)
    cc = N.StepCoef(*coef)
    coef = tuple(getattr(cc, f) for f, _ in N.StepCoef._fields_)  # the fp32 values the kernel gets
    dd = [t.to(dev) for t in (x, sc, sh, w, bias)]
    sd, nd = sample.to(dev), noise.to(dev)
    nbytes = int(L.llie_final_conv_pack_bytes(C))
    eref, eab, esl = R.final_conv_ref(dtype, x, sc, sh, w, bias, True)
    step = R.lcm_step_ref(eref, eab, esl, sample, noise, coef)
    tag = f"{H}x{W}/c{C}/o{cout}/dt{dtype}/v{vpred}c{clamp}l{last}"
    eps_runs = []
    for with_out, with_cl in ((True, True), (False, True), (True, False), (False, False)):
        def call():
            out = Guarded((B, cout, H, W), dev) if with_out else None
            prev, cl, pack = Guarded((B, cout, H, W), dev), Guarded((B, cout, H, W), dev) if with_cl else None, _pack(dev, nbytes)
            N.check(L.llie_final_conv(dtype, *(t.data_ptr() for t in dd), out.ptr if out else None, B, H, W, C, cout, 1, ctypes.byref(cc),
                                      sd.data_ptr(), None if last else nd.data_ptr(), prev.ptr, cl.ptr if cl else None, pack.ptr, nbytes,
                                      _st()), "final_conv")
            torch.cuda.synchronize()
            assert _last() == _final_name(1, dtype), _last()
            return out.cpu("eps") if out else None, prev.cpu("prev"), cl.cpu("clamped") if cl else None
        o, p, c = _twice(call, ("eps", "prev", "clamped"))
        _ratio(p, *step["prev"], R.BAR_STEP, f"step_prev/{tag}")
        if c is not None:
            _ratio(c, *step["clamped"], R.BAR_STEP, f"step_clamped/{tag}")
            assert torch.equal(c, p.clamp(-1.0, 1.0)), "clamped is not clip(prev)"
        if o is not None:
            _ratio(o, eref, eab, esl, R.BAR_FINAL, f"step_eps/{tag}")
            eps_runs.append(o)
    _same(eps_runs[0], eps_runs[1], "the noise prediction with and without `clamped`")


# =============================================================================================
# llie_se_gate (small.hip): the gate from int64 fixed-point totals by each path Run::se_gate can take
SE_P = 324
SE0 = [(0, 64, 6), (0, 192, 48), (0, 384, 96), (0, 512, 128), (0, 768, 24)] + [(d, c, s) for d in H2 for c, s in
                                                                                 ((128, 12), (256, 64), (384, 96), (512, 128))]
SE1 = [(d, c, s) for d in DTYPES for c, s in ((768, 192), (96, 24))]
SE2 = [(d, c, s, b) for d in H2 for c, s, b in ((512, 64, 3), (768, 192, 3), (1024, 512, 3), (512, 64, 33))]


def _se_inputs(B, C, Cs, dtype, key):
    g = _gen("se_gate", key, B, C, Cs, dtype)
    tot = torch.round(torch.randn(B, C, generator=g, dtype=torch.float64) * SE_P * 0.5 * R.SE_FIX).to(torch.int64)  # both signs
    w1, w2 = _rt(torch.randn(Cs, C, generator=g) / math.sqrt(C), dtype), _rt(torch.randn(C, Cs, generator=g) / math.sqrt(Cs), dtype)
    b1, b2 = torch.randn(Cs, generator=g) * 2.5 + 2.5, torch.randn(C, generator=g) * 0.5  # hidden on both sides of 0 and of 6
    return tot, w1, b1, w2, b2


@pytest.mark.parametrize("dtype,C,Cs", SE0, ids=[f"dt{d}-c{c}-s{s}" for d, c, s in SE0])
def test_se_gate_one_launch_vs_float64(dev, dtype, C, Cs):
    """Path 0, se_gate_kernel: Cs off the vector width (6 in fp32, 12 in the 2-byte types: the scalar tail of fc2), Cs > 64 (a second
    pass of the 64 row groups of fc1), more than eight vector steps per row (fc1 at C = 768 in fp32; fc2 at Cs = 128 in every type),
    one, two and three workgroups per image (C <= 384, 512, 768).  The hidden layer never leaves LDS: the gate is compared with the reference's, fc1's
    absolute sum carried through W2.  B = 2.  Measured worst ratio (MI355X, seeds 0..2): 0.64 fp32, 0.66 fp16, 0.56 bf16; bar BAR_SE_GATE = 17."""
    L = N.lib()
    B = 2
    tot, w1, b1, w2, b2 = _se_inputs(B, C, Cs, dtype, 0)
    dd = [t.to(dev) for t in (tot, w1, b1, w2, b2)]

    def call():
        gate = Guarded((B, C), dev)
        N.check(L.llie_se_gate(dtype, dd[0].data_ptr(), SE_P, dd[1].data_ptr(), dd[2].data_ptr(), dd[3].data_ptr(), dd[4].data_ptr(), gate.ptr,
                               B, C, Cs, 0, None, None, _st()), "se_gate")
        torch.cuda.synchronize()
        assert _last() == "se_gate_kernel", _last()
        return (gate.cpu("gate"),)
    (gk,) = _twice(call, ("gate",))
    _, _, (gt, ga, gs) = R.se_totals_ref(dtype, tot, SE_P, w1, b1, w2, b2, 0)
    _ratio(gk, gt, ga, gs, R.BAR_SE_GATE, f"se_gate0/c{C}/s{Cs}/dt{dtype}")


@pytest.mark.parametrize("dtype,C,Cs", SE1, ids=[f"dt{d}-c{c}-s{s}" for d, c, s in SE1])
def test_se_gate_row_pair_vs_float64(dev, dtype, C, Cs):
    """Path 1, se_fc1_kernel + se_fc2_kernel reading the totals (no pool pass), at the first width past se_gate_kernel's range and a
    narrow one; hidden and gate per entry, the gate against the reference fed with the kernel's own hidden.  B = 2 and B = 5 (a
    second pass of four images).  Measured worst ratio (MI355X, seeds 0..2): hidden 0.31, gate 1.36, alike in every type; bar
    BAR_SE_GATE = 17."""
    L = N.lib()
    for B in (2, 5):
        tot, w1, b1, w2, b2 = _se_inputs(B, C, Cs, dtype, 1)
        dd = [t.to(dev) for t in (tot, w1, b1, w2, b2)]

        def call():
            hid, gate = Guarded((B, Cs), dev), Guarded((B, C), dev)
            N.check(L.llie_se_gate(dtype, dd[0].data_ptr(), SE_P, dd[1].data_ptr(), dd[2].data_ptr(), dd[3].data_ptr(), dd[4].data_ptr(),
                                   gate.ptr, B, C, Cs, 1, hid.ptr, None, _st()), "se_gate")
            torch.cuda.synchronize()
            assert _last() == "se_fc1_kernel+se_fc2_kernel", _last()
            return hid.cpu("hidden"), gate.cpu("gate")
        hk, gk = _twice(call, ("hidden", "gate"))
        _, (h, ha, hs), (gt, ga, gs) = R.se_totals_ref(dtype, tot, SE_P, w1, b1, w2, b2, 1, hidden=hk)
        _ratio(hk, h, ha, hs, R.BAR_SE_GATE, f"se_gate1_hidden/c{C}/s{Cs}/b{B}/dt{dtype}")
        _ratio(gk, gt, ga, gs, R.BAR_SE_GATE, f"se_gate1/c{C}/s{Cs}/b{B}/dt{dtype}")


@pytest.mark.parametrize("dtype,C,Cs,B", SE2, ids=[f"dt{d}-c{c}-s{s}-b{b}" for d, c, s, b in SE2])
def test_se_gate_mfma_pair_vs_float64(dev, dtype, C, Cs, B):
    """Path 2, se_fc1_mfma_kernel + se_fc2_mfma_kernel: two, three and four K slices per column block, one to eight k-steps per wave
    of fc2, B = 3 (29 masked rows) and B = 33 (a second batch block with one live row).  `pre` is compared as a 2^-32 fixed-point
    number, the gate against the reference fed with the kernel's own `pre`; one row of `pre` past the batch keeps its prefill (the
    call zero-fills batch x Cs entries and the kernel masks the rest).  Measured worst ratio (MI355X, seeds 0..2), fp16 / bf16: pre
    0.29 / 0.27, gate 1.63 / 1.32; bar BAR_SE_GATE = 17."""
    L = N.lib()
    tot, w1, b1, w2, b2 = _se_inputs(B, C, Cs, dtype, 2)
    dd = [t.to(dev) for t in (tot, w1, b1, w2, b2)]

    def call():
        pre, gate = Guarded((B + 1, Cs), dev, torch.int64, fill=77), Guarded((B, C), dev)
        N.check(L.llie_se_gate(dtype, dd[0].data_ptr(), SE_P, dd[1].data_ptr(), dd[2].data_ptr(), dd[3].data_ptr(), dd[4].data_ptr(), gate.ptr,
                               B, C, Cs, 2, None, pre.ptr, _st()), "se_gate")
        torch.cuda.synchronize()
        assert _last() == "se_fc1_mfma_kernel+se_fc2_mfma_kernel", _last()
        return pre.cpu("pre"), gate.cpu("gate")
    pk, gk = _twice(call, ("pre", "gate"))
    assert (pk[B] == 77).all(), "pre written past the batch"
    _, (p, pa, ps), (gt, ga, gs) = R.se_totals_ref(dtype, tot, SE_P, w1, b1, w2, b2, 2, pre=pk[:B])
    _ratio(pk[:B].double() / R.SE_PRE, p, pa, ps, R.BAR_SE_GATE, f"se_gate2_pre/c{C}/s{Cs}/b{B}/dt{dtype}")
    _ratio(gk, gt, ga, gs, R.BAR_SE_GATE, f"se_gate2/c{C}/s{Cs}/b{B}/dt{dtype}")


# =============================================================================================
# llie_affine_add (small.hip)
AFF_PARAMS = [(d, c, p, f) for d in DTYPES for c in (32, 96, 768) for p in (64, 25, 100, 65) for f in (True, False)]


@pytest.mark.parametrize("dtype,C,P,full", AFF_PARAMS, ids=[f"dt{d}-c{c}-p{p}-{'full' if f else 'bare'}" for d, c, p, f in AFF_PARAMS])
def test_affine_add_vs_float64(dev, dtype, C, P, full):
    """llie_affine_add: a full 64-row tile, a partial one (25), one of each (100 = 64 + 36) and a one-row tile (65: fewer rows than
    waves); 32, 96 and 768 channels (768: more vectors per row than lanes in every type); with residual and statistics, and with
    neither.  B = 2.  Measured worst ratio (MI355X, seeds 0..2), output: 0 in every type (inside the ulp of the stored value), bar
    BAR_AFFINE = 2 from the kernel's two further fp32 roundings; statistics: 1.73 / 2.15 / 1.17, bar BAR_AFFINE_STATS = 22."""
    L = N.lib()
    B = 2
    g = _gen("affine", dtype, C, P)
    x, res = _rt(torch.randn(B, P, C, generator=g) * 1.5, dtype), _rt(torch.randn(B, P, C, generator=g), dtype)
    sc, sh = torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g) * 0.7
    xd, rd, scd, shd = (t.to(dev) for t in (x, res, sc, sh))
    nt = (P + 63) // 64

    def call():
        y = Guarded((B, P, C), dev, TDT[dtype])
        slab = _slab(dev, B, nt, 2, C) if full else None
        N.check(L.llie_affine_add(dtype, xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), rd.data_ptr() if full else None, y.ptr,
                                  slab.ptr if full else None, B * P, C, P, _st()), "affine_add")
        torch.cuda.synchronize()
        return y.cpu("affine y"), _split(slab.cpu("affine stats"), B, nt, "affine stats") if full else None
    y, s = _twice(call, ("y", "stats"))
    tag = f"c{C}/p{P}/dt{dtype}/{'full' if full else 'bare'}"
    _ratio(y, *R.affine_add_ref(dtype, x, sc, sh, res if full else None), R.BAR_AFFINE, f"affine/{tag}")
    if full:
        _ratio(s, *R.tile_stats_ref(y, 64), R.BAR_AFFINE_STATS, f"affine_stats/{tag}")


# =============================================================================================
# llie_nchw_to_nhwc / llie_nhwc_to_nchw (small.hip)
CVT_PARAMS = [(d, t, p) for d in DTYPES for t in ((32, 32, 0), (64, 96, 32), (32, 96, 64)) for p in (64, 192)]
CVT_IDS = [f"dt{d}-c{t[0]}of{t[1]}at{t[2]}-p{p}" for d, t, p in CVT_PARAMS]


@pytest.mark.parametrize("dtype,tri,P", CVT_PARAMS, ids=CVT_IDS)
def test_nchw_to_nhwc_bits_and_slab(dev, dtype, tri, P):
    """Channels [coff, coff + C) of a fp32 [B][Csrc][P] tensor: the NHWC values are round_T(x) bit for bit; the slab ([B][P / 64][2][C],
    with and without) against the sums of the stored values.  Measured worst ratio (MI355X, seeds 0..2): 5.76 fp32, 7.77 fp16, 4.78
    bf16 (one thread adds a tile's 64 pixels one after the other); bar BAR_CONVERT_STATS = 78."""
    L = N.lib()
    B, (C, Csrc, coff) = 2, tri
    x = torch.randn(B, Csrc, P, generator=_gen("cvt", dtype, tri, P)) * 1.5
    xd = x.to(dev)
    want = _rt(x[:, coff:coff + C], dtype).permute(0, 2, 1).contiguous()
    for full in (True, False):
        def call():
            y = Guarded((B, P, C), dev, TDT[dtype])
            slab = _slab(dev, B, P // 64, 2, C) if full else None
            N.check(L.llie_nchw_to_nhwc(dtype, xd.data_ptr(), y.ptr, slab.ptr if full else None, B, C, P, Csrc, coff, _st()), "nchw_to_nhwc")
            torch.cuda.synchronize()
            return y.cpu("nhwc"), _split(slab.cpu("nhwc stats"), B, P // 64, "nhwc stats") if full else None
        y, s = _twice(call, ("y", "stats"))
        _same(y, want, "nchw_to_nhwc against round_T(x)")
        if full:
            _ratio(s, *R.tile_stats_ref(y, 64), R.BAR_CONVERT_STATS, f"nhwc_stats/c{C}of{Csrc}at{coff}/p{P}/dt{dtype}")


@pytest.mark.parametrize("dtype,tri,P", CVT_PARAMS, ids=CVT_IDS)
def test_nhwc_to_nchw_bits_and_untouched_channels(dev, dtype, tri, P):
    """The way back: channels [coff, coff + C) of the fp32 [B][Cdst][P] destination are float(x) bit for bit, every other channel keeps
    its NaN prefill."""
    L = N.lib()
    B, (C, Cdst, coff) = 2, tri
    x = _rt(torch.randn(B, P, C, generator=_gen("cvt_back", dtype, tri, P)) * 1.5, dtype)
    xd = x.to(dev)

    def call():
        y = Guarded((B, Cdst, P), dev)
        N.check(L.llie_nhwc_to_nchw(dtype, xd.data_ptr(), y.ptr, B, C, P, Cdst, coff, _st()), "nhwc_to_nchw")
        torch.cuda.synchronize()
        return (y.cpu("nchw"),)
    (y,) = _twice(call, ("y",))
    _same(y[:, coff:coff + C].contiguous(), x.float().permute(0, 2, 1).contiguous(), "nhwc_to_nchw against float(x)")
    assert torch.isnan(y[:, :coff]).all() and torch.isnan(y[:, coff + C:]).all(), "channels outside [coff, coff + C) written"


# =============================================================================================
# llie_pw_gemm_dot (gemm.hip): the epilogue the backward pass uses, one case per tile class
def _pick(path, cfg):
    return next(c for c in FK.GEMM_CASES if c.path == path and c.cfg == cfg)


DOT_CASES = [_pick("bk128", "128, 128, 2, 2, 128"), _pick("bk64", "128, 32, 4, 1, 64"), _pick("ktail", "128, 64, 2, 2, 64"),
             _pick("bk32f", "128, 128, 2, 2, 32"), _pick("bm64", "64, 64, 2, 2, 32"), _pick("ragged", "64, 32, 2, 1, 32")]
DOT_PARAMS = [(c, d) for c in DOT_CASES for d in c.dts]


@pytest.mark.parametrize("case,dtype", DOT_PARAMS, ids=[f"{c.name}-dt{d}" for c, d in DOT_PARAMS])
def test_pw_gemm_dot_vs_float64(dev, case, dtype):
    """llie_pw_gemm_dot on one of test_pw_gemm_vs_float64's cases per tile class (BK 128, BK 64 with BN 32, KTAIL, the fp32 BK 32 form,
    64-row tiles, ragged tiles): the output as there (BAR_GEMM), and both halves of the slab -- (sum out * dot, sum out) per tile --
    against the stored output and `dot`.  Measured worst ratio (MI355X, seeds 0..2), slab: 0.84 fp32, 0.57 fp16, 0.37 bf16, bar
    BAR_GEMM_DOT = 9; output: 4.25 / 0.15 / 0.05 under BAR_GEMM = 50."""
    L = N.lib()
    c = case
    xs, tabs, lds, w, bias, dot = FK._gemm_inputs(c.segs, c.n, c.p, c.B, dtype, c.name)  # the residual draw serves as `dot`
    d = lambda t: t.to(dev) if t is not None else None  # noqa: E731
    xd, tabd, wd, bd, dd = [d(x) for x in xs], [(d(a), d(b)) for a, b in tabs], d(w), d(bias), d(dot)
    rows = int(L.llie_pw_gemm_tile_rows(c.p))
    nt = (c.p + rows - 1) // rows
    arr = (N.GemmSeg * len(c.segs))()
    for i, ((ch, act, aff), x, (sc, sh)) in enumerate(zip(c.segs, xd, tabd)):
        arr[i] = N.GemmSeg(x.data_ptr(), ch, _ptr(sc), _ptr(sh), lds[i] if aff else 0, act)

    def call():
        out, slab = Guarded((c.B, c.p, c.n), dev, TDT[dtype]), _slab(dev, c.B, nt, 2, c.n)
        N.check(L.llie_pw_gemm_dot(dtype, arr, len(c.segs), wd.data_ptr(), bd.data_ptr(), dd.data_ptr(), out.ptr, slab.ptr, c.B * c.p, c.n,
                                   c.p, _st()), "pw_gemm_dot")
        torch.cuda.synchronize()
        assert _last() == f"pw_gemm_kernel<{TNAME[dtype]}, {c.cfg}>", _last()
        return out.cpu("gemm out"), _split(slab.cpu("gemm dot stats"), c.B, nt, "gemm dot stats")
    o, s = _twice(call, ("out", "stats"))
    cut = [(sc[:, :ch] if sc is not None else None, sh[:, :ch] if sh is not None else None) for (ch, _, _), (sc, sh) in zip(c.segs, tabs)]
    _ratio(o, *R.pw_gemm_ref(dtype, xs, [sg[1] for sg in c.segs], cut, w, bias, None), R.BAR_GEMM, f"gemm_dot_out/{c.name}/dt{dtype}")
    _ratio(s, *R.gemm_dot_stats_ref(o, dot, rows), R.BAR_GEMM_DOT, f"gemm_dot/{c.name}/dt{dtype}")


# =============================================================================================
# refusals: every contract clause of every new entry; nothing may be written
def _refused(calls, bufs, ok=(N.ERR_ARG,)):
    before = [b.clone() for b in bufs]
    for what, rc in calls:
        assert rc in ok, (what, rc)
    torch.cuda.synchronize()
    for a, b in zip(before, bufs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "a refused call changed a buffer"


def test_init_conv_refusals(dev):
    """NULL tensors, x1 without c1 and c1 without x1, c0 < 1, more than 8 input channels, H or W off the multiples of 8, Cout off the
    multiples of 32, the MFMA kernel in fp32, use_mfma outside {0, 1}, a short or misaligned pack, a dtype outside 0..2."""
    L = N.lib()
    x = torch.full((2 * 8 * 16 * 16,), NAN, device=dev)
    out = torch.full((2 * 16 * 16 * 64,), NAN, device=dev)
    nb = int(L.llie_init_conv_pack_bytes(6, 32))
    pack = torch.full((nb // 4 + 4,), NAN, device=dev)
    p, o, k = x.data_ptr(), out.data_ptr(), pack.data_ptr()

    def call(dtype=1, x0=p, c0=3, x1=p, c1=3, w=p, b=p, y=o, H=16, W=16, co=32, mfma=1, pk=k, n=nb, B=2):
        return L.llie_init_conv(dtype, x0, c0, x1, c1, w, b, y, None, B, H, W, co, mfma, pk, n, _st())
    bad = [dict(x0=None), dict(w=None), dict(b=None), dict(y=None), dict(pk=None), dict(x1=None), dict(c1=0), dict(c0=0), dict(c0=5, c1=4),
           dict(H=12), dict(W=20), dict(co=48), dict(co=0), dict(dtype=0), dict(mfma=2), dict(n=nb - 16), dict(pk=k + 4), dict(dtype=3), dict(B=0)]
    _refused([(kw, call(**kw)) for kw in bad], [x, out, pack])
    assert L.llie_init_conv_tiles(12, 16, 0) == N.ERR_ARG and L.llie_init_conv_pack_bytes(9, 32) == N.ERR_ARG
    assert L.llie_init_conv_pack_bytes(6, 48) == N.ERR_ARG
    x.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out.view(torch.float16)[:2 * 16 * 16 * 32]).any()


def test_final_conv_refusals(dev):
    """NULL tensors, C off the multiples of 32, Cout outside 1..4, H or W off the multiples of 8, the MFMA kernel in fp32, a short or
    misaligned pack; the step on the VALU kernel, without sample or prev, without noise unless is_last; without the step: no out, or
    one of the step's tensors given."""
    L = N.lib()
    x = torch.full((2 * 16 * 16 * 64,), NAN, device=dev)
    out = torch.full((2 * 4 * 16 * 16,), NAN, device=dev)
    nb = int(L.llie_final_conv_pack_bytes(64))
    pack = torch.full((nb // 4 + 4,), NAN, device=dev)
    p, o, k = x.data_ptr(), out.data_ptr(), pack.data_ptr()
    cc, cl = N.StepCoef(0.8, 0.6, 0.9, 0.43, 0, 0, 0), N.StepCoef(0.8, 0.6, 0.9, 0.43, 1, 0, 0)

    def call(dtype=1, xin=p, sc=p, w=p, b=p, y=o, H=16, W=16, C=64, co=3, mfma=1, coef=None, sample=None, noise=None, prev=None, clamped=None,
             pk=k, n=nb):
        return L.llie_final_conv(dtype, xin, sc, sc, w, b, y, 2, H, W, C, co, mfma, ctypes.byref(coef) if coef else None, sample, noise, prev,
                                 clamped, pk, n, _st())
    bad = [dict(xin=None), dict(sc=None), dict(w=None), dict(b=None), dict(pk=None), dict(C=48), dict(C=0), dict(co=5), dict(co=0), dict(H=12),
           dict(W=20), dict(dtype=0), dict(dtype=3), dict(mfma=-1), dict(n=nb - 16), dict(pk=k + 4), dict(y=None), dict(sample=o), dict(prev=o),
           dict(clamped=o), dict(noise=o), dict(coef=cc, mfma=0, sample=o, noise=o, prev=o), dict(coef=cc, noise=o, prev=o),
           dict(coef=cc, sample=o, noise=o), dict(coef=cc, sample=o, prev=o)]
    _refused([(kw, call(**kw)) for kw in bad], [x, out, pack])
    assert L.llie_final_conv_pack_bytes(48) == N.ERR_ARG
    prev = torch.full((2 * 3 * 16 * 16,), NAN, device=dev)
    x.zero_()
    assert call(coef=cl, y=None, sample=p, prev=prev.data_ptr()) == 0  # no noise when is_last, no out
    torch.cuda.synchronize()
    assert not torch.isnan(prev).any() and torch.isnan(out).all()


def test_se_gate_refusals(dev):
    """NULL tensors, sizes < 1, a path outside 0..2; path 0: C off 16 vectors, more than 48 KiB of LDS; path 1: no hidden scratch, rows
    beyond 4096; path 2: fp32, no pre scratch, C or Cs outside the MFMA pair's shapes."""
    L = N.lib()
    t = torch.full((64 * 1024,), NAN, device=dev)
    p = t.data_ptr()

    def call(dtype=1, tot=p, w1=p, gate=p, P=64, B=2, C=512, Cs=64, path=0, hid=p, pre=p):
        return L.llie_se_gate(dtype, tot, P, w1, p, p, p, gate, B, C, Cs, path, hid, pre, _st())
    bad = [dict(tot=None), dict(w1=None), dict(gate=None), dict(P=0), dict(B=0), dict(C=0), dict(Cs=0), dict(path=3), dict(path=-1), dict(dtype=3),
           dict(C=192), dict(dtype=0, C=96), dict(C=12288, Cs=64), dict(path=1, hid=None), dict(path=1, C=4224), dict(path=2, dtype=0),
           dict(path=2, pre=None), dict(path=2, C=384), dict(path=2, C=640), dict(path=2, Cs=32), dict(path=2, Cs=96), dict(path=2, Cs=576)]
    _refused([(kw, call(**kw)) for kw in bad], [t])


def test_affine_add_and_converter_refusals(dev):
    """affine_add: NULL tensors, M not a multiple of P, C off the multiples of 8 or beyond 2048; the converters: NULL tensors, C off
    the multiples of 32, P off the multiples of 64, a negative offset, channels [coff, coff + C) outside the other side's count."""
    L = N.lib()
    t = torch.full((2 * 64 * 96,), NAN, device=dev)
    p = t.data_ptr()

    def aff(dtype=1, x=p, sc=p, y=p, M=128, C=32, P=64):
        return L.llie_affine_add(dtype, x, sc, sc, None, y, None, M, C, P, _st())

    def fwd(dtype=1, x=p, y=p, B=2, C=32, P=64, Cs=96, off=32):
        return L.llie_nchw_to_nhwc(dtype, x, y, None, B, C, P, Cs, off, _st())

    def back(dtype=1, x=p, y=p, B=2, C=32, P=64, Cd=96, off=32):
        return L.llie_nhwc_to_nchw(dtype, x, y, B, C, P, Cd, off, _st())
    calls = [(("aff", kw), aff(**kw)) for kw in (dict(x=None), dict(sc=None), dict(y=None), dict(M=100), dict(C=12), dict(C=4096), dict(P=0),
                                                 dict(M=0), dict(dtype=3), dict(dtype=-1))]
    for name, f in (("fwd", fwd), ("back", back)):
        calls += [((name, kw), f(**kw)) for kw in (dict(x=None), dict(y=None), dict(B=0), dict(C=48), dict(C=0), dict(P=100), dict(P=0), dict(off=-32),
                                                   dict(off=80), dict(C=64, off=64), dict(dtype=3))]
    _refused(calls, [t])


def test_pw_gemm_dot_refusals(dev):
    """No dot, no slab, llie_pw_gemm's own segment clauses (LLIE_ERR_ARG), and the launcher's shape contract (its invalid-value status,
    which the entry reports as LLIE_ERR_SHAPE)."""
    L = N.lib()
    x = torch.full((256 * 128,), NAN, dtype=torch.float16, device=dev)
    s = torch.full((2 * 2 * 128,), NAN, device=dev)
    p, q = x.data_ptr(), s.data_ptr()

    def call(seg=(64, 0, True, True, 64), dot=p, stats=q, n=64, M=256, P=128, w=p):
        ch, act, sc, sh, ld = seg
        arr = (N.GemmSeg * 1)(N.GemmSeg(p, ch, q if sc else None, q if sh else None, ld, act))
        return L.llie_pw_gemm_dot(1, arr, 1, w, None, dot, p, stats, M, n, P, _st())
    bad = [dict(dot=None), dict(stats=None), dict(w=None), dict(seg=(64, 2, True, True, 64)), dict(seg=(64, 1, False, False, 0)),
           dict(seg=(64, 0, True, True, 32)), dict(n=48), dict(seg=(48, 0, True, True, 48)), dict(M=200)]
    _refused([(kw, call(**kw)) for kw in bad], [x, s], ok=(N.ERR_ARG, N.ERR_SHAPE))
