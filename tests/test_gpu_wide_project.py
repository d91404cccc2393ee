"""The wide decoder blocks without h2 (irbx.hip, section 3: dwconv3x3_pool + dwconv3x3_project, knob "wide_project"), through their
entry points and once through the engine.

Layers: 192 -> 64 (hid 768) as segments 128 + 64 and as one segment, 384 -> 128 (hid 1536) as 256 + 128; fp16 and bf16; B = 3.
Maps: 16 x 32 (2 x 2 tiles of 8 x 16: every tile touches a corner) and 24 x 48 (3 x 3 tiles, one interior).  A workgroup of
dwconv3x3_project owns exactly one tile and one of dwconv3x3_pool eight image rows, so no launch walks further.

  * pool totals: exact on dyadic operands (the method of test_gpu_expand_pool_border.py), and on random operands at most twice as
    far from float64 as the totals dwconv3x3 leaves on the same inputs (the rule of test_expand_pool_totals);
  * y against float64 from the definition, next to the unfused pair (llie_dwconv3x3_ex + llie_pw_gemm) on the same operands: the
    new kernel's maximum error may be at most twice the pair's.  Both round twice between h1 and y, at different places: the new
    path the activated h1 and the gated weights T(6 w gate), the pair h2 and gate * h2;
  * dyadic operands: y and every slab entry exact; gate = 0 gives the shortcut alone and equals zeroed depthwise weights;
  * reruns bit-equal, an image alone equals its row of the batch, guard regions around y, the slab and the totals intact;
  * the launchers refuse what the predicate refuses, without launching;
  * one 192 -> 64 block through llie_module_forward: the launch sequence at both knob settings, and the outputs.
"""
import importlib
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")
U = importlib.import_module("cv-diffusion-model_amd.unet")

DTYPES = [(1, torch.float16), (2, torch.bfloat16)]
LAYERS = [(128, 64, 64), (192, 0, 64), (256, 128, 128)]      # (c0, c1, cout); Chid = 4 (c0 + c1)
MAPS = [(16, 32), (24, 48)]
B = 3
FIX = float(2 ** 24)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def depthwise64(a, w9):
    """a [B][H][W][C] float64, w9 [9][C] float64 tap-major -> zero-padded depthwise 3x3, [B][H][W][C]"""
    return R.dw_from_padded(R.pad_zero(a), w9)[0]


def random_inputs(c0, c1, cout, H, W, tdt):
    """Operands as the engine hands them over (CPU): h1 and x in T, norm2's tables already / 6, fp32 depthwise weights [9][Chid],
    a gate in (0, 1), the K-concatenated project | skip matrix in T."""
    cin = c0 + c1
    chid = 4 * cin
    g = torch.Generator().manual_seed(cin * 1000 + c0 + 7 * H + W)
    t = {}
    t["h1"] = (2.0 * torch.randn(B, H, W, chid, generator=g)).to(tdt)
    t["sc"] = (0.5 + torch.rand(B, chid, generator=g)) / 6
    t["sh"] = (1.0 + 2.0 * torch.rand(B, chid, generator=g)) / 6
    t["wd"] = 0.3 * torch.randn(9, chid, generator=g)
    t["gate"] = torch.rand(B, chid, generator=g)
    t["x"] = torch.randn(B, H, W, cin, generator=g).to(tdt)
    t["wps"] = (torch.randn(cout, chid + cin, generator=g) / math.sqrt(chid + cin)).to(tdt)
    return t


def exact_inputs(c0, c1, cout, H, W, tdt):
    """Dyadic operands: h1 in {-1, 0, 1, 2} under the affine t -> 2^20 t - 2^19 gives a in {0, 1}; depthwise weights are multiples of
    1/2 without zero, so 6 w is -6, -3, 3 or 6; the gate is 1; project rows hold eight and skip rows four entries of +-1; x in
    {-1, 0, 1, 2}.  Every product and sum of either kernel is then an integer: h2 of at most 54, y of a few hundred at most."""
    cin = c0 + c1
    chid = 4 * cin
    g = torch.Generator().manual_seed(cin * 77 + c0 + 3 * H + W)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
    t = {}
    t["h1"] = ri(-1, 2, B, H, W, chid).to(tdt)
    t["sc"] = torch.full((B, chid), 2.0 ** 20)
    t["sh"] = torch.full((B, chid), -2.0 ** 19)
    t["wd"] = torch.tensor([-1.0, -0.5, 0.5, 1.0])[ri(0, 3, 9, chid)]
    t["gate"] = torch.ones(B, chid)
    t["x"] = ri(-1, 2, B, H, W, cin).to(tdt)
    wps = torch.zeros(cout, chid + cin)
    for r in range(cout):
        wps[r, torch.randperm(chid, generator=g)[:8]] = (2.0 * ri(0, 1, 8) - 1.0)
        wps[r, chid + torch.randperm(cin, generator=g)[:4]] = (2.0 * ri(0, 1, 4) - 1.0)
    t["wps"] = wps.to(tdt)
    return t


def ref64(t, tdt, round_weights=False):
    """float64 from the definition: (pool totals [B][Chid], y [B][H][W][cout]); a is not rounded.  round_weights: the depthwise
    weights as the kernels stage them, T(6 w) (the totals' reference, as in test_expand_pool_totals), else exact"""
    chid = t["h1"].shape[-1]
    a = (t["h1"].double() * t["sc"].double()[:, None, None, :] + t["sh"].double()[:, None, None, :]).clamp(0, 1)
    w6 = (6 * t["wd"]).to(tdt).double() if round_weights else 6 * t["wd"].double()
    h2 = depthwise64(a, w6)
    wp, wsk = t["wps"][:, :chid].double(), t["wps"][:, chid:].double()
    y = (h2 * t["gate"].double()[:, None, None, :]) @ wp.t() + t["x"].double() @ wsk.t()
    return h2.sum((1, 2)), y


_cases = {}


def case(kind, c0, c1, cout, H, W, tdt):
    """operands and float64 references, computed once per case and shared"""
    key = (kind, c0, c1, cout, H, W, tdt)
    if key not in _cases:
        t = (exact_inputs if kind == "exact" else random_inputs)(c0, c1, cout, H, W, tdt)
        tot_ref, y_ref = ref64(t, tdt, round_weights=True)
        if kind != "exact":
            y_ref = ref64(t, tdt)[1]
        _cases[key] = (t, tot_ref, y_ref)
    return _cases[key]


class GuardedI64:
    """int64 totals between canaries, zeroed (the kernels add)"""

    def __init__(self, shape, dev):
        n = int(math.prod(shape))
        self.full = torch.full((n + 32,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        self.v = self.full[16:16 + n].view(shape)
        self.v.zero_()

    def cpu(self):
        f = self.full.cpu()
        assert (f[:16] == 0x5A5A5A5A5A5A).all() and (f[-16:] == 0x5A5A5A5A5A5A).all(), "pool totals: wrote outside the buffer"
        return f[16:-16].view(self.v.shape)


def run_pool(dev, dtype, t, b0=0, b1=B, old=False):
    """pool totals [b][Chid] of images [b0, b1): dwconv3x3_pool, or (old) what dwconv3x3 leaves next to its h2"""
    L = N.lib()
    nb = b1 - b0
    _, H, W, chid = t["h1"].shape
    d = {k: t[k][b0:b1].contiguous().to(dev) for k in ("h1", "sc", "sh")}
    wd = t["wd"].to(dev)
    tot = GuardedI64((nb, chid), dev)
    if old:
        h2 = torch.empty_like(d["h1"])
        N.check(L.llie_dwconv3x3_ex(dtype, d["h1"].data_ptr(), h2.data_ptr(), d["sc"].data_ptr(), d["sh"].data_ptr(), wd.data_ptr(), None,
                                    tot.v.data_ptr(), 1, nb, H, W, chid, _st()), "dwconv3x3_ex")
    else:
        N.check(L.llie_dwconv3x3_pool(dtype, d["h1"].data_ptr(), d["sc"].data_ptr(), d["sh"].data_ptr(), wd.data_ptr(), tot.v.data_ptr(),
                                      nb, H, W, chid, _st()), "dwconv3x3_pool")
    torch.cuda.synchronize()
    return tot.cpu()


def run_project(dev, dtype, tdt, t, c0, c1, cout, b0=0, b1=B, gate=None, wd=None):
    """(y [b][H][W][cout], slab [b][tiles][2][cout]) of images [b0, b1) from dwconv3x3_project, outputs NaN-filled and guarded"""
    L = N.lib()
    nb = b1 - b0
    _, H, W, chid = t["h1"].shape
    d = {k: t[k][b0:b1].contiguous().to(dev) for k in ("h1", "sc", "sh")}
    gd = (t["gate"] if gate is None else gate)[b0:b1].contiguous().to(dev)
    wdd = (t["wd"] if wd is None else wd).to(dev)
    x0 = t["x"][b0:b1, ..., :c0].contiguous().to(dev)
    x1 = t["x"][b0:b1, ..., c0:].contiguous().to(dev) if c1 else None
    wps = t["wps"].to(dev)
    nt = int(L.llie_irbx_project_tiles(H, W))
    y = R.Guarded((nb, H, W, cout), dev, tdt)
    slab = R.Guarded((nb, nt, 2, cout), dev)
    N.check(L.llie_dwconv3x3_project(dtype, d["h1"].data_ptr(), d["sc"].data_ptr(), d["sh"].data_ptr(), wdd.data_ptr(), gd.data_ptr(),
                                     x0.data_ptr(), c0, x1.data_ptr() if c1 else None, c1, wps.data_ptr(), wps.shape[1], cout, y.ptr, slab.ptr,
                                     nb, H, W, _st()), "dwconv3x3_project")
    torch.cuda.synchronize()
    yc, sc = y.cpu("y"), slab.cpu("slab")
    assert torch.isfinite(yc.float()).all() and torch.isfinite(sc).all(), "entries left unwritten"
    return yc, sc


def run_unfused(dev, dtype, tdt, t, c0, c1, cout):
    """y of the unfused pair on the same operands: dwconv3x3 (s6) writes h2, the project GEMM gates it and adds the skip segments"""
    L = N.lib()
    _, H, W, chid = t["h1"].shape
    P = H * W
    d = {k: t[k].to(dev) for k in ("h1", "sc", "sh", "wd", "gate", "wps")}
    x0 = t["x"][..., :c0].contiguous().to(dev)
    x1 = t["x"][..., c0:].contiguous().to(dev) if c1 else None
    h2 = torch.empty_like(d["h1"])
    N.check(L.llie_dwconv3x3_ex(dtype, d["h1"].data_ptr(), h2.data_ptr(), d["sc"].data_ptr(), d["sh"].data_ptr(), d["wd"].data_ptr(), None,
                                None, 1, B, H, W, chid, _st()), "dwconv3x3_ex")
    segs = [N.GemmSeg(h2.data_ptr(), chid, d["gate"].data_ptr(), None, chid, 0), N.GemmSeg(x0.data_ptr(), c0, None, None, 0, 0)]
    if c1:
        segs.append(N.GemmSeg(x1.data_ptr(), c1, None, None, 0, 0))
    arr = (N.GemmSeg * len(segs))(*segs)
    y = torch.empty(B, H, W, cout, dtype=tdt, device=dev)
    N.check(L.llie_pw_gemm(dtype, arr, len(segs), d["wps"].data_ptr(), None, None, y.data_ptr(), None, B * P, cout, P, _st()), "pw_gemm")
    torch.cuda.synchronize()
    return y.cpu()


def tile_sums(y, cout):
    """[B][H][W][cout] stored y -> [B][tiles][2][cout] float64 (sum, sum of squares) per 8 x 16 tile, tiles row-major"""
    q = y.double()
    b, H, W, _ = q.shape
    q = q.view(b, H // 8, 8, W // 16, 16, cout).permute(0, 1, 3, 2, 4, 5).reshape(b, (H // 8) * (W // 16), 128, cout)
    return torch.stack([q.sum(2), (q * q).sum(2)], 2)


# ------------------------------------------------------------------ 1. the pool pass
@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("chid", [768, 1536])
def test_pool_totals_exact(dev, dtype, tdt, H, W, chid):
    """a in {0, 1}, 6 w an integer: every fp32 operation is exact, so pool_tot must EQUAL 2^24 x the float64 total of the
    definition (the sum of the depthwise output), every entry.  Reruns are bit-equal and an image alone gives its row."""
    c0, c1, cout = (128, 64, 64) if chid == 768 else (256, 128, 128)
    t, ref, _ = case("exact", c0, c1, cout, H, W, tdt)
    assert torch.equal(ref, ref.round()) and ref.abs().max().item() < 2 ** 24 and (ref != 0).any()
    got = run_pool(dev, dtype, t)
    bad = (got != (ref * FIX).to(torch.int64)).nonzero()
    print(f"|total|max {ref.abs().max().item():.0f}, totals that differ: {bad.shape[0]}")
    assert bad.shape[0] == 0, f"{bad.shape[0]} totals differ; first (image, channel) {bad[:4].tolist()}"
    assert torch.equal(got, run_pool(dev, dtype, t))
    for i in range(B):
        assert torch.equal(got[i:i + 1], run_pool(dev, dtype, t, i, i + 1)), i


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("chid", [768, 1536])
def test_pool_totals_random(dev, dtype, tdt, H, W, chid):
    """The rule of test_expand_pool_totals: at most twice as far from float64 as the totals dwconv3x3 leaves on the same inputs (same
    rounding points, another summation order); reruns bit-equal, an image alone gives the bits of its row."""
    c0, c1, cout = (128, 64, 64) if chid == 768 else (256, 128, 128)
    t, ref, _ = case("random", c0, c1, cout, H, W, tdt)
    new, old = run_pool(dev, dtype, t), run_pool(dev, dtype, t, old=True)
    err_new = (new.double() / FIX - ref).abs().max().item()
    err_old = (old.double() / FIX - ref).abs().max().item()
    msg = f"max |total - float64|: dwconv3x3_pool {err_new:.3e}, dwconv3x3 {err_old:.3e}, |ref|max {ref.abs().max().item():.3e}"
    print(msg)
    assert err_new <= 2 * err_old, msg
    assert torch.equal(new, run_pool(dev, dtype, t))
    for i in range(B):
        assert torch.equal(new[i:i + 1], run_pool(dev, dtype, t, i, i + 1)), i


# ------------------------------------------------------------------ 2. the depthwise-project pass
@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("c0,c1,cout", LAYERS)
def test_project_vs_float64_and_the_unfused_pair(dev, dtype, tdt, H, W, c0, c1, cout):
    """max |y - float64| of dwconv3x3_project at most twice that of dwconv3x3 + pw_gemm on the same h1, tables, gate and weights;
    reruns bit-equal, an image alone equals its row of the batch (y and slab), guards intact (run_project)."""
    t, _, ref = case("random", c0, c1, cout, H, W, tdt)
    y, slab = run_project(dev, dtype, tdt, t, c0, c1, cout)
    y_old = run_unfused(dev, dtype, tdt, t, c0, c1, cout)
    err_new = (y.double() - ref).abs().max().item()
    err_old = (y_old.double() - ref).abs().max().item()
    msg = (f"Y_ERR {c0}+{c1}->{cout} {H}x{W} {str(tdt)[6:]}: max |y - float64| dwconv3x3_project {err_new:.3e}, dwconv3x3 + pw_gemm "
           f"{err_old:.3e}, |ref|max {ref.abs().max().item():.3e}")
    print(msg)
    assert err_new <= 2 * err_old, msg
    # the slab against the stored y: fp32 sums of 128 values in a fixed order
    ts = tile_sums(y, cout)
    assert torch.allclose(slab.double(), ts, rtol=1e-5, atol=1e-4 * max(1.0, ts.abs().max().item()))
    y2, slab2 = run_project(dev, dtype, tdt, t, c0, c1, cout)
    assert torch.equal(R._bits(y), R._bits(y2)) and torch.equal(slab, slab2)
    for i in range(B):
        yi, si = run_project(dev, dtype, tdt, t, c0, c1, cout, i, i + 1)
        assert torch.equal(R._bits(y[i:i + 1]), R._bits(yi)) and torch.equal(slab[i:i + 1], si), i


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("c0,c1,cout", LAYERS)
def test_project_exact_gate_zero_and_slab(dev, dtype, tdt, H, W, c0, c1, cout):
    """Dyadic operands: y is an integer of at most 256, so the stored y equals T(float64 y) and every slab entry equals the sums
    of its own tile's y, exactly.  gate = 0 gives the shortcut alone -- exact on these integer operands -- and so do zeroed
    depthwise weights, bit for bit in y and slab."""
    t, _, ref = case("exact", c0, c1, cout, H, W, tdt)
    chid = 4 * (c0 + c1)
    assert torch.equal(ref, ref.round()) and ref.abs().max().item() <= 256
    y, slab = run_project(dev, dtype, tdt, t, c0, c1, cout)
    assert torch.equal(y.double(), ref.float().to(tdt).double())
    assert torch.equal(slab.double(), tile_sums(y, cout))
    y0, slab0 = run_project(dev, dtype, tdt, t, c0, c1, cout, gate=torch.zeros(B, chid))
    shortcut = t["x"].double() @ t["wps"][:, chid:].double().t()
    assert torch.equal(y0.double(), shortcut) and torch.equal(slab0.double(), tile_sums(y0, cout))
    yz, slabz = run_project(dev, dtype, tdt, t, c0, c1, cout, wd=torch.zeros(9, chid))
    assert torch.equal(R._bits(yz), R._bits(y0)) and torch.equal(slabz, slab0)


# ------------------------------------------------------------------ 3. the predicate and the launchers
def test_launchers_refuse_what_the_predicate_refuses(dev):
    L = N.lib()
    base = dict(dtype=1, c0=128, c1=64, cout=64, H=16, W=32, x1=True, ld=None)
    nan = float("nan")
    h1 = torch.zeros(1, 24, 48, 1536, dtype=torch.float16, device=dev)
    tab = torch.ones(1, 2048, device=dev)
    wd = torch.zeros(9, 2048, device=dev)
    x = torch.zeros(1, 24, 48, 512, dtype=torch.float16, device=dev)
    wps = torch.zeros(256, 2560, dtype=torch.float16, device=dev)
    y = torch.full((1, 24, 48, 256), nan, dtype=torch.float16, device=dev)
    slab = torch.full((1, 9, 2, 256), nan, device=dev)
    tot = torch.zeros(1, 2048, dtype=torch.int64, device=dev)

    def supported(k):
        return bool(L.llie_wide_project_supported(k["dtype"], k["c0"] + k["c1"], k["c0"], 4 * (k["c0"] + k["c1"]), k["cout"], 1, 0, k["H"], k["W"]))

    def project(k):
        cin = k["c0"] + k["c1"]
        return L.llie_dwconv3x3_project(k["dtype"], h1.data_ptr(), tab.data_ptr(), tab.data_ptr(), wd.data_ptr(), tab.data_ptr(), x.data_ptr(), k["c0"],
                                        x.data_ptr() if k["c1"] else None, k["c1"], wps.data_ptr(), k["ld"] or 5 * cin, k["cout"], y.data_ptr(),
                                        slab.data_ptr(), 1, k["H"], k["W"], _st())

    def pool(k, chid):
        return L.llie_dwconv3x3_pool(k["dtype"], h1.data_ptr(), tab.data_ptr(), tab.data_ptr(), wd.data_ptr(), tot.data_ptr(), 1, k["H"], k["W"], chid, _st())

    assert supported(base)
    for kw in (dict(dtype=0), dict(H=12), dict(W=24), dict(cout=128), dict(c0=64, c1=32, cout=32), dict(c0=256, c1=0, cout=256),
               dict(c0=256, c1=256, cout=256), dict(c0=256, c1=128, cout=64), dict(c0=120, c1=72)):
        k = {**base, **kw}
        assert not supported(k), kw
        assert project(k) != 0, kw
    for kw in (dict(dtype=0), dict(H=12), dict(W=24)):
        assert pool({**base, **kw}, 768) != 0, kw
    assert pool(base, 384) != 0 and pool(base, 1024) != 0
    # a padded layer and a missing skip conv have no launcher form: the predicate alone
    assert not L.llie_wide_project_supported(1, 192, 128, 768, 64, 1, 1, 16, 32) and not L.llie_wide_project_supported(1, 192, 128, 768, 64, 0, 0, 16, 32)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(slab).all() and (tot == 0).all(), "a refused call wrote its output"


# ------------------------------------------------------------------ 4. one block through the engine
TDIM = 256
GN = "gn_finalize_kernel"


def block_forward(dev, dtype, knob):
    """y and [(class, kernel family)] of one forward of the 192 -> 64 block (split 128) at B = 2, 16 x 32"""
    L = N.lib()
    nb, H, W, cin, cout = 2, 16, 32, 192, 64
    cfg = U._module_cfg(N.LLIE_IRB, cin, cout, TDIM, split=128)
    cfg.compute_dtype = N.dtype_code(dtype)
    h = N.Handle(cfg)
    try:
        N.check(L.llie_tune(b"wide_project", knob))
        g = torch.Generator().manual_seed(19264)
        params = [(0.1 * torch.randn(shape, generator=g)).to(dev) for _, shape in h.params()]
        h.load_all(params, _st())
        x = torch.randn(nb, cin, H, W, generator=g).to(dev)
        temb = torch.randn(nb, TDIM, generator=g).to(dev)
        y = torch.empty(nb, cout, H, W, device=dev)
        nbytes = h.workspace_bytes(nb, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        h.profile_begin(31)
        N.check(L.llie_module_forward(h.h, x.data_ptr(), temb.data_ptr(), y.data_ptr(), nb, H, W, ws.data_ptr(), nbytes, _st()), "forward")
        torch.cuda.synchronize()
        rows = h.profile_dump()
        assert torch.isfinite(y).all()
        return y.cpu(), [(cls, name.split("<")[0]) for cls, name, _tag, _ms, _b in rows], nbytes
    finally:
        L.llie_tune(b"wide_project", 1)
        h.close()


def test_block_through_the_engine(dev):
    """Knob 1: norm1, pw_expand (unchanged: it still writes h1 and its slab), norm2, the pool pass, SE, dwconv3x3_project; knob 0:
    today's six launches.  The outputs: against the fp32 engine on the same parameters (its own error is some 1e-6 of the values,
    far below fp16's, so it stands in for float64 here) the new sequence may err at most twice as much as the old one -- the bound
    of the y check.  Without h2 the block's workspace is smaller."""
    GEMM, DW, SE, OTHER = N.K_GEMM, N.K_DW, N.K_SE, N.K_OTHER
    y1, seq1, ws1 = block_forward(dev, "fp16", 1)
    y0, seq0, ws0 = block_forward(dev, "fp16", 0)
    yr, _, _ = block_forward(dev, "fp32", 1)
    print(seq1, seq0)
    assert [s for s in seq1 if s[0] != SE] == [(OTHER, GN), (GEMM, "pw_expand_kernel"), (OTHER, GN), (DW, "dwconv3x3_pool_kernel"),
                                              (DW, "dwconv3x3_project_kernel")]
    assert [s for s in seq0 if s[0] != SE] == [(OTHER, GN), (GEMM, "pw_expand_kernel"), (OTHER, GN), (DW, "dwconv3x3_kernel"),
                                              (GEMM, "pw_gemm_kernel")]
    assert len(seq1) == 6 and len(seq0) == 6 and seq1[4][0] == SE and seq0[4] == seq1[4]
    err1, err0 = (y1 - yr).abs().max().item(), (y0 - yr).abs().max().item()
    print(f"Y_ERR engine 128+64->64 16x32 fp16: max |y - fp32 engine| wide {err1:.3e}, unfused {err0:.3e}, |y|max {yr.abs().max().item():.3e}")
    assert not torch.equal(y1, y0)
    assert err1 <= 2 * err0, (err1, err0)
    assert ws1 < ws0, (ws1, ws0)
