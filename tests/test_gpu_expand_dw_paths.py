"""expand_dw (irbx.hip) on every loop structure its launcher can choose, h2 and SE pool totals exactly.

The launcher picks tiles per workgroup (tpw: runs of 4, 2 or 1 tiles along x, or an even split under the knob "irbx_grid") and
64-channel chunks per workgroup (cpw) from the size of the launch; llie_expand_dw_plan reports the choice.  What the kernel carries
from one tile or chunk to the next -- the prefetched x halo (32 channels), the expand-weight prefetch that wraps to the first chunk,
the pool partial that waits for the next barrier, the totals summed over a workgroup's tiles, the sH / red parity of the
double-buffered build, the barrier that frees sX -- runs only where those loops iterate, so every case below asserts the plan it
was built to reach before anything else.  CASES lists them; tests/test_expand_dw_paths_host.py proves on the CPU that the
list leaves out no (tpw, cpw, double-buffered) class the rules can produce, and that the operands can tell the seeded faults.

Exact operands (tests/expand_dw_refs.py: small integers all the way, tables that differ per image and per channel), built and
referenced on the device: h2 must equal the reference in every entry and the totals 2^24 * sum_px h2, bit for bit, with and
without totals and on a rerun.  Exact 0 / 1 activations cannot see a wrong rounding point, so the two largest paths also run
random operands: images of the batch against the same image launched alone, bit for bit, and against float64.
"""
import importlib
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_dw_refs as X  # noqa: E402

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

DTYPES = [(1, torch.float16, "_Float16"), (2, torch.bfloat16, "__bf16")]
GUARD = 1024   # NaN elements in front of and behind h2: whole 16-byte vectors in both types
SENTINEL = 0x5A5A5A5A5A5A5A5   # in front of and behind the totals
INPUTS = [(32, 32), (64, 64), (96, 96), (96, 64)]   # (Cin, c0): one input segment, and 96 channels as 64 + 32
ALL = {32: 2, 64: 4, 96: 6}                         # 64-channel chunks of Chid = 4 Cin


def _case(path, cin, c0, H, W, B, tpw, cpw, gx, dbuf=0, grid=0):
    return dict(path=path, cin=cin, c0=c0, H=H, W=W, B=B, tpw=tpw, cpw=cpw, gx=gx, gy=ALL[cin] // cpw, dbuf=dbuf, grid=grid)


def _cases():
    """one dict per launch; (tpw, cpw, gx) is what the case is meant to reach -- the plan function decides, and the test asserts it"""
    out = []
    for cin, c0 in INPUTS:
        low = 3 if cin == 96 else 1                      # cpw of a small launch: halved while even
        for dbuf in ((0, 1) if cin == 32 else (0,)):     # irbx_dbuf: the double-buffered build exists at 32 channels only
            # today's path: one tile, one chunk (three at 96) per workgroup
            out.append(_case("one", cin, c0, 8, 16, 3, 1, low, 1, dbuf))
            out.append(_case("one", cin, c0, 24, 48, 3, 1, low, 9, dbuf))
            if cin == 64:   # 540 workgroups: cpw halves once, the chunk loop runs with blockIdx.y > 0
                out.append(_case("cpw-mid", cin, c0, 24, 48, 60, 1, 2, 9, dbuf))
            # 9 * 114 = 1026 workgroups: all chunks, the weight prefetch wraps to chunk 0, tiles_x = 3 allows no run
            out.append(_case("cpw-all", cin, c0, 24, 48, 114, 1, ALL[cin], 9, dbuf))
            # tiles_x = 6: runs of two, border-interior, interior-interior, interior-border; 9 * 228 = 2052 workgroups
            out.append(_case("tpw2", cin, c0, 24, 96, 228, 2, ALL[cin], 9, dbuf))
            # tiles_x = 8: the smallest launch with runs of four, 6 * 342 = 2052 workgroups
            out.append(_case("tpw4", cin, c0, 24, 128, 342, 4, ALL[cin], 6, dbuf))
            # even split ("irbx_grid" = grid.x * B * grid.y): runs of 9, 4 + 5 and 2 + 2 + 2 + 3 tiles that wrap rows
            for gx in (1, 2, 4):
                out.append(_case("even", cin, c0, 24, 48, 2, 0, low, gx, dbuf, grid=gx * 2 * (ALL[cin] // low)))
            # ... and with the other chunk counts the rules give: all chunks (4 + 5 tiles), at 64 channels two
            out.append(_case("even-all", cin, c0, 24, 48, 114, 0, ALL[cin], 2, dbuf, grid=2 * 114))
            if cin == 64:
                out.append(_case("even-mid", cin, c0, 24, 48, 60, 0, 2, 2, dbuf, grid=2 * 60 * 2))
    return sorted(out, key=lambda c: (c["cin"], c["B"], c["H"], c["W"]))   # neighbours share operands and reference


CASES = _cases()


def _id(c, d):
    return (f"{c['path']}{c['gx'] if c['path'] == 'even' else ''}-{c['cin']}{'' if c['c0'] == c['cin'] else 'split'}"
            f"{'-dbuf' if c['dbuf'] else ''}-{c['H']}x{c['W']}x{c['B']}-{'fp16' if d == 1 else 'bf16'}")


PARAMS = [pytest.param(c, d, tdt, tn, id=_id(c, d)) for c in CASES for (d, tdt, tn) in DTYPES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_shared = {}   # the operands and reference of the last (Cin, B, H, W): both dtypes, both segmentations and all knob settings use them


def exact_case(dev, cin, B, H, W):
    key = (cin, B, H, W)
    if _shared.get("key") != key:
        _shared.clear()
        t = X.exact_operands(cin, B, H, W, dev, 7 * cin + 3 * H + W + B)
        ref = X.exact_h2(t)
        X.assert_exact(ref)
        _shared.update(key=key, t=t, ref=ref, tot=X.exact_totals(ref))
    return _shared["t"], _shared["ref"], _shared["tot"]


def launch(L, dtype, tdt, t, c0, totals):
    """h2 (device, T) and the totals (or None) of one launch.  h2 starts as NaN inside a buffer with NaN guard regions, the totals
    as 0 between sentinels; returns (h2, totals, guards intact).  t: fp32 operands on the device."""
    st = torch.cuda.current_stream().cuda_stream
    B, H, W, cin = t["x"].shape
    chid = 4 * cin
    x0 = t["x"][..., :c0].to(tdt).contiguous()
    x1 = t["x"][..., c0:].to(tdt).contiguous() if c0 < cin else None
    w1 = t["w1"].to(tdt)
    n = B * H * W * chid
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=tdt, device=x0.device)
    tbuf = torch.full((B * chid + 128,), SENTINEL, dtype=torch.int64, device=x0.device)
    tbuf[64:64 + B * chid] = 0
    N.check(L.llie_expand_dw(dtype, x0.data_ptr(), c0, x1.data_ptr() if x1 is not None else None, cin - c0, t["s1"].data_ptr(),
                             t["b1"].data_ptr(), w1.data_ptr(), t["s2"].data_ptr(), t["b2"].data_ptr(), t["wd"].data_ptr(),
                             buf[GUARD:].data_ptr(), tbuf[64:].data_ptr() if totals else None, B, H, W, st), "expand_dw")
    torch.cuda.synchronize()
    guards = bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all() and
                  (tbuf[:64] == SENTINEL).all() and (tbuf[64 + B * chid:] == SENTINEL).all())
    return buf[GUARD:GUARD + n].view(B, H, W, chid), (tbuf[64:64 + B * chid].view(B, chid) if totals else None), guards


def set_knobs(L, dbuf, grid):
    N.check(L.llie_tune(b"irbx_dbuf", dbuf))
    N.check(L.llie_tune(b"irbx_grid", grid))


# ------------------------------------------------------------------ 1. exact operands, every launch path
@pytest.mark.parametrize("c,dtype,tdt,tname", PARAMS)
def test_exact_operands_every_launch_path(dev, c, dtype, tdt, tname):
    """The launch reaches the plan the case was built for and the kernel named for it; h2 equals the reference in every entry and
    the totals equal 2^24 * sum_px h2; nothing is written outside h2 and the totals; the run without totals stores the same h2
    bits and a second run the same bits, totals included."""
    L = N.lib()
    cin, c0, B, H, W = c["cin"], c["c0"], c["B"], c["H"], c["W"]
    t, ref, tot_ref = exact_case(dev, cin, B, H, W)
    try:
        set_knobs(L, c["dbuf"], c["grid"])
        assert X.plan(L, cin, B, H, W) == (c["tpw"], c["cpw"], c["gx"], c["gy"])
        h2, tot, guards = launch(L, dtype, tdt, t, c0, True)
        assert L.llie_last_kernel().decode() == f"expand_dw_kernel<{tname}, {cin // 16}, {c['dbuf']}>"
        assert guards
        assert torch.equal(h2.float(), ref), f"{(h2.float() != ref).sum().item()} entries of h2 differ (NaN = never written)"
        assert torch.equal(tot, tot_ref), f"{(tot != tot_ref).sum().item()} pool totals differ"
        h2n, _, guards_n = launch(L, dtype, tdt, t, c0, False)
        assert guards_n and torch.equal(h2n.view(torch.int16), h2.view(torch.int16))
        del h2n
        h2r, totr, guards_r = launch(L, dtype, tdt, t, c0, True)
        assert guards_r and torch.equal(h2r.view(torch.int16), h2.view(torch.int16)) and torch.equal(totr, tot)
    finally:
        set_knobs(L, 0, 0)


# ------------------------------------------------------------------ 2. random operands on the two largest paths
def random_operands(cin, B, H, W, tdt, device, seed):
    """block_inputs of tests/test_gpu_expand_dw_project.py drawn on the device: x and W1 already rounded to T (kept in fp32), per-image tables"""
    g = torch.Generator(device=device).manual_seed(seed)
    chid = 4 * cin

    def rnd(f, *shape):
        return f(*shape, generator=g, device=device)

    t = {"x": rnd(torch.randn, B, H, W, cin).to(tdt).float(),
         "s1": 0.15 + 0.1 * rnd(torch.rand, B, cin), "b1": 0.3 + 0.2 * rnd(torch.rand, B, cin),
         "w1": (rnd(torch.randn, chid, cin) / math.sqrt(cin)).to(tdt).float(),
         "s2": 0.5 + rnd(torch.rand, B, chid), "b2": 1.0 + 2.0 * rnd(torch.rand, B, chid),
         "wd": 0.3 * rnd(torch.randn, 9, chid)}
    return t


def image(t, i):
    return {k: (v[i:i + 1].contiguous() if k in ("x", "s1", "b1", "s2", "b2") else v) for k, v in t.items()}


@pytest.mark.parametrize("dtype,tdt,tname", DTYPES)
@pytest.mark.parametrize("cin,c0", INPUTS)
@pytest.mark.parametrize("H,W,B,tpw", [(24, 48, 114, 1), (24, 128, 342, 4)])
def test_random_operands_batch_rows_vs_image_alone_and_float64(dev, H, W, B, tpw, cin, c0, dtype, tdt, tname):
    """Images 0, 1, B / 2 and B - 1 of a launch with all chunks per workgroup (tpw = 1 and runs of four): h2 and totals equal, bit
    for bit, the same image launched alone (one tile and one chunk -- three at 96 -- per workgroup: the path of the small tests),
    and h2 is within H2_BOUND of float64 (front64, for these four images only)."""
    from test_gpu_expand_dw_project import H2_BOUND, front64
    L = N.lib()
    assert X.plan(L, cin, B, H, W)[:2] == (tpw, ALL[cin]) and X.plan(L, cin, 1, H, W)[:2] == (1, 3 if cin == 96 else 1)
    t = random_operands(cin, B, H, W, tdt, dev, 1000 * cin + H + W + dtype)
    h2, tot, guards = launch(L, dtype, tdt, t, c0, True)
    assert guards
    for i in (0, 1, B // 2, B - 1):
        ti = image(t, i)
        h2i, toti, gi = launch(L, dtype, tdt, ti, c0, True)
        assert gi and not torch.isnan(h2i).any()
        assert torch.equal(h2i.view(torch.int16), h2[i:i + 1].view(torch.int16)), i
        assert torch.equal(toti, tot[i:i + 1]) and toti.abs().sum().item() > 0, i
        tc = {k: v.cpu().to(tdt) if k in ("x", "w1") else v.cpu() for k, v in ti.items()}
        ref = front64(tc, tdt, round_weights=True).permute(0, 2, 3, 1)
        rmax = ref.abs().max().item()
        err = (h2i.cpu().double() - ref).abs().max().item() / max(1.0, rmax)
        print(f"image {i}: max |h2 - float64| / max(1, |ref|max) = {err:.4e}, |ref|max {rmax:.3e}")
        assert err <= H2_BOUND[dtype], (i, err)
