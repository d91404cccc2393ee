"""What tests/test_gpu_expand_dw_paths.py relies on, checked without a GPU.

  * the exact-operand builder (tests/expand_dw_refs.py): rounding to fp16 or bf16 wherever the kernel rounds changes nothing, and
    every per-tile pool sum is an integer below 2^24
  * the operands have teeth: references computed the way a kernel with a seeded fault would compute them -- image 0's norm2
    table for every image, chunk 0's depthwise weights for every chunk, the previous tile's x for the second tile of a run, a
    pool partial dropped for the last tile of a run -- differ from the true reference, and the first two would not with the
    identity tables of the older exact tests
  * llie_expand_dw_plan through the library: the rules against hand-computed plans, the refusals, the "irbx_grid*" knobs
  * every (tiles per workgroup, chunks per workgroup, double-buffered) class the rules can produce has an exact-operand GPU case
"""
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_dw_refs as X  # noqa: E402
import test_gpu_expand_dw_paths as G  # noqa: E402

N = importlib.import_module("cv-diffusion-model_amd._native")
CPU = torch.device("cpu")
SMALL = [(32, 3, 8, 16), (64, 3, 24, 48), (96, 2, 24, 48), (32, 3, 24, 96)]   # (Cin, B, H, W)


def operands(cin, B, H, W):
    return X.exact_operands(cin, B, H, W, CPU, 7 * cin + 3 * H + W + B)


# ------------------------------------------------------------------ 1. the builder
@pytest.mark.parametrize("cin,B,H,W", SMALL)
def test_exact_operands_round_nowhere(cin, B, H, W):
    """h2 with a rounding to T at every point where the kernel rounds (x, a', W1, a, the fp32 product 6 w, h2) equals the unrounded
    float64 result in fp16 and in bf16; it is integral with |h2| <= 9; the per-tile pool sums stay below 2^24; the tables do differ
    per image and per channel."""
    t = operands(cin, B, H, W)
    ref = X.exact_h2(t, conv_dtype=torch.float64)
    X.assert_exact(ref)
    for tdt in (torch.float16, torch.bfloat16):
        assert torch.equal(X.exact_h2(t, tdt=tdt, conv_dtype=torch.float64), ref), tdt
        assert torch.equal((6.0 * t["wd"]).to(tdt).float(), t["k6"])
    assert torch.equal(X.exact_h2(t).double(), ref)                       # the fp32 shifted adds of the device reference
    ts = X.tile_sums(ref)
    assert ts.abs().max().item() <= 9 * 128 < 2 ** 24 and torch.equal(ts, ts.round())
    assert torch.equal(X.exact_totals(ref), (ts.sum((1, 2)) * 2 ** 24).to(torch.int64))
    for k in ("s1", "b1", "s2"):
        assert not torch.equal(t[k][0], t[k][1]) and t[k][0].unique().numel() > 1, k
    chid = 4 * cin
    assert not torch.equal(t["k6"][:, :64], t["k6"][:, chid - 64:])


# ------------------------------------------------------------------ 2. seeded faults
@pytest.mark.parametrize("cin,B,H,W", SMALL[1:])
def test_seeded_faults_change_the_reference(cin, B, H, W):
    """Each reference below is what a kernel with one indexing fault would store.  The GPU file compares h2 and the totals with
    torch.equal, so `differs` is all it takes -- asserted per image / chunk / tile, where the fault acts."""
    t = operands(cin, B, H, W)
    chid = 4 * cin
    ref = X.exact_h2(t, conv_dtype=torch.float64)
    tot = X.exact_totals(ref)
    ident = dict(t, s1=torch.ones(B, cin), b1=torch.zeros(B, cin), s2=torch.ones(B, chid))   # the tables of the older exact tests
    ref_ident = X.exact_h2(ident, conv_dtype=torch.float64)

    # image 0's norm2 table for every image
    bad = X.exact_h2(t, conv_dtype=torch.float64, s2=t["s2"][0:1].expand(B, -1))
    assert torch.equal(bad[0], ref[0])
    for i in range(1, B):
        assert not torch.equal(bad[i], ref[i]) and not torch.equal(X.exact_totals(bad)[i], tot[i]), i
    assert torch.equal(X.exact_h2(ident, conv_dtype=torch.float64, s2=ident["s2"][0:1].expand(B, -1)), ref_ident)   # identity tables: blind
    # ... and image 0's norm1 table
    bad = X.exact_h2(dict(t, s1=t["s1"][0:1].expand(B, -1), b1=t["b1"][0:1].expand(B, -1)), conv_dtype=torch.float64)
    for i in range(1, B):
        assert not torch.equal(bad[i], ref[i]), i

    # chunk 0's depthwise weights for every chunk
    bad = X.exact_h2(t, conv_dtype=torch.float64, k6=t["k6"][:, torch.arange(chid) % 64])
    assert torch.equal(bad[..., :64], ref[..., :64])
    for q in range(1, chid // 64):
        assert not torch.equal(bad[..., 64 * q:64 * q + 64], ref[..., 64 * q:64 * q + 64]), q
    # ... and chunk 0's norm2 table (per channel)
    bad = X.exact_h2(t, conv_dtype=torch.float64, s2=t["s2"][:, torch.arange(chid) % 64])
    for q in range(1, chid // 64):
        assert not torch.equal(bad[..., 64 * q:64 * q + 64], ref[..., 64 * q:64 * q + 64]), q

    # the previous tile's x for the second tile of a run (runs of two along x; rows of three or six tiles)
    tiles_x = W // X.TILE_W
    prev = X.exact_h2(t, conv_dtype=torch.float64, x=t["x"].roll(X.TILE_W, 2))      # every tile computed from its left neighbour's x
    for tx in range(1, tiles_x, 2):
        cols = slice(tx * X.TILE_W, (tx + 1) * X.TILE_W)
        for ty in range(H // X.TILE_H):
            rows = slice(ty * X.TILE_H, (ty + 1) * X.TILE_H)
            assert not torch.equal(prev[:, rows, cols], ref[:, rows, cols]), (ty, tx)

    # a pool partial dropped for the last tile of a run: fixed runs of 1, 2 and 3 tiles and the even splits of the GPU cases
    ts = X.tile_sums(ref).reshape(B, -1, chid)
    for tpw, gx in ((1, 0), (tiles_x // 3, 0), (tiles_x, 0), (0, 1), (0, 2), (0, 4)):
        for first, last in X.runs(tpw, gx, H, W):
            dropped = ts.clone()
            dropped[:, last - 1] = 0
            bad_tot = (dropped.sum(1) * 2 ** 24).to(torch.int64)
            for i in range(B):
                assert not torch.equal(bad_tot[i], tot[i]), (tpw, gx, first, last, i)


def test_runs_of_the_even_split():
    """the runs the even-split cases are listed for: 9 tiles over 1, 2 and 4 workgroups"""
    assert X.runs(0, 1, 24, 48) == [(0, 9)]
    assert X.runs(0, 2, 24, 48) == [(0, 4), (4, 9)]
    assert X.runs(0, 4, 24, 48) == [(0, 2), (2, 4), (4, 6), (6, 9)]
    assert X.runs(4, 0, 24, 128)[:3] == [(0, 4), (4, 8), (8, 12)] and len(X.runs(2, 0, 24, 96)) == 9


# ------------------------------------------------------------------ 3. llie_expand_dw_plan
def knobs(L, **kw):
    for k, v in kw.items():
        N.check(L.llie_tune(k.encode(), v))


PLANS = [  # (Cin, B, H, W, project) -> (tpw, cpw, grid.x, grid.y), computed by hand from the two rules
    ((32, 3, 8, 16, 0), (1, 1, 1, 2)),           # 3 workgroups: cpw 2 -> 1
    ((64, 3, 24, 48, 0), (1, 1, 9, 4)),          # 27: cpw 4 -> 2 -> 1
    ((96, 3, 24, 48, 0), (1, 3, 9, 2)),          # cpw 6 -> 3, odd
    ((64, 56, 24, 48, 0), (1, 1, 9, 4)),         # 504: 2 chunks per workgroup would give 1008 < 1024
    ((64, 57, 24, 48, 0), (1, 2, 9, 2)),         # 513 * 2 = 1026
    ((64, 60, 24, 48, 0), (1, 2, 9, 2)),
    ((32, 113, 24, 48, 0), (1, 1, 9, 2)),        # 1017 < 1024
    ((32, 114, 24, 48, 0), (1, 2, 9, 1)),        # 1026: all chunks; tiles_x = 3 allows no run
    ((96, 113, 24, 48, 0), (1, 3, 9, 2)),
    ((96, 114, 24, 48, 0), (1, 6, 9, 1)),
    ((64, 227, 24, 96, 0), (1, 4, 18, 1)),       # 9 * 227 = 2043 < 2048; tiles_x = 6 is no multiple of 4
    ((64, 228, 24, 96, 0), (2, 4, 9, 1)),        # 2052
    ((96, 341, 24, 128, 0), (2, 6, 12, 1)),      # 6 * 341 = 2046 < 2048, 12 * 341 >= 2048
    ((96, 342, 24, 128, 0), (4, 6, 6, 1)),
    ((32, 32, 64, 64, 0), (1, 2, 32, 1)),        # 32 tiles: runs of 4 / 2 give 256 / 512 workgroups, single tiles 1024
    ((32, 1, 1080, 1920, 0), (4, 2, 4050, 1)),   # a frame on its own: 135 x 120 tiles
    ((32, 32, 128, 256, 1), (4, 2, 64, 1)),      # expand_dw_project: 64 * 32 = 2048
    ((64, 3, 24, 48, 1), (1, 4, 9, 1)),          # ... always all chunks, grid.y = 1
    ((96, 3, 24, 48, 1), (1, 6, 9, 1)),
]


def test_plan_rules_refusals_and_grid_knobs():
    L = N.lib()
    for args, want in PLANS:
        assert X.plan(L, *args) == want, args
    p = (ctypes.c_int * 4)(7, 7, 7, 7)
    for args in ((32, 3, 8, 16, 0, None), (0, 3, 8, 16, 0, p), (-32, 3, 8, 16, 0, p), (32, 0, 8, 16, 0, p), (32, 3, 0, 16, 0, p),
                 (32, 3, 8, -16, 0, p), (32, 3, 8, 16, 2, p), (32, 3, 8, 16, -1, p)):
        assert L.llie_expand_dw_plan(*args) == N.ERR_ARG, args
    for args in ((48, 3, 8, 16, 0, p), (128, 3, 8, 16, 0, p), (16, 3, 8, 16, 0, p), (32, 3, 20, 16, 0, p), (32, 3, 8, 40, 0, p),
                 (32, 1, 216, 304, 1, p)):    # 65 664 pixels: no multiple of the 1024 rows of a statistics partial
        assert L.llie_expand_dw_plan(*args) == N.ERR_SHAPE, args
    assert list(p) == [7, 7, 7, 7]           # a refused call writes nothing
    try:
        # "irbx_grid" = workgroups per launch: grid.x = knob / (B * grid.y) clamped to [1, tiles], tpw = 0; cpw as without the knob
        knobs(L, irbx_grid=8)
        assert X.plan(L, 32, 2, 24, 48) == (0, 1, 2, 2) and X.plan(L, 64, 2, 24, 48) == (0, 1, 1, 4) and X.plan(L, 96, 2, 24, 48) == (0, 3, 2, 2)
        assert X.plan(L, 32, 114, 24, 48) == (0, 2, 1, 1)                 # 8 / 114 < 1
        assert X.plan(L, 32, 2, 24, 48, 1) == (1, 2, 9, 1)                # expand_dw_project takes no grid knob
        knobs(L, irbx_grid=1 << 20)
        assert X.plan(L, 64, 60, 24, 48) == (0, 2, 9, 2)                  # at most one workgroup per tile
        knobs(L, irbx_grid=0, irbx_grid4=240)                             # the 64-channel knob alone
        assert X.plan(L, 64, 60, 24, 48) == (0, 2, 2, 2) and X.plan(L, 32, 60, 24, 48) == (1, 1, 9, 2) and X.plan(L, 96, 60, 24, 48) == (1, 3, 9, 2)
        knobs(L, irbx_grid4=0, irbx_grid2=8, irbx_grid6=16)
        assert X.plan(L, 32, 2, 24, 48) == (0, 1, 2, 2) and X.plan(L, 96, 2, 24, 48) == (0, 3, 4, 2) and X.plan(L, 64, 2, 24, 48) == (1, 1, 9, 4)
    finally:
        knobs(L, irbx_grid=0)
    for args, want in PLANS:
        assert X.plan(L, *args) == want, args


def test_gpu_cases_reach_the_plans_they_name():
    """every case of the GPU file, through the library: the GPU test asserts the same before it launches"""
    L = N.lib()
    try:
        for c in G.CASES:
            knobs(L, irbx_grid=c["grid"])
            assert X.plan(L, c["cin"], c["B"], c["H"], c["W"]) == (c["tpw"], c["cpw"], c["gx"], c["gy"]), c
            for first, last in X.runs(c["tpw"], c["gx"], c["H"], c["W"]):
                assert last > first
    finally:
        knobs(L, irbx_grid=0)
    ids = [p.id for p in G.PARAMS]
    assert len(set(ids)) == len(ids)


def test_launch_classes_all_covered():
    """The (tpw, cpw, double-buffered) classes of the GPU file's cases equal, per input width, the classes the rules can produce:
    enumerated through the library over batches 1 .. 400 of the test shapes, larger maps and whole frames, with and without the grid
    knob.  (tpw > 1 needs 2048 workgroups and so always comes with all chunks; the double-buffered build exists at 32 channels.)"""
    L = N.lib()
    shapes = [(8, 16), (24, 48), (24, 96), (24, 128), (16, 32), (64, 64), (128, 128), (256, 256), (512, 512), (1080, 1920)]
    for cin in (32, 64, 96):
        can = set()
        try:
            for grid in (0, 1, 300, 5000):
                knobs(L, irbx_grid=grid)
                for H, W in shapes:
                    for B in range(1, 401):
                        tpw, cpw, gx, gy = X.plan(L, cin, B, H, W)
                        assert cpw * gy == cin // 16 and (tpw == 0) == (grid > 0) and 1 <= gx <= (H // 8) * (W // 16)
                        can.add((tpw, cpw))
        finally:
            knobs(L, irbx_grid=0)
        can = {(tpw, cpw, dbuf) for (tpw, cpw) in can for dbuf in ((0, 1) if cin == 32 else (0,))}
        for c0 in {c["c0"] for c in G.CASES if c["cin"] == cin}:     # each segmentation of the input on its own
            covered = {(c["tpw"], c["cpw"], c["dbuf"]) for c in G.CASES if c["cin"] == cin and c["c0"] == c0}
            assert covered == can, (cin, c0, sorted(can - covered), sorted(covered - can))
    assert {(c["cin"], c["c0"]) for c in G.CASES} == {(32, 32), (64, 64), (96, 96), (96, 64)}
