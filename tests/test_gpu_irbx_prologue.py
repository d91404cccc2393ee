"""The prologue of expand_dw and expand_dw_project (irbx.hip): what a workgroup stages before its first tile -- the depthwise
weights as [tap pair][channel] dwords (times the image's SE gate where the gate is folded in), the gate table of the 64-channel
form, norm2's table with its shift / 6, norm1's table -- and the first tile's x, which leaves in the prologue at every width.

Operands that can tell a staging fault (tests/expand_dw_refs.py supplies x, norm1, W1 and norm2's scale; everything is a small
integer times a power of two, so no product and no sum on the way rounds):

    6 wd[tap][c]   = +-m 2^e: m = the tap's odd number out of 1, 3, .., 17 in an order that turns with the channel, e = (c // 9) % 3,
                     signs random but for taps 0..3, which spell c // 27.  An odd m times a power of two names (m, e): the nine taps
                     of a channel differ in every image, and the nine-vectors of any two channels differ (asserted below)
    gate[b][c]     = 2^(((3 b + 5 c) % 4) - 1): differs between neighbouring images and neighbouring channels
    norm2 shift    = 0 or 6 per image and channel: shift / 6 is 0 or 1, a missing / 6 gives 6
    Wp             +-1 where c % Cout == o: every hidden channel reaches exactly one output
    Wskip          entries in {-1, 0, 1}

(The products 6 wd gate cannot ALL differ over image, channel and tap: bf16 has 8 significand bits, and sums that stay exact in fp32
allow some 6 binary orders of magnitude -- a few hundred values for up to 342 x 384 x 9 products.  What differs is what a staging
fault can confuse: the taps of a channel, the channels of an image, neighbouring images; norm1 / norm2 tables are random per image.)

a' and a are 0 or 1, h1 / 6 is an integer, gate * h2 is at most 81 x 16 in steps of 1 / 2 (exact in T), and y = Wp (gate h2) +
shortcut is exact in the fp32 accumulators: the kernel's only rounding is y to T, from an exact value, which the float64 reference
repeats.  So h2, the pool totals, y and the per-tile sums of y must EQUAL the reference.  The per-tile sums of y^2 are 128 fp32
adds of values that are not exact: they are held to 128 x 2^-24 x sum y^2, the bound of a recursive fp32 sum in any order.
test_reference_tells_staging_faults feeds the reference each fault once -- two taps swapped, the two taps of every pair swapped,
channels shifted by 1 and by 64, the next image's gate / norm2 table, no gate, the shift not divided by 6 -- and asserts that
the output changes.

Shapes: the smallest that reach each path, asserted with llie_expand_dw_plan (SHAPES).  Outputs and the statistics slab start as
NaN, and every case runs twice on the same buffers.
"""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_dw_refs as X  # noqa: E402

pytestmark = pytest.mark.gpu
N = importlib.import_module("cv-diffusion-model_amd._native")

DTYPES = [(1, torch.float16, "_Float16"), (2, torch.bfloat16, "__bf16")]
# (kind, Cin, c0, Cout): plain expand_dw at the three widths; the three project forms (identity 32 / 64, 64 + 32 -> 32 with the skip conv)
KERNELS = [("dw", 32, 32, 0), ("dw", 64, 64, 0), ("dw", 96, 96, 0), ("proj", 32, 32, 32), ("proj", 64, 64, 64), ("proj", 96, 64, 32)]
# (B, H, W, tiles per workgroup): one all-border tile per image and a gate per image; 3 x 3 tiles, the centre one interior, one
# tile per workgroup: the unpredicated early load; runs of two; runs of four: the prefetch between tiles and its end-of-run guard
SHAPES = [(3, 8, 16, 1), (2, 24, 48, 1), (228, 24, 96, 2), (342, 24, 128, 4)]
ODD = [1, 3, 5, 7, 9, 11, 13, 15, 17]
GUARD = 1024  # NaN elements in front of and behind an output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def operands(cin, cout, B, H, W, device, seed):
    """fp32 tensors on `device`; the values of the module docstring"""
    t = X.exact_operands(cin, B, H, W, device, seed)
    g = torch.Generator(device=device).manual_seed(seed + 1)
    chid = 4 * cin
    c = torch.arange(chid, device=device)
    tap = torch.arange(9, device=device)[:, None]
    m = torch.tensor(ODD, device=device)[(2 * tap + c) % 9]
    sign = torch.randint(0, 2, (9, chid), generator=g, device=device) * 2 - 1
    sign[:4] = 1 - 2 * (((c // 27) >> tap[:4]) & 1)   # (c % 9, (c // 9) % 3, c // 27) names the channel: no two nine-vectors agree
    t["k6"] = (sign * m).float() * 2.0 ** ((c // 9) % 3).float()
    t["wd"] = t["k6"] / 6.0
    b = torch.arange(B, device=device)[:, None]
    t["gate"] = 2.0 ** (((3 * b + 5 * c) % 4) - 1).float()
    t["b2"] = 6.0 * torch.randint(0, 2, (B, chid), generator=g, device=device).float()
    if cout:
        o = torch.arange(cout, device=device)[:, None]
        t["wp"] = ((c % cout) == o).float() * (torch.randint(0, 2, (1, chid), generator=g, device=device) * 2 - 1).float()
        t["wskip"] = (torch.randint(-1, 2, (cout, cin), generator=g, device=device) *
                      (torch.rand(cout, cin, generator=g, device=device) < 0.2)).float()
    return t


def image_rows(t, idx):
    """the operands of images idx (a list) as a batch of their own"""
    sel = torch.tensor(idx, device=t["x"].device)
    return {k: (v[sel].contiguous() if k in ("x", "s1", "b1", "s2", "b2", "gate") else v) for k, v in t.items()}


def reference(t, project, identity, tdt, k6=None, gate=None, s2=None, b2=None, sixth=True, check=True):
    """float64 on the operands' device: h2 [B][H][W][Chid] (the gate included if project), and for project y [B][H][W][Cout]
    rounded to T.  k6 / gate / s2 / b2 replace an operand and sixth = False leaves the shift undivided (the seeded faults).
    check: every value is exact where the kernel holds it (T or an fp32 accumulator)."""
    k6 = t["k6"] if k6 is None else k6
    gate = t["gate"] if gate is None else gate
    s2 = t["s2"] if s2 is None else s2
    b2 = t["b2"] if b2 is None else b2
    x = t["x"].double()
    B, H, W, _ = x.shape
    ap = (x * t["s1"].double()[:, None, None, :] + t["b1"].double()[:, None, None, :]).clamp(0, 1)
    acc = ap @ t["w1"].double().t()                                                   # h1 / 6
    a = (acc * s2.double()[:, None, None, :] + b2.double()[:, None, None, :] / (6.0 if sixth else 1.0)).clamp(0, 1)
    w = k6.double()[None].expand(B, -1, -1)                                           # [B][9][Chid]: the staged weights
    if project:
        w = w * gate.double()[:, None, :]
    pad = torch.nn.functional.pad(a, (0, 0, 1, 1, 1, 1))
    h2 = torch.zeros_like(a)
    for tap in range(9):
        h2 += pad[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, :] * w[:, tap][:, None, None, :]
    out = {"h2": h2}
    if check:
        in_t = lambda v: torch.equal(v.float().to(tdt).double(), v)  # noqa: E731
        assert torch.equal(ap, ap.round()) and torch.equal(a, a.round()) and torch.equal(acc, acc.round())
        assert in_t(w) and in_t(h2) and (w != 0).all() and h2.abs().max().item() >= 8
        assert X.tile_sums(h2).abs().max().item() < 2 ** 22                          # the pool partials, in steps of 1 / 2
    if project:
        y = h2 @ t["wp"].double().t() + (x if identity else x @ t["wskip"].double().t())
        if check:
            assert torch.equal(2 * y, (2 * y).round()) and y.abs().max().item() < 2 ** 22   # exact in fp32, in any order
        out["y"] = y.float().to(tdt).double()                                         # the kernel's one rounding
    return out


class Launch:
    """one kernel on one set of operands: the device buffers (outputs NaN, between NaN guards) and run(), which may be repeated"""

    def __init__(self, L, kind, c0, cout, dtype, tdt, t):
        self.L, self.kind, self.dtype, self.t = L, kind, dtype, t
        B, H, W, cin = t["x"].shape
        self.dims = (B, H, W, cin, c0, cout)
        dev = t["x"].device
        self.x0 = t["x"][..., :c0].to(tdt).contiguous()
        self.x1 = t["x"][..., c0:].to(tdt).contiguous() if c0 < cin else None
        self.w1 = t["w1"].to(tdt)
        cout_ = cout if kind == "proj" else 4 * cin
        self.n = B * H * W * cout_
        self.obuf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=tdt, device=dev)
        self.out = self.obuf[GUARD:GUARD + self.n].view(B, H, W, cout_)
        if kind == "proj":
            self.nt = int(L.llie_irbx_project_tiles(H, W))
            self.stats = torch.full((B, self.nt, 2, cout), float("nan"), device=dev)
            self.wp = (t["wp"] if c0 == cin else torch.cat([t["wp"], t["wskip"]], 1)).to(tdt).contiguous()
        else:
            self.tot = torch.zeros(B, 4 * cin, dtype=torch.int64, device=dev)

    def run(self):
        L, t, st = self.L, self.t, torch.cuda.current_stream().cuda_stream
        B, H, W, cin, c0, cout = self.dims
        x1 = self.x1.data_ptr() if self.x1 is not None else None
        common = (t["s1"].data_ptr(), t["b1"].data_ptr(), self.w1.data_ptr(), t["s2"].data_ptr(), t["b2"].data_ptr(), t["wd"].data_ptr())
        if self.kind == "dw":
            self.tot.zero_()   # the launch adds into the totals: zeroing them is the caller's part
            N.check(L.llie_expand_dw(self.dtype, self.x0.data_ptr(), c0, x1, cin - c0, *common, self.out.data_ptr(), self.tot.data_ptr(),
                                     B, H, W, st), "expand_dw")
        elif c0 == cin:
            N.check(L.llie_expand_dw_project(self.dtype, self.x0.data_ptr(), cin, *common, t["gate"].data_ptr(), self.wp.data_ptr(),
                                             self.out.data_ptr(), self.stats.data_ptr(), B, H, W, st), "expand_dw_project")
        else:
            N.check(L.llie_expand_dw_project_skip(self.dtype, self.x0.data_ptr(), c0, x1, cin - c0, *common, t["gate"].data_ptr(),
                                                  self.wp.data_ptr(), self.wp.shape[1], cout, self.out.data_ptr(), self.stats.data_ptr(),
                                                  B, H, W, st), "expand_dw_project_skip")
        torch.cuda.synchronize()
        assert torch.isnan(self.obuf[:GUARD]).all() and torch.isnan(self.obuf[GUARD + self.n:]).all(), "written outside the output"
        return self


def kernel_name(kind, cin, cout, tname):
    if kind == "dw":
        return f"expand_dw_kernel<{tname}, {cin // 16}, 0>"
    return f"expand_dw_project_kernel<{tname}, {cin // 16}{'' if cout == cin else f', {cout}'}>"


def assert_equals_reference(run, ref, rows=None):
    """the outputs of images `rows` of the launch (all if None) against the reference of exactly those images"""
    sel = slice(None) if rows is None else torch.tensor(rows, device=run.out.device)
    got = run.out[sel].double()
    if run.kind == "dw":
        assert torch.equal(got, ref["h2"]), f"{(got != ref['h2']).sum().item()} entries of h2 differ (NaN = never written)"
        assert torch.equal(run.tot[sel], X.exact_totals(ref["h2"])), "pool totals differ"
        return
    y = ref["y"]
    assert torch.equal(got, y), f"{(got != y).sum().item()} entries of y differ (NaN = never written)"
    B, H, W, C = y.shape
    st = run.stats[sel].double()
    assert torch.equal(st[:, :, 0], X.tile_sums(y).view(B, -1, C)), "per-tile sums of y differ"
    sq = X.tile_sums(y * y).view(B, -1, C)
    assert ((st[:, :, 1] - sq).abs() <= 128 * 2.0 ** -24 * sq).all(), "per-tile sums of y^2 outside the bound of an fp32 sum"


_shared = {}   # operands of the last (Cin, Cout, B, H, W): both dtypes use them


def shared_operands(dev, cin, cout, B, H, W):
    key = (cin, cout, B, H, W)
    if _shared.get("key") != key:
        _shared.clear()
        _shared.update(key=key, t=operands(cin, cout, B, H, W, dev, 11 * cin + 5 * H + W + B + cout))
    return _shared["t"]


def _id(k, s, d):
    return f"{k[0]}{k[1]}{'' if k[2] == k[1] else 'split'}-{s[1]}x{s[2]}x{s[0]}-{'fp16' if d[0] == 1 else 'bf16'}"


PARAMS = [pytest.param(k, s, d, id=_id(k, s, d)) for k in KERNELS for s in SHAPES for d in DTYPES]


@pytest.mark.parametrize("k,s,d", PARAMS)
def test_prologue_exact_on_every_path(dev, k, s, d):
    """The launch takes the path the shape was chosen for and the kernel named for it.  Small shapes: every output of every image
    equals the float64 reference.  Runs of two and four tiles: images 0, 1, B / 2 and B - 1 equal the reference AND, bit for bit,
    the same image launched alone (one tile per workgroup).  A second run on the same buffers gives the same."""
    (kind, cin, c0, cout), (B, H, W, tpw), (dtype, tdt, tname) = k, s, d
    L = N.lib()
    project, identity = kind == "proj", c0 == cin
    plan = X.plan(L, cin, B, H, W, 1 if project else 0)
    assert plan[0] == tpw and plan[2] == (H // 8) * (W // 16) // tpw, plan
    if tpw > 1:
        assert plan[1] == cin // 16 and X.plan(L, cin, 1, H, W, 1 if project else 0)[0] == 1
    t = shared_operands(dev, cin, cout, B, H, W)
    # the nine taps of a channel differ (in size, so under any gate too), and so do the nine-vectors of any two channels
    assert (t["k6"].abs().sort(0).values.diff(dim=0) > 0).all() and torch.unique(t["k6"], dim=1).shape[1] == 4 * cin
    run = Launch(L, kind, c0, cout, dtype, tdt, t).run()
    assert L.llie_last_kernel().decode() == kernel_name(kind, cin, cout, tname)
    rows = None if tpw == 1 else [0, 1, B // 2, B - 1]
    ref = reference(t if rows is None else image_rows(t, rows), project, identity, tdt)
    assert_equals_reference(run, ref, rows)
    first = run.out.clone().view(torch.int16)
    run.run()
    assert torch.equal(run.out.view(torch.int16), first), "the second run on the same buffers differs"
    assert_equals_reference(run, ref, rows)
    if rows is not None:
        for i in rows:
            alone = Launch(L, kind, c0, cout, dtype, tdt, image_rows(t, [i])).run()
            assert torch.equal(alone.out.view(torch.int16), run.out[i:i + 1].view(torch.int16)), i
            if project:
                assert torch.equal(alone.stats.view(torch.int32), run.stats[i:i + 1].view(torch.int32)), i
            else:
                assert torch.equal(alone.tot, run.tot[i:i + 1]), i


@pytest.mark.parametrize("kind,cin,c0,cout", KERNELS)
def test_reference_tells_staging_faults(dev, kind, cin, c0, cout):
    """each staging fault, fed to the reference once, changes the output the kernel is compared on"""
    B, H, W, _ = SHAPES[0]
    t = operands(cin, cout, B, H, W, dev, 11 * cin + 5 * H + W + B + cout)
    project, identity = kind == "proj", c0 == cin
    key = "y" if project else "h2"
    clean = reference(t, project, identity, torch.bfloat16)[key]
    k6 = t["k6"]
    pairs = [1, 0, 3, 2, 5, 4, 7, 6, 8]
    faults = {"two taps swapped": dict(k6=k6[[0, 2, 1, 3, 4, 5, 6, 7, 8]]),
              "the two taps of every pair swapped": dict(k6=k6[pairs]),
              "tap 8 dropped": dict(k6=torch.cat([k6[:8], torch.zeros_like(k6[:1])])),
              "channels shifted by 1": dict(k6=k6.roll(1, 1)),
              "channels shifted by 64": dict(k6=k6.roll(64, 1)),
              "norm2 scale of the next image": dict(s2=t["s2"].roll(1, 0)),
              "norm2 shift of the next image": dict(b2=t["b2"].roll(1, 0)),
              "norm2 shift of the next channel": dict(b2=t["b2"].roll(1, 1)),
              "shift not divided by 6": dict(sixth=False)}
    if project:
        faults.update({"gate of the next image": dict(gate=t["gate"].roll(1, 0)), "gate of the next channel": dict(gate=t["gate"].roll(1, 1)),
                       "no gate": dict(gate=torch.ones_like(t["gate"]))})
    for name, f in faults.items():
        bad = reference(t, project, identity, torch.bfloat16, check=False, **f)[key]
        differ = (bad != clean).flatten(1).any(1)
        assert differ.all(), f"{name}: images {(~differ).nonzero().flatten().tolist()} give the clean output"
