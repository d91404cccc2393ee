"""Plain float64 references of the kernels behind the C ABI's per-kernel entry points, and the comparison helpers of the kernel
tests (tests/test_gpu_forward_kernels.py, tests/test_gpu_boundary_kernels.py, tests/test_forward_refs_host.py,
tests/test_gpu_backward_kernels.py, tests/test_backward_refs_host.py, tests/test_gpu_expand_gram_kernels.py).

Pure torch on CPU tensors, one function per operation.  A reference mirrors exactly the roundings its kernel does -- listed in each
docstring, read from the kernel -- and nothing else: fp32 accumulation becomes float64.  Every reference returns
(ref, abssum, slack), all float64 and of the output's shape:
  ref     the value before the kernel's final rounding to the storage type T;
  abssum  the absolute sum of the entry's terms as the kernel forms them (what fp32 accumulation error is proportional to);
  slack   what a comparison may subtract from |out - ref| before the bar applies: one ulp of T at ref for outputs stored in T,
          plus the effect of an operand whose rounding to T sits on a midpoint (`_flip_slack`).
An entry passes when |out - ref| - slack < BAR * 2^-24 * abssum (`_ratio`).  The BAR_* constants at the end were measured on the
MI355X (the worst ratio over every case of the kernel and three seeds stands beside each; the bar is about 10x that).

Layouts are the kernels': activations NHWC, [B][P][C] or [B][H][W][C]; tables [B][ld] fp32; dtype 0 fp32, 1 fp16, 2 bf16.
"""
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
TDT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
EPS_T = {0: 2.0 ** -23, 1: 2.0 ** -10, 2: 2.0 ** -7}  # one ulp relative to the leading power of two
EMIN_T = {0: -126, 1: -14, 2: -126}                   # exponent of the smallest normal (fp16 subnormals keep 2^-24 steps)
ACT_NONE, ACT_RELU6, ACT_SILU, ACT_RELU6_S6 = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ comparison helpers
def _rt(x, dtype):
    """fp32 -> the storage type (a CPU tensor of that type)."""
    return x.float().to(TDT[dtype])


def _r64(x, dtype):
    """float64 value rounded to fp32 and then to the storage type, back in float64."""
    return x.float().to(TDT[dtype]).double()


def _ulp(x, dtype):
    """one ulp of the storage type at |x| (float64)."""
    a = x.abs().clamp_min(1e-38)
    return torch.exp2(torch.floor(torch.log2(a)).clamp_min(EMIN_T[dtype])) * EPS_T[dtype]


def _flip_slack(v, dtype, err=None):
    """Where round_T(v) could come out differently when the kernel's fp32 value differs from v by up to `err` (default: a few fp32
    ulps of v): err + one ulp of T; 0 elsewhere."""
    if dtype == 0:
        return torch.zeros_like(v)
    d = v.abs() * 2.0 ** -18 if err is None else err
    lo, hi = _r64(v - d, dtype), _r64(v + d, dtype)
    return torch.where(lo != hi, d + _ulp(v, dtype), torch.zeros_like(v))


def _ratio(out, ref, abssum, slack=None, bar=None, what=""):
    """worst |out - ref| / (2^-24 * abssum) after the allowed slack; asserts it is below `bar`."""
    out = out.double()
    assert torch.isfinite(out).all(), f"{what}: entries left unwritten (NaN) or non-finite"
    err = (out - ref).abs()
    if slack is not None:
        err = (err - slack).clamp_min(0.0)
    r = (err / (U * abssum).clamp_min(1e-300)).max().item()
    print(f"RATIO {what} {r:.3f}")
    if bar is not None:
        assert r < bar, f"{what}: worst error {r:.2f} x 2^-24 of the absolute sum (bar {bar})"
    return r


def _f32(x):
    """one fp32 rounding of a float64 value"""
    return x.float().double()


# ------------------------------------------------------------------------------------------------ device buffers of the GPU tests
CANARY = 12352.0  # exact in fp16 and bf16
GUARD = 16        # canary elements on each side (keeps 16-byte alignment for every type)
NAN = float("nan")


class Guarded:
    """A device buffer of `shape` between two rows of canaries, filled with `fill` (NaN: entries never written show up)."""

    def __init__(self, shape, dev, dtype=torch.float32, fill=NAN):
        n = int(math.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), CANARY, dtype=dtype, device=dev)
        self.v = self.full[GUARD:GUARD + n].view(shape)
        self.v.fill_(fill)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def cpu(self, what=""):
        f = self.full.cpu()
        assert (f[:GUARD] == CANARY).all() and (f[-GUARD:] == CANARY).all(), f"{what}: wrote outside its buffer"
        return f[GUARD:-GUARD].view(self.v.shape)


def _bits(t):
    return t.float().view(torch.int32) if t.dtype != torch.int64 else t


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: two calls differ"


def _slab(dev, B, nt, *inner):
    """a [B][nt][inner] slab as the kernels index it, plus one extra guarded entry past the helper's count"""
    return Guarded((B * nt + 1,) + inner, dev)


def _split(s, B, nt, what):
    assert torch.isnan(s[B * nt:]).all(), f"{what}: written past the helper's tile count"
    return s[:B * nt].view(B, nt, *s.shape[1:])


# ------------------------------------------------------------------------------------------------ llie_pw_gemm (gemm.hip)
def gemm_operand(dtype, x, act, sc, sh):
    """One K segment's MFMA operand [B][P][ch] and its rounding slack.  x: [B][P][ch] of T; sc / sh: [B][ch] fp32 or None.
    pw_gemm_kernel's stage(): without a table the segment is used as loaded (the activation is skipped with the table, which is
    why llie_pw_gemm refuses an activation without one); with one, z = fma(x, sc, sh) in fp32 (one rounding; sh absent = 0),
    act 1 relu6(z), act 3 clamp01(z), act 0 z, and the result is rounded to T."""
    v = x.double()
    if sc is None:
        assert act == ACT_NONE and sh is None
        return v, torch.zeros_like(v)
    z = _f32(v * sc.double()[:, None, :] + (sh.double()[:, None, :] if sh is not None else 0.0))
    if act == ACT_RELU6:
        z = z.clamp(0.0, 6.0)
    elif act == ACT_RELU6_S6:
        z = z.clamp(0.0, 1.0)
    else:
        assert act == ACT_NONE, "the forward GEMM has no other prologue"
    return _r64(z, dtype), _flip_slack(z, dtype)


def pw_gemm_ref(dtype, xs, acts, tabs, w, bias=None, res=None):
    """llie_pw_gemm: out[b][p][n] = oscale * sum_seg sum_k A'_seg[b][p][k] W[n][k] + bias[n] + res[b][p][n].
    xs: list of [B][P][ch] T tensors; acts: the segments' act codes; tabs: (scale, shift) per segment, each [B][ch] fp32 or None
    (already cut to the segment's channels); w: [N][K] of T; bias fp32 [N]; res [B][P][N] of T.
    Roundings mirrored: the operand A' (gemm_operand); W as given in T; fp32 accumulation -> float64; epilogue v = acc * oscale
    + bias + res in fp32 (oscale = 6 iff the segments are act 3) -> taken exact; the store rounds v to T (slack: one ulp of T)."""
    ops, sls = zip(*(gemm_operand(dtype, x, a, t[0], t[1]) for x, a, t in zip(xs, acts, tabs)))
    A, S, W = torch.cat(ops, -1), torch.cat(sls, -1), w.double()
    osc = 6.0 if acts[0] == ACT_RELU6_S6 else 1.0
    ref, ab, sl = (A @ W.t()) * osc, (A.abs() @ W.abs().t()) * osc, (S @ W.abs().t()) * osc
    if bias is not None:
        ref, ab = ref + bias.double(), ab + bias.double().abs()
    if res is not None:
        ref, ab = ref + res.double(), ab + res.double().abs()
    return ref, ab, sl + _ulp(ref, dtype)


def tile_stats_ref(stored, rows):
    """Statistics slab of a [B][P][N] output as stored: [B][ceil(P / rows)][2][N] = (sum, sum of squares) over each tile of `rows`
    pixel rows (the last one partial when P % rows != 0: absent rows count for nothing), from the stored values (exact in fp32;
    the squares are rounded to fp32 once, which the bar covers).  -> (ref, abssum, slack)."""
    q = stored.double()
    B, P, N = q.shape
    nt = (P + rows - 1) // rows
    qp = torch.zeros(B, nt * rows, N, dtype=torch.float64)
    qp[:, :P] = q
    qp = qp.view(B, nt, rows, N)
    ref = torch.stack([qp.sum(2), (qp * qp).sum(2)], 2)
    ab = torch.stack([qp.abs().sum(2), (qp * qp).sum(2)], 2)
    return ref, ab, _ulp(ref, 0)


# ------------------------------------------------------------------------------------------------ llie_dwconv3x3(_ex) (dwconv.hip)
def dw_operand(dtype, x, sc, sh, s6=False, no_act=False):
    """The activated input [B][H][W][C] of the depthwise conv and its rounding slack.  dw_body_impl's activate(): z = fma(x, sc, sh)
    in fp32, relu6(z) (no_act: z; s6: clamp01(z), the tables holding scale / 6 and shift / 6), rounded to T."""
    z = _f32(x.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :])
    if s6:
        z = z.clamp(0.0, 1.0)
    elif not no_act:
        z = z.clamp(0.0, 6.0)
    return _r64(z, dtype), _flip_slack(z, dtype)


def dw_weights(dtype, w9c, s6=False):
    """[9][C] fp32 -> the kernel's packed weights: T(w), or T(6.f * w) (the product in fp32) for s6."""
    return _r64(_f32(w9c.double() * 6.0) if s6 else w9c.double(), dtype)


def pad_zero(a):
    """[B][H][W][C] -> [B][H+2][W+2][C], zero border (the conv's padding, applied after the activation)"""
    return torch.nn.functional.pad(a, (0, 0, 1, 1, 1, 1))


def dw_from_padded(ap, wt):
    """sum over the nine taps of wt[3 ky + kx][c] * ap[b][y + ky][x + kx][c]; -> (sum, absolute sum)"""
    H, W = ap.shape[1] - 2, ap.shape[2] - 2
    ref, ab = 0.0, 0.0
    for t in range(9):
        win = ap[:, t // 3:t // 3 + H, t % 3:t % 3 + W, :]
        ref, ab = ref + win * wt[t], ab + win.abs() * wt[t].abs()
    return ref, ab


def dwconv3x3_ref(dtype, x, sc, sh, w9c, s6=False, no_act=False):
    """llie_dwconv3x3 / _ex: out = depthwise3x3(act(x * sc + sh)), zero padding after the activation.  Roundings mirrored: the
    operand (dw_operand), the weights (dw_weights), fp32 accumulation -> float64, the store rounds to T (one ulp of slack)."""
    a, s = dw_operand(dtype, x, sc, sh, s6, no_act)
    wt = dw_weights(dtype, w9c, s6)
    ref, ab = dw_from_padded(pad_zero(a), wt)
    sl, _ = dw_from_padded(pad_zero(s), wt.abs())
    return ref, ab, sl + _ulp(ref, dtype)


def strip_pool_ref(stored, tx, seg_rows=8):
    """SE pool slab of a [B][H][W][C] output as stored: [B][ceil(H / 8) * ceil(W / tx)][C], entry (segment, strip) = the sum over
    its 8 rows x tx columns that lie in the image (exact fp32 values, fp32 adds).  -> (ref, abssum, slack)."""
    q = stored.double()
    B, H, W, C = q.shape
    ny, nx = (H + seg_rows - 1) // seg_rows, (W + tx - 1) // tx
    qp = torch.zeros(B, ny * seg_rows, nx * tx, C, dtype=torch.float64)
    qp[:, :H, :W] = q
    qp = qp.view(B, ny, seg_rows, nx, tx, C)
    ref, ab = qp.sum((2, 4)).reshape(B, ny * nx, C), qp.abs().sum((2, 4)).reshape(B, ny * nx, C)
    return ref, ab, _ulp(ref, 0)


# ------------------------------------------------------------------------------------------------ llie_conv3x3 (conv.hip)
def _up_axis(n):
    """bilinear x2, align_corners=False, along one axis of n samples, as conv3x3_kernel's patch_src: src = (dst + 0.5) / 2 - 0.5
    clamped at 0, upper neighbour clamped at n - 1.  -> (i0, i1, l1) for the 2n outputs."""
    s = ((torch.arange(2 * n, dtype=torch.float64) + 0.5) * 0.5 - 0.5).clamp_min(0.0)
    i0 = s.floor().long()
    return i0, (i0 + 1).clamp_max(n - 1), s - i0.double()


def upsample2x_ref(x):
    """[B][H][W][C] float64 -> [B][2H][2W][C]: ly0 (lx0 f00 + lx1 f01) + ly1 (lx0 f10 + lx1 f11); the weights are 0, 1/4, 3/4, 1."""
    y0, y1, ly = _up_axis(x.shape[1])
    x0, x1, lx = _up_axis(x.shape[2])
    lx = lx[None, None, :, None]
    ly = ly[None, :, None, None]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def conv_operand(dtype, x, mode):
    """The map the nine taps read, [B][H'][W'][Cin], and its rounding slack: the input itself (modes 0 and 2, exact), or (mode 1)
    the bilinear x2 blend, computed in fp32 and ROUNDED TO T before the MFMA (commit_item: f32_to_vec<T>)."""
    v = x.double()
    if mode != 1:
        return v, torch.zeros_like(v)
    z = upsample2x_ref(v)
    return _r64(z, dtype), _flip_slack(z, dtype)


def conv_from_padded(ap, w, stride):
    """ap: [B][Hp][Wp][Cin] (already padded by one pixel), w: [9][Cout][Cin] tap-major; out[y][x] = sum_tap ap[s y + ky][s x + kx]
    . w[tap]^T over Ho = (Hp - 3) // s + 1 rows.  -> (sum, absolute sum)"""
    Ho, Wo = (ap.shape[1] - 3) // stride + 1, (ap.shape[2] - 3) // stride + 1
    ref, ab = 0.0, 0.0
    for t in range(9):
        ky, kx = t // 3, t % 3
        win = ap[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]
        ref, ab = ref + win @ w[t].t(), ab + win.abs() @ w[t].abs().t()
    return ref, ab


def conv3x3_ref(dtype, x, w, bias, mode):
    """llie_conv3x3: mode 0 stride 2 pad 1 (Hi, Wi even), mode 1 bilinear x2 then stride 1 pad 1, mode 2 stride 1 pad 1.
    x: [B][Hi][Wi][Cin] of T, w: [9][Cout][Cin] of T, bias fp32 [Cout] or None.  Roundings mirrored: the operand (conv_operand),
    fp32 accumulation -> float64, acc + bias in fp32 -> exact, the store rounds to T (one ulp of slack)."""
    a, s = conv_operand(dtype, x, mode)
    W = w.double()
    stride = 2 if mode == 0 else 1
    ref, ab = conv_from_padded(pad_zero(a), W, stride)
    sl, _ = conv_from_padded(pad_zero(s), W.abs(), stride)
    if bias is not None:
        ref, ab = ref + bias.double(), ab + bias.double().abs()
    return ref, ab, sl + _ulp(ref, dtype)


def conv_tile_stats_ref(stored, tw, th=8):
    """Statistics slab of a [B][Ho][Wo][Cout] output as stored: [B][ceil(Ho / th) * ceil(Wo / tw)][2][Cout], tile = th rows x tw
    columns, row-major tile index, pixels past the image count for nothing.  -> (ref, abssum, slack)."""
    q = stored.double()
    B, H, W, C = q.shape
    ny, nx = (H + th - 1) // th, (W + tw - 1) // tw
    qp = torch.zeros(B, ny * th, nx * tw, C, dtype=torch.float64)
    qp[:, :H, :W] = q
    qp = qp.view(B, ny, th, nx, tw, C)
    s1, s2, sa = qp.sum((2, 4)), (qp * qp).sum((2, 4)), qp.abs().sum((2, 4))
    ref = torch.stack([s1, s2], 3).reshape(B, ny * nx, 2, C)
    ab = torch.stack([sa, s2], 3).reshape(B, ny * nx, 2, C)
    return ref, ab, _ulp(ref, 0)


# ------------------------------------------------------------------------------------------------ llie_linattn (small.hip)
def _phi(x):
    return torch.where(x > 0, x + 1.0, torch.exp(x.clamp_max(0.0)))


def linattn_splits_ranges(N, nsplit):
    """position ranges of linattn_kv_kernel's splits: nsplit equal spans"""
    span = N // nsplit
    return [(i * span, (i + 1) * span) for i in range(nsplit)]


def linattn_ref(qkv, heads, ranges):
    """llie_linattn on qkv [B][N][3 * 32 heads] (q | k | v, head-major): phi = elu + 1 on q and k in fp32 (__expf), kv[d][e] =
    sum_n phi(k[n][d]) v[n][e] and ksum[d] per position range of `ranges` (fp32 partials, added in split order), out = phi(q) kv /
    (phi(q) . ksum + 1e-6f).  No operand is rounded to T; only the store is.  -> (out, abssum, kv, kv_abssum): out / abssum
    [B][N][32 heads] with |.| propagated through numerator and denominator (den > 0, so its relative error is that of a sum of
    positive terms and contributes |out|); kv / kv_abssum [len(ranges)][B][heads][32][33], column 32 = ksum."""
    B, N, _ = qkv.shape
    inner = heads * 32
    q, k, v = (z.double().view(B, N, heads, 32).permute(0, 2, 3, 1) for z in qkv.split(inner, dim=2))  # [b][h][d][n]
    Q, K = _phi(q), _phi(k)
    parts, aparts = [], []
    for lo, hi in ranges:
        Kr, Vr = K[..., lo:hi], v[..., lo:hi]
        ks = Kr.sum(-1)[..., None]
        parts.append(torch.cat([torch.einsum("bhdn,bhen->bhde", Kr, Vr), ks], -1))
        aparts.append(torch.cat([torch.einsum("bhdn,bhen->bhde", Kr, Vr.abs()), ks], -1))
    kv, kva = torch.stack(parts), torch.stack(aparts)
    tot, tota = kv.sum(0), kva.sum(0)
    num = torch.einsum("bhdn,bhde->bhen", Q, tot[..., :32])
    numa = torch.einsum("bhdn,bhde->bhen", Q, tota[..., :32])
    den = torch.einsum("bhdn,bhd->bhn", Q, tot[..., 32])[:, :, None, :] + float(torch.tensor(1e-6, dtype=torch.float32))
    out, outa = num / den, numa / den + (num / den).abs()
    rows = lambda t: t.permute(0, 3, 1, 2).reshape(B, N, inner)  # noqa: E731
    return rows(out), rows(outa), kv, kva


# ------------------------------------------------------------------------------------------------ llie_groupnorm_finalize (small.hip)
def gn_finalize_ref(slabs, groups, P, gamma, beta, film, film_per_image, eps, post_scale):
    """llie_groupnorm_finalize.  slabs: list of fp32 [B][ntiles][2][ch] (a virtual channel concat); film: [rows][2 C] or None,
    one row per image (film_per_image) or row 0 for all.  From the fp32 slab values as given, in float64: mean = S1 / n, var =
    max(S2 / n - mean^2, 0), rstd = 1 / sqrt(var + eps); scale = gamma rstd (1 + fs) post, shift = ((beta - mean rstd gamma) (1 + fs)
    + fh) post (post_scale 0 = none).  The kernel sums the tiles in fp64 and does the rest in fp32, so no rounding is mirrored.
    -> (scale, shift, abs_scale, abs_shift), [B][C]: the absolute sums are those of the two expressions, times 1 + kappa 2^-29
    with kappa = (S2 / n) / (var + eps) the condition of the variance (the fp64 cancellation in S2 / n - mean^2, 2^-53 kappa,
    expressed in units of 2^-24)."""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    S = torch.cat([s.double().sum(1) for s in slabs], -1)  # [B][2][C]
    B, _, C = S.shape
    cg = C // groups
    n = float(cg * P)
    s1, s2 = S[:, 0].view(B, groups, cg).sum(-1), S[:, 1].view(B, groups, cg).sum(-1)
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    kappa = (s2 / n) / (var + eps)
    rc = lambda t: t.repeat_interleave(cg, dim=1)  # noqa: E731
    mean, rstd, cond = rc(mean), rc(rstd), 1.0 + rc(kappa) * 2.0 ** -29
    g, b = gamma.double()[None, :], beta.double()[None, :]
    sc, sh = g * rstd, b - mean * rstd * g
    sha = b.abs() + (mean * rstd * g).abs()
    if film is not None:
        f = film.double() if film_per_image else film.double()[:1].expand(B, -1)
        fs, fh = 1.0 + f[:, :C], f[:, C:2 * C]
        sc, sh, sha = sc * fs, sh * fs + fh, sha * fs.abs() + fh.abs()
    if post_scale != 0.0:
        ps = float(torch.tensor(post_scale, dtype=torch.float32))
        sc, sh, sha = sc * ps, sh * ps, sha * abs(ps)
    return sc, sh, sc.abs() * cond, sha * cond


# ------------------------------------------------------------------------------------------------ llie_se_mlp (small.hip)
def se_mlp_ref(sums, P, w1, b1, w2, b2, mean=None, hidden=None):
    """llie_se_mlp: mean = sums * (1.f / P), hidden = relu6(W1 mean + b1), gate = sigmoid(W2 hidden + b2); sums fp32 [B][C], w1
    [Cs][C] and w2 [C][Cs] of T (used as given), biases fp32.  Every stage is fp32 with nothing rounded to T; a later stage can be
    fed the kernel's own `mean` / `hidden`, so that each stage is judged alone.  -> ((mean, abs), (hidden, abs), (gate, abs));
    the gate's absolute sum is sigma' (sum |w| |h| + |b|) + sigma (the __expf and the division act on sigma itself)."""
    m = sums.double() / P
    ma = m.abs()
    mm = m if mean is None else mean.double()
    W1, W2 = w1.double(), w2.double()
    h = (mm @ W1.t() + b1.double()).clamp(0.0, 6.0)
    ha = mm.abs() @ W1.abs().t() + b1.double().abs()
    hh = h if hidden is None else hidden.double()
    v = hh @ W2.t() + b2.double()
    va = hh.abs() @ W2.abs().t() + b2.double().abs()
    g = torch.sigmoid(v)
    return (m, ma), (h, ha), (g, g * (1 - g) * va + g)


# ------------------------------------------------------------------------------------------------ llie_init_conv (conv_edge.hip)
def oihw_taps(w):
    """OIHW [O][I][3][3] -> tap-major [9][O][I] (tap = 3 ky + kx), float64"""
    return w.double().permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1])


def init_conv_ref(dtype, x0, x1, w, bias, mfma):
    """llie_init_conv: out NHWC [B][H][W][Cout] = conv3x3(cat(x0, x1), w) + bias, stride 1, zero padding.  x0 / x1 fp32 NCHW (x1
    may be None), w fp32 OIHW, bias fp32.  Roundings mirrored -- VALU kernel: none (fp32 inputs and weights, the bias is the first
    term of the fp32 sum); MFMA kernel: inputs and weights rounded to T (exact functions of the fp32 values, so no flip slack), fp32
    accumulation -> float64, T(acc + bias).  One ulp of T of slack for the store."""
    x = torch.cat([x0] + ([x1] if x1 is not None else []), 1).double().permute(0, 2, 3, 1)
    W = oihw_taps(w)
    if mfma:
        x, W = _r64(x, dtype), _r64(W, dtype)
    ref, ab = conv_from_padded(pad_zero(x), W, 1)
    ref, ab = ref + bias.double(), ab + bias.double().abs()
    return ref, ab, _ulp(ref, dtype)


# ------------------------------------------------------------------------------------------------ llie_final_conv (conv_edge.hip)
def silu_operand(dtype, x, sc, sh, rounded):
    """The output head's activated operand [B][H][W][C]: z = fma(x, sc, sh) in fp32 (one rounding), a = z / (1 + exp(-z)).  The
    kernels evaluate it with __expf (v_exp_f32 on z log2(e): relative error (1.5 |z| + 2) 2^-24) and an IEEE division (VALU kernel) or
    v_rcp_f32 and a product (MFMA kernel), 2 x 2^-24 more: err = |a| (1.5 |z| + 4) 2^-24.  rounded (the MFMA kernel): a is rounded to
    T and err enters through _flip_slack; else a stays fp32 and err is returned for the caller's absolute sum.
    -> (a, slack or None, err)"""
    z = _f32(x.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :])
    a = z * torch.sigmoid(z)
    err = a.abs() * (1.5 * z.abs() + 4.0) * U
    if rounded:
        return _r64(a, dtype), _flip_slack(a, dtype, err), err
    return a, None, err


def final_conv_ref(dtype, x, sc, sh, w, bias, mfma):
    """llie_final_conv without the fused step: eps fp32 NCHW [B][Cout][H][W] = conv3x3(silu(x sc + sh), w) + bias, zero padding
    outside the image (after the activation).  x NHWC [B][H][W][C] of T, sc / sh fp32 [B][C], w fp32 OIHW (Cout <= 4), bias fp32.
    Roundings mirrored -- VALU kernel: the operand and the weights stay fp32 (the operand's evaluation error joins the absolute sum,
    in units of 2^-24); MFMA kernel: operand and weights rounded to T (silu_operand's flip slack), fp32 accumulation -> float64.
    The output is fp32: one fp32 ulp of slack."""
    a, asl, err = silu_operand(dtype, x, sc, sh, mfma)
    W = oihw_taps(w)
    if mfma:
        W = _r64(W, dtype)
    ref, ab = conv_from_padded(pad_zero(a), W, 1)
    if mfma:
        sl, _ = conv_from_padded(pad_zero(asl), W.abs(), 1)
    else:
        extra, _ = conv_from_padded(pad_zero(err / U), W.abs(), 1)
        ab, sl = ab + extra, torch.zeros_like(ref)
    ref, ab = ref + bias.double(), ab + bias.double().abs()
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()  # noqa: E731
    return nchw(ref), nchw(ab), nchw(sl + _ulp(ref, 0))


def lcm_step_ref(eps, eps_ab, eps_sl, sample, noise, coef):
    """The scheduler step of final_conv_mfma_kernel's epilogue, in the kernel's operation order (separate fp32 operations, no
    contraction): x0 = sa x - sb e (v-prediction) or (x - sb e) / sa; clamped to [-1, 1] if clamp_x0; prev = x0 if is_last else sap
    x0 + sbp n; clamped = clip(prev, -1, 1).  eps / eps_ab / eps_sl: final_conv_ref's triple; coef = (sa, sb, sap, sbp, is_last,
    vpred, clamp_x0) with fp32 coefficient values.  The absolute sums carry the conv's through sb (/ sa) and sap; clamping is
    1-Lipschitz and changes neither sum nor slack.  -> {"x0" | "prev" | "clamped": (ref, abssum, slack)}"""
    sa, sb, sap, sbp = (float(torch.tensor(c, dtype=torch.float32)) for c in coef[:4])
    is_last, vpred, clamp_x0 = coef[4:]
    x, e = sample.double(), eps
    if vpred:
        x0, ab, sl = sa * x - sb * e, (sa * x).abs() + sb * eps_ab, sb * eps_sl
    else:
        x0, ab, sl = (x - sb * e) / sa, (x.abs() + sb * eps_ab) / sa, sb * eps_sl / sa
    if clamp_x0:
        x0 = x0.clamp(-1.0, 1.0)
    prev, pab, psl = x0, ab, sl
    if not is_last:
        prev, pab, psl = sap * x0 + sbp * noise.double(), sap * ab + (sbp * noise.double()).abs(), sap * sl
    return {"x0": (x0, ab, sl + _ulp(x0, 0)), "prev": (prev, pab, psl + _ulp(prev, 0)),
            "clamped": (prev.clamp(-1.0, 1.0), pab, psl + _ulp(prev, 0))}


# ------------------------------------------------------------------------------------------------ llie_se_gate (small.hip)
SE_FIX = 2.0 ** 24      # kPoolFixScale: the depthwise kernels' channel totals are fixed point, x 2^24
SE_PRE = 2.0 ** 32      # kSePreScale: fc1 pre-activations of the MFMA pair


def se_totals_ref(dtype, totals, P, w1, b1, w2, b2, path, hidden=None, pre=None):
    """llie_se_gate: the SE gate from int64 fixed-point channel totals [B][C].  w1 [Cs][C], w2 [C][Cs] of T, biases fp32.
    Paths 0 (se_gate_kernel) and 1 (se_fc1_kernel + se_fc2_kernel): mean = float(double(total) * (1.0 / (P 2^24))) exactly as the
    kernels form it, hidden = relu6(W1 mean + b1) and the gate in fp32 with nothing rounded to T.
    Path 2 (se_fc1_mfma_kernel + se_fc2_mfma_kernel): mean = T(float(total) * float(1.f / (float(P) 2^24))), mirrored bit for bit;
    every 64-channel slice of K (one wave) adds its fp32 partial product, rounded to a multiple of 2^-32, into `pre`; hidden =
    T(relu6(float(pre) 2^-32 + b1)); fc2 on the MFMA with fp32 accumulation.
    A later stage can be fed the kernel's own `hidden` (path 1) or `pre` (path 2: int64, from which the hidden operand follows
    exactly) so that each stage is judged alone; without them the first stage's error is carried into the gate: its absolute sum
    joins the gate's (paths 0, 1) or widens the flip slack of the rounded hidden (path 2: 8 x 2^-24 of fc1's absolute sum -- at
    most four accumulation roundings per slice, the int64 -> float conversion, the sum with b1 -- plus the fixed-point steps).
    -> (mean, (stage, abs, slack), (gate, abs, slack)); stage = hidden (paths 0, 1) or pre x 2^-32 before ReLU6 and bias (path 2)."""
    W1, W2, B1, B2 = w1.double(), w2.double(), b1.double(), b2.double()
    if path != 2:
        m = (totals.double() * (1.0 / (float(P) * SE_FIX))).float().double()
        h, ha = (m @ W1.t() + B1).clamp(0.0, 6.0), m.abs() @ W1.abs().t() + B1.abs()
        hh = h if hidden is None else hidden.double()
        v, va = hh @ W2.t() + B2, hh.abs() @ W2.abs().t() + B2.abs()
        if hidden is None:
            va = va + ha @ W2.abs().t()
        g = torch.sigmoid(v)
        return m, (h, ha, _ulp(h, 0)), (g, g * (1 - g) * va + g, _ulp(g, 0))
    inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(P), dtype=torch.float32) * torch.tensor(SE_FIX, dtype=torch.float32))
    m = (totals.float() * inv).to(TDT[dtype]).double()
    ns = m.shape[1] // 64
    parts = torch.einsum("bsk,jsk->sbj", m.view(m.shape[0], ns, 64), W1.view(W1.shape[0], ns, 64))
    p = (torch.round(parts * SE_PRE) / SE_PRE).sum(0)
    pa = m.abs() @ W1.abs().t()
    psl = torch.full_like(p, ns / SE_PRE)
    if pre is not None:
        hT, hsl = ((pre.double() / SE_PRE).float() + b1.float()).clamp(0.0, 6.0).to(TDT[dtype]).double(), torch.zeros_like(p)
    else:
        hf = (p + B1).clamp(0.0, 6.0)
        hT, hsl = _r64(hf, dtype), _flip_slack(hf, dtype, 8.0 * U * (pa + B1.abs()) + psl)
    v, va = hT @ W2.t() + B2, hT.abs() @ W2.abs().t() + B2.abs()
    g = torch.sigmoid(v)
    return m, (p, pa, psl), (g, g * (1 - g) * va + g, g * (1 - g) * (hsl @ W2.abs().t()) + _ulp(g, 0))


# ------------------------------------------------------------------------------------------------ llie_affine_add (small.hip)
def affine_add_ref(dtype, x, sc, sh, res=None):
    """llie_affine_add: y[b][p][c] = fma(x, sc[b][c], sh[b][c]) in fp32 (one rounding, mirrored), + res in fp32 (-> exact), stored
    in T.  x / res [B][P][C] of T, sc / sh fp32 [B][C].  tile_stats_ref(stored, 64) is its slab."""
    p, q = x.double() * sc.double()[:, None, :], sh.double()[:, None, :]
    ref, ab = _f32(p + q), p.abs() + q.abs()
    if res is not None:
        ref, ab = ref + res.double(), ab + res.double().abs()
    return ref, ab, _ulp(ref, dtype)


# ------------------------------------------------------------------------------------------------ llie_pw_gemm_dot (gemm.hip)
def gemm_dot_stats_ref(stored, dot, rows):
    """The slab of pw_gemm's `dot` epilogue: [B][ceil(P / rows)][2][N] = (sum stored * dot, sum stored) over each tile of `rows`
    pixel rows, absent rows counting for nothing; stored / dot [B][P][N] of T (products rounded to fp32 once, which the bar
    covers).  -> (ref, abssum, slack)."""
    q, d = stored.double(), dot.double()
    B, P, N = q.shape
    nt = (P + rows - 1) // rows
    pad = lambda t: torch.cat([t, torch.zeros(B, nt * rows - P, N, dtype=torch.float64)], 1).view(B, nt, rows, N)  # noqa: E731
    qp, dp = pad(q), pad(d)
    ref = torch.stack([(qp * dp).sum(2), qp.sum(2)], 2)
    ab = torch.stack([(qp * dp).abs().sum(2), qp.abs().sum(2)], 2)
    return ref, ab, _ulp(ref, 0)


# ------------------------------------------------------------------------------------------------ llie_dwconv3x3_backward (dwconv.hip)
MASK_EDGE = 2.0 ** -21  # mask_unsure: z within this much of (|bx bas| + |bab|) from 0 or 6 -- eight fp32 ulps of the larger term


def relu6_mask_ref(bx, bas, bab):
    """The ReLU6 derivative as dw_body_impl<BWD> forms it: z = bx * bas + bab in fp32, mask = 0 < z < 6, strict on both sides.
    Mirrored with one rounding (a fused multiply-add); the compiler may also round the product first, which moves z by at most one
    ulp of |bx bas| + |bab|, so an entry whose z lies within MASK_EDGE of that magnitude from 0 or 6 may take either value -- unless
    product and sum are exact in fp32 (then every evaluation order gives the same z: an exact 0 or 6 is masked, no doubt about it).
    -> (mask, mask_unsure), bool [B][H][W][C]"""
    p, q = bx.double() * bas.double()[:, None, None, :], bab.double()[:, None, None, :]
    z = _f32(p + q)
    edge = MASK_EDGE * (p.abs() + q.abs())
    inexact = (_f32(p) != p) | (z != p + q)
    return (z > 0.0) & (z < 6.0), ((z.abs() <= edge) | ((z - 6.0).abs() <= edge)) & inexact


def dwconv3x3_bwd_ref(dtype, g, gs, gb, w9c, bx, bas, bab):
    """llie_dwconv3x3_backward: dz = round_T(depthwise3x3(round_T(g * gs + gb), w9c) * [0 < bx * bas + bab < 6]), zero padding; w9c
    is the [9][C] table the kernel is given (the forward weights with the taps reversed).  Roundings mirrored: the operand
    dh2 = fma(g, gs, gb) in fp32 rounded to T (dw_operand with no_act), the weights rounded to T, fp32 accumulation -> float64, the
    mask's z (relu6_mask_ref), the store rounds to T (one ulp of slack).  An entry whose mask is unsure may be 0 or the unmasked
    value: its slack is that value's magnitude.  Masked entries have abssum 0 and slack 0: the kernel must store an exact zero.
    -> (ref, abssum, slack, mask_unsure)"""
    a, s = dw_operand(dtype, g, gs, gb, no_act=True)
    wt = dw_weights(dtype, w9c)
    acc, ab = dw_from_padded(pad_zero(a), wt)
    sl, _ = dw_from_padded(pad_zero(s), wt.abs())
    mask, unsure = relu6_mask_ref(bx, bas, bab)
    m = mask.double()
    ref = acc * m
    slack = torch.where(unsure, acc.abs() + sl + _ulp(acc, dtype), (sl + _ulp(ref, dtype)) * m)
    return ref, torch.where(unsure, ab, ab * m), slack, unsure


def strip_stats2_ref(dz_stored, bx, tx, seg_rows=8):
    """The statistics slab of llie_dwconv3x3_backward from the dz it stored: [B][ceil(H / 8) * ceil(W / tx)][2][C], entry (segment,
    strip) = tile index segment * tiles_x + strip, plane 0 the sum of dz and plane 1 the sum of dz * bx over the tile's 8 rows x tx
    columns that lie in the image (fp32 adds of exact values; the products are rounded to fp32 once, which the bar covers).
    -> (ref, abssum, slack)"""
    q, x = dz_stored.double(), bx.double()
    B, H, W, C = q.shape
    ny, nx = (H + seg_rows - 1) // seg_rows, (W + tx - 1) // tx

    def tiles(t):
        tp = torch.zeros(B, ny * seg_rows, nx * tx, C, dtype=torch.float64)
        tp[:, :H, :W] = t
        return tp.view(B, ny, seg_rows, nx, tx, C).sum((2, 4)).reshape(B, ny * nx, C)
    ref = torch.stack([tiles(q), tiles(q * x)], 2)
    ab = torch.stack([tiles(q.abs()), tiles((q * x).abs())], 2)
    return ref, ab, _ulp(ref, 0)


# The maps of the depthwise tests, forward and backward -- (H, W, TX, ragged): TX = the strip width launch_dw_t takes; non-square maps
# both ways round.  13 x 24: ragged rows on a width that is 8 (mod 16) -- the ragged kernel has no 8-wide form and runs 16-wide strips,
# and llie_dwconv3x3_tiles must count those
DW_MAPS = [(8, 24, 8, False), (16, 8, 8, False), (8, 40, 8, False), (16, 16, 16, False), (8, 48, 16, False), (16, 32, 32, False),
           (8, 64, 32, False), (9, 13, 16, True), (13, 9, 16, True), (13, 12, 16, True), (25, 18, 32, True), (18, 25, 32, True),
           (9, 20, 32, True), (25, 50, 32, True), (25, 32, 32, True), (9, 16, 16, True), (13, 24, 16, True)]
# the backward test adds a last segment of four rows (H = 12) on whole 16-wide strips
DW_BWD_MAPS = DW_MAPS + [(12, 16, 16, True)]
DW_BWD_CASES = [(H, W, tx, rg, dtype, 2 * (32 if dtype == 0 else 64)) for H, W, tx, rg in DW_BWD_MAPS for dtype in (0, 1, 2)]
# (H, strip height, B, dtype) at W = 8 and one channel chunk: a strip as high as the map, and two 16-row strips (the second one's slab
# segments start at 2)
DW_BWD_STRIPS = [(H, H, 1024, dtype) for H in (16, 32, 64) for dtype in (0, 1, 2)] + [(32, 16, 512, dtype) for dtype in (0, 1, 2)]


def seeded(seed0, *key):
    """the generator of one test case; seed0 = LLIE_FWD_TEST_SEED"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 1000003 + 7919 * seed0)


def dw_bwd_inputs(B, H, W, C, dtype, seed0, key):
    """Inputs of llie_dwconv3x3_backward as Back::irb_bwd meets them: g = d(a3) and bx = h1 of T, gs = the SE gate in (0, 1), gb =
    d(mean) / P, w = the flipped taps, bas / bab = norm2's affine.  z = bx bas + bab has mean 3 and deviation about 2.5, so that
    roughly a tenth of the entries lies below 0, a tenth above 6, and (relu6_mask_ref) next to none within rounding of either edge;
    channel 0 holds exact zeros and sixes.
    -> (g, gs, gb, w, bx, bas, bab)"""
    gn = seeded(seed0, "dw_bwd", key, dtype)
    g = _rt(torch.randn(B, H, W, C, generator=gn), dtype)
    gs, gb = torch.rand(B, C, generator=gn) * 0.9 + 0.05, torch.randn(B, C, generator=gn) * 0.1
    w = torch.randn(9, C, generator=gn) / 3
    bx = _rt(torch.randn(B, H, W, C, generator=gn) * 2, dtype)
    bas, bab = torch.rand(B, C, generator=gn) + 0.5, torch.randn(B, C, generator=gn) * 1.5 + 3.0
    # channel 0: z = bx exactly, with every fourth pixel exactly 6 and every fourth exactly 0 -- both edges of the strict mask
    bas[:, 0], bab[:, 0] = 1.0, 0.0
    d = (torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 4
    bx[:, :, :, 0] = torch.where(d == 0, 6.0, torch.where(d == 2, 0.0, bx[:, :, :, 0].float())).to(bx.dtype)
    return g, gs, gb, w, bx, bas, bab


def dw_bwd_case_inputs(case, seed0):
    H, W, tx, rg, dtype, C = case
    return dw_bwd_inputs(3, H, W, C, dtype, seed0, (H, W, C))


def dw_bwd_strip_inputs(H, rows, dtype, seed0):
    return dw_bwd_inputs(3, H, 8, 32 if dtype == 0 else 64, dtype, seed0, ("strip", H, rows))


def mask_unsure_ok(unsure, tx):
    """The condition the backward depthwise cases must meet for their mask to be decided by the reference: unsure entries are at most
    0.1 % of the case, and in no (8-row segment, strip, channel) tile do they make up every pixel."""
    B, H, W, C = unsure.shape
    ny, nx = (H + 7) // 8, (W + tx - 1) // tx
    cnt = torch.zeros(B, ny * 8, nx * tx, C)
    cnt[:, :H, :W] = unsure.float()
    inside = torch.zeros(1, ny * 8, nx * tx, 1)
    inside[:, :H, :W] = 1.0
    per_tile = cnt.view(B, ny, 8, nx, tx, C).sum((2, 4))
    pixels = inside.view(1, ny, 8, nx, tx, 1).sum((2, 4))
    return unsure.float().mean().item() <= 1e-3 and bool((per_tile < pixels).all())


# ------------------------------------------------------------------------------------------------ the backward pass's glue (bwd.hip)
def bias_grad_ref(g, Cstore):
    """llie_bias_grad: out[c] = sum over the rows of g [M][C] (T values, fp32 adds) for c < Cstore.  -> (ref, abssum, slack)"""
    q = g.double()[:, :Cstore]
    ref = q.sum(0)
    return ref, q.abs().sum(0), _ulp(ref, 0)


def pack_planes_ref(dtype, x0, x1):
    """llie_pack_planes: fp32 planes x0 [B][c0][P], x1 [B][c1][P] or None -> [B * P][32] of T: channel c < c0 from x0, c0 <= c < c0 + c1
    from x1, the rest zero; each value rounded to T once (exact: the test asks for equal bits)."""
    xs = torch.cat([x0] + ([x1] if x1 is not None else []), 1)            # [B][c0 + c1][P]
    B, c, P = xs.shape
    out = torch.zeros(B, P, 32)
    out[:, :, :c] = xs.permute(0, 2, 1)
    return _rt(out.reshape(B * P, 32), dtype)


def add_into_ref(dtype, dst, src):
    """llie_add_into: the fp32 sum of two T values, rounded to T once (IEEE operations: the test asks for equal bits)."""
    return (dst.float() + src.float()).to(TDT[dtype])


def sin_freqs(dim):
    """SinusoidalPosEmb's frequency table as llie_create tabulates it: q = (float(-ln 1e4) * i) / half in fp32, exp in double, to fp32"""
    half = dim // 2
    q = (torch.tensor(-math.log(10000.0), dtype=torch.float32) * torch.arange(half, dtype=torch.float32)) / float(half)
    return q.double().exp().float()


def sin_embed_ref(t, freqs):
    """sin_embed_kernel / time_embed_kernel: arg = float(t) * freqs[i], one fp32 product (mirrored); emb = [cos(arg) | sin(arg)].
    cosf / sinf reduce an argument of up to 999 with an absolute, not a relative error, so the absolute sum of an entry is 1 (the
    functions' amplitude).  -> (ref, abssum, slack) [rows][dim]"""
    arg = (t.float()[:, None] * freqs.float()[None, :]).double()
    ref = torch.cat([arg.cos(), arg.sin()], 1)
    return ref, torch.ones_like(ref), _ulp(ref, 0)


def _silu_err(z):
    """evaluation error of siluf(z) = z / (1 + __expf(-z)) in units of 2^-24, as silu_operand states it: |silu(z)| (1.5 |z| + 4)"""
    return (z * torch.sigmoid(z)).abs() * (1.5 * z.abs() + 4.0)


def time_embed_ref(emb, w1, b1, w3, b3):
    """time_embed_kernel after the embedding: hidden = silu(W1 emb + b1), temb = W3 hidden + b3, silu_temb = silu(temb), all fp32
    with nothing rounded in between (-> float64).  emb: the kernel's own fp32 embedding, so that the MLP is judged alone.  The
    hidden layer's error is carried on: |silu'| times its pre-activation's absolute sum plus the evaluation error of siluf joins
    temb's absolute sum, and likewise for silu_temb.  -> ((temb, abssum, slack), (silu_temb, abssum, slack))"""
    e, W1, W3 = emb.double(), w1.double(), w3.double()
    z1, z1a = e @ W1.t() + b1.double(), e.abs() @ W1.abs().t() + b1.double().abs()
    dsilu = lambda z: torch.sigmoid(z) * (1 + z * (1 - torch.sigmoid(z)))  # noqa: E731
    h, ha = z1 * torch.sigmoid(z1), dsilu(z1).abs() * z1a + _silu_err(z1)
    temb, ta = h @ W3.t() + b3.double(), (h.abs() + ha) @ W3.abs().t() + b3.double().abs()
    st, sa = temb * torch.sigmoid(temb), dsilu(temb).abs() * ta + _silu_err(temb)
    return (temb, ta, _ulp(temb, 0)), (st, sa, _ulp(st, 0))


def pointwise_bwd_ref(kind, a, b, scale=0.0):
    """llie_pointwise_backward on fp32 vectors: kind 0 a b (1 - b); 1 (0 < b < 6 ? a : 0), exact; 2 a silu'(b) with sigmoid from
    __expf (the evaluation error grows with |b| as for siluf); 3 a * scale, one rounding, exact.  -> (ref, abssum) -- abssum None
    where the test asks for equal bits."""
    a64, b64 = a.double(), (b.double() if b is not None else None)
    if kind == 0:
        return a64 * b64 * (1 - b64), a64.abs() * b64.abs() * (1 + b64.abs())
    if kind == 1:
        return torch.where((b64 > 0) & (b64 < 6), a64, torch.zeros_like(a64)), None
    if kind == 2:
        sg = torch.sigmoid(b64)
        return a64 * sg * (1 + b64 * (1 - sg)), a64.abs() * sg * (1 + b64.abs() * (1 - sg)) * (1.5 * b64.abs() + 4.0)
    return _f32(a64 * float(torch.tensor(scale, dtype=torch.float32))), None


# ------------------------------------------------------------------------------------------------ llie_pw_expand (pwx.hip)
def pw_expand_nsplit(M, N):
    """nsplit_for (pwx.hip) with one 32-channel block per LDS buffer: the channels of a 128-pixel tile are halved over workgroups
    while the grid has fewer than 512 of them, each part keeps at least two 32-channel blocks and stays a multiple of 64 wide."""
    ns, nb = 1, N // 32
    while (M // 128) * ns < 512 and nb % (2 * ns) == 0 and N // (64 * ns) >= 2 and (N // (2 * ns)) % 64 == 0:
        ns *= 2
    return ns


def pw_expand_grid(M, N):
    """-> (nsplit, tile remap on, nit): the remap of pw_expand_body runs where the 128-pixel tiles are a multiple of 8; nit = the
    32-channel weight buffers a workgroup walks through."""
    ns = pw_expand_nsplit(M, N)
    return ns, (M // 128) % 8 == 0, N // ns // 32


def pw_expand_weights(dtype, w32):
    """pack_expand_kernel's (T)(w * 6.f), [N][K] float64.  fp16: hipcc folds the product and the conversion into one v_fma_mixlo_f16
    (w * 6 + 0), the exact product rounded ONCE to fp16; bf16 has no such instruction: the product is rounded to fp32, then to bf16.
    (The two differ where the fp32 product sits on an fp16 midpoint, about one weight in 10^4.)"""
    e = w32.double() * 6.0  # exact: 24 + 3 significant bits
    if dtype == 1:
        return torch.from_numpy(e.numpy().astype(np.float16).astype(np.float64))  # numpy converts float64 to float16 directly
    return _r64(_f32(e), dtype)


def pw_expand_ref(dtype, xs, tabs, w32):
    """llie_pw_expand: out[b][p][n] = sum_seg sum_k a'_seg[b][p][k] W6[n][k], a' = T(clamp01(x s + b)) with per-image tables
    (gemm_operand, act 3), W6 = T(6 W) (pw_expand_weights).  xs: list of [B][P][ch] T tensors; tabs: (scale, shift) per segment, each
    [B][ch] fp32 (already cut to the segment's channels); w32 fp32 [N][K].  Roundings mirrored: the operand, the weights; fp32
    accumulation -> float64; the store rounds to T (one ulp of slack).  abssum and the flip slack are formed as pw_gemm_ref forms
    them.  tile_stats_ref(stored, 128) is its statistics slab.  -> (ref, abssum, slack)"""
    ops, sls = zip(*(gemm_operand(dtype, x, ACT_RELU6_S6, t[0], t[1]) for x, t in zip(xs, tabs)))
    A, S, W = torch.cat(ops, -1), torch.cat(sls, -1), pw_expand_weights(dtype, w32)
    ref, ab, sl = A @ W.t(), A.abs() @ W.abs().t(), S @ W.abs().t()
    return ref, ab, sl + _ulp(ref, dtype)


# ------------------------------------------------------------------------------------------------ llie_gram_stats / llie_gram_finalize (gram.hip)
def gram_rows(P):
    """gram_rows (gram.hip): pixels per workgroup -- 4096, halved down to 512 while P is no multiple of it or gives fewer than 16
    workgroups.  nwg = P // gram_rows(P)."""
    rp = 4096
    while rp > 512 and (P % rp or P // rp < 16):
        rp >>= 1
    return rp


def gram_operand(dtype, x, sc, bi):
    """a' [B][p][K] as gram_activate8 forms it, and its rounding slack.  act_clamp01_pack: fp16 is one v_fma_mix with the clamp
    modifier, the exact x s + b rounded ONCE to fp16; bf16 is fmaf, the clamp, then the conversion.  The reference rounds the exact
    value to fp32 and then to T, which differs from either only where the fp32 value lies within one fp32 ulp of a rounding
    boundary of T: that, not gemm_operand's wider margin, is the flip slack here -- over 10^4 to 10^5 pixels the wider one would
    add up to more than the error of a kernel that never rounded a' at all (test_gram_bars_have_teeth)."""
    z = _f32(x.double() * sc.double()[:, None, :] + bi.double()[:, None, :]).clamp(0.0, 1.0)
    return _r64(z, dtype), _flip_slack(z, dtype, _ulp(z, 0))


def gram_ref(dtype, x0, x1, sc, bi, chunk=8192):
    """llie_gram_stats: G[b] = sum_px a' a'^T [K][K] and m[b] = sum_px a' [K] of a' = T(clamp01(x s + b)) over the virtual concat of x0
    [B][P][c0] and x1 [B][P][c1] (or None); sc / bi fp32 [B][K].  Roundings mirrored: the operand (gram_operand); the products
    of two T values are exact in fp32, fp32 accumulation -> float64.  The terms are non-negative, so the absolute sums are G and m
    themselves.  Slack: one fp32 ulp, plus for every activation whose rounding to T may fall the other way its step times the other
    factor (both factors on the diagonal).  Formed in chunks of pixels.  -> ((G, abssum, slack), (m, abssum, slack))"""
    x = torch.cat([x0, x1], 2) if x1 is not None else x0
    B, P, K = x.shape
    G, SG = torch.zeros(B, K, K, dtype=torch.float64), torch.zeros(B, K, K, dtype=torch.float64)
    m, sm = torch.zeros(B, K, dtype=torch.float64), torch.zeros(B, K, dtype=torch.float64)
    for p0 in range(0, P, chunk):
        a, s = gram_operand(dtype, x[:, p0:p0 + chunk], sc, bi)
        G += torch.einsum("bpi,bpj->bij", a, a)
        cross = torch.einsum("bpi,bpj->bij", s, a)
        SG += cross + cross.transpose(1, 2) + torch.einsum("bpi,bpj->bij", s, s)
        m += a.sum(1)
        sm += s.sum(1)
    return (G, G, SG + _ulp(G, 0)), (m, m, sm + _ulp(m, 0))


def gram_finalize_ref(dtype, gtot, w, K, P, gamma, beta, film, film_stride, eps, post_scale):
    """llie_gram_finalize: norm2 + FiLM of h1 = 6 W a' from the Gram totals.  gtot fp32 [B][K K + K] (G row-major, then m) exactly as
    the kernel is given it; w [4 K][K] of T; 32 groups of K / 8 channels; film (or None): flat fp32, image b's row starting at b *
    film_stride, (1 + film scale) at [c] and the FiLM shift at [4 K + c].  In float64 from those values: S1_c = 6 w_c . m, S2_c = 36
    w_c^T G w_c, summed over the group; mean = S1 / n, var = max(S2 / n - mean^2, 0), n = (K / 8) P; rstd = 1 / sqrt(var + eps);
    scale = gamma rstd (1 + fs) post, shift = ((beta - mean rstd gamma) (1 + fs) + fh) post (post_scale 0 = none).  The kernel forms
    the sums and the variance in fp64 and the rest in fp32, so no rounding is mirrored.  The cancellation is treated as
    gn_finalize_ref treats it: the absolute sums are those of the two expressions times 1 + kappa 2^-29, with kappa the absolute
    sum of the quadratic form's terms (36 |w|^T G |w| / n, G >= 0) plus mean^2, over var + eps.
    -> (scale, shift, abs_scale, abs_shift), [B][4 K]"""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    g64, W = gtot.double(), w.double()
    B, C, cg = g64.shape[0], 4 * K, K // 8
    G, m = g64[:, :K * K].view(B, K, K), g64[:, K * K:]
    s1 = 6.0 * torch.einsum("ck,bk->bc", W, m)
    s2 = 36.0 * torch.einsum("ci,bij,cj->bc", W, G, W)
    s2a = 36.0 * torch.einsum("ci,bij,cj->bc", W.abs(), G.abs(), W.abs())
    n = float(cg * P)
    grp = lambda t: t.view(B, 32, cg).sum(-1)  # noqa: E731
    mean = grp(s1) / n
    var = (grp(s2) / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    kappa = (grp(s2a) / n + mean * mean) / (var + eps)
    rc = lambda t: t.repeat_interleave(cg, dim=1)  # noqa: E731
    mean, rstd, cond = rc(mean), rc(rstd), 1.0 + rc(kappa) * 2.0 ** -29
    g, b = gamma.double()[None, :], beta.double()[None, :]
    sc, sh = g * rstd, b - mean * rstd * g
    sha = b.abs() + (mean * rstd * g).abs()
    if film is not None:
        flat = film.double().reshape(-1)
        f = torch.stack([flat[i * film_stride:i * film_stride + 2 * C] for i in range(B)])
        fs, fh = 1.0 + f[:, :C], f[:, C:]
        sc, sh, sha = sc * fs, sh * fs + fh, sha * fs.abs() + fh.abs()
    if post_scale != 0.0:
        ps = float(torch.tensor(post_scale, dtype=torch.float32))
        sc, sh, sha = sc * ps, sh * ps, sha * abs(ps)
    return sc, sh, sc.abs() * cond, sha * cond


# ------------------------------------------------------------------------------------------------ llie_film / llie_silu_rows (small.hip)
def film_ref(st, wf, bf):
    """llie_film: film[r][f] = bf[f] + sum_t wf[f][t] st[r][t], all fp32 with nothing rounded in between (-> float64).  st [rows][T],
    wf [F][T], bf [F].  -> (ref, abssum, slack)"""
    s, W, b = st.double(), wf.double(), bf.double()
    ref = s @ W.t() + b
    return ref, s.abs() @ W.abs().t() + b.abs(), _ulp(ref, 0)


def silu_ref(x):
    """llie_silu_rows: siluf(x) = x / (1 + __expf(-x)) on fp32 values.  The absolute sum is the evaluation error silu_operand states,
    |silu(x)| (1.5 |x| + 4), in units of 2^-24.  -> (ref, abssum, slack)"""
    z = x.double()
    ref = z * torch.sigmoid(z)
    return ref, _silu_err(z), _ulp(ref, 0)


# ------------------------------------------------------------------------------------------------ cases of tests/test_gpu_expand_gram_kernels.py
# llie_pw_expand: (segments, N, P, B, affine_ld - K, (nsplit, tile remap, nit)): the grid values are what launch_cfg takes for the full
# batch (pw_expand_grid re-derives them in tests/test_forward_refs_host.py; the GPU test asserts nsplit through llie_pw_expand_nsplit)
PWX_CASES = [
    ([128], 64, 128, 3, 0, (1, False, 2)),             # nsplit 1, the smallest N
    ([128], 576, 128, 3, 0, (1, False, 18)),           # nsplit 1, an 18-buffer channel loop
    ([64, 64], 512, 256, 3, 24, (8, False, 2)),        # two segments, affine_ld = K + 24
    ([192], 128, 128, 8, 0, (2, True, 2)),             # nsplit 2, tile remap (8 tiles), NCH = 3: the prefetch does not rotate
    ([64, 64, 64], 768, 384, 1, 24, (4, False, 6)),    # three segments (koff2), affine_ld = K + 24
    ([128, 64], 1152, 1024, 1, 0, (2, True, 18)),      # the bench's nsplit = 2 with a long loop, remap
    ([256], 1024, 128, 5, 0, (16, False, 2)),          # NCH = 4: the 3-deep prefetch rotates once
    ([128, 64, 64], 1024, 256, 4, 0, (16, True, 2)),   # ... over three segments
    ([384], 1536, 128, 3, 0, (8, False, 6)),           # NCH = 6
    ([256, 64, 64], 1536, 1024, 1, 0, (8, True, 6)),   # NCH = 6 over three segments
    ([512], 2048, 128, 2, 0, (32, False, 2)),          # K = 512: stores straight from registers, NCH = 8
    ([384, 64, 64], 2048, 256, 4, 0, (32, True, 2)),   # ... over three segments
    ([512], 1088, 128, 2, 0, (1, False, 34)),          # K = 512 with a 34-buffer loop, nsplit 1
]
# llie_gram_stats: (c0, c1, P, B, nwg)
GRAM_CASES = [(32, 0, 512, 3, 1), (64, 32, 1536, 2, 3), (32, 32, 4096, 2, 8), (96, 0, 8704, 2, 17), (32, 0, 17408, 1, 17),
              (64, 0, 16384, 2, 16), (64, 32, 65536, 1, 16)]


def pwx_inputs(gen, dtype, segs, n, P, B, ld_extra=0):
    """The input family of test_gpu_round3._expand_case: x ~ 1.5 N(0, 1) rounded to T, w ~ N(0, 1 / K), norm1's tables as gn_finalize
    emits them for act 3 (scale / 6 in [1/12, 1/4], shift / 6 ~ N(0.4, 0.5) / 6).  The tables are one [B][K + ld_extra] pair that every
    segment reads at its own channel offset.  -> (xs [B][P][ch], w32 [n][K], sc, bi)"""
    K = sum(segs)
    xs = [_rt(torch.randn(B, P, c, generator=gen) * 1.5, dtype) for c in segs]
    w32 = torch.randn(n, K, generator=gen) / math.sqrt(K)
    sc = (torch.rand(B, K + ld_extra, generator=gen) + 0.5) / 6
    bi = (torch.randn(B, K + ld_extra, generator=gen) * 0.5 + 0.4) / 6
    return xs, w32, sc, bi


def seg_tables(segs, sc, bi):
    """the per-segment cuts of one table pair: [(scale [B][ch], shift [B][ch])]"""
    offs = [sum(segs[:i]) for i in range(len(segs))]
    return [(sc[:, o:o + c], bi[:, o:o + c]) for o, c in zip(offs, segs)]


def gram_inputs(gen, dtype, c0, c1, P, B, family):
    """family "gauss": the inputs of pwx_inputs; "ones": tables that make every activation of the first input exactly 1 (scale 0, shift
    1) and every other exactly 0, so that G and m are exact integers (P or 0).  -> (x0, x1 or None, sc, bi)"""
    K = c0 + c1
    x0 = _rt(torch.randn(B, P, c0, generator=gen) * 1.5, dtype)
    x1 = _rt(torch.randn(B, P, c1, generator=gen) * 1.5, dtype) if c1 else None
    sc = (torch.rand(B, K, generator=gen) + 0.5) / 6
    bi = (torch.randn(B, K, generator=gen) * 0.5 + 0.4) / 6
    if family == "ones":
        sc, bi = torch.zeros(B, K), torch.zeros(B, K)
        bi[:, :c0] = 1.0
    return x0, x1, sc, bi


def gram_fin_inputs(gen, dtype, K, P, B, hard):
    """The two families of test_gpu_round4._gram_case: plain, and "hard" -- nearly constant activations near the clamp's upper end with
    expand rows of (almost) zero sum, where the variance is a small difference of large terms.  The totals are formed in float64 from
    the T activations and handed over in fp32, as llie_gram_stats leaves them.  -> (gtot fp32 [B][K K + K], w [4 K][K] of T, a)"""
    if hard:
        a = (0.9 + 0.02 * torch.randn(B, P, K, generator=gen)).clamp(0, 1)
        w = torch.randn(4 * K, K, generator=gen) / math.sqrt(K)
        w = w - w.mean(1, keepdim=True) * 0.98
    else:
        a = torch.rand(B, P, K, generator=gen).clamp(0, 1) * (torch.rand(B, 1, K, generator=gen) + 0.2)
        w = torch.randn(4 * K, K, generator=gen) / math.sqrt(K)
    a, w = _rt(a, dtype), _rt(w, dtype)
    ad = a.double()
    gtot = torch.cat([torch.einsum("bpi,bpj->bij", ad, ad).reshape(B, K * K), ad.sum(1)], 1).float()
    return gtot, w, a


# ------------------------------------------------------------------------------------------------ bars
# BAR x 2^-24 x abssum per entry.  "worst" = the worst ratio |out - ref| / (2^-24 abssum) measured on the MI355X over all cases of
# the kernel in tests/test_gpu_forward_kernels.py and seeds 0, 1, 2 (LLIE_FWD_TEST_SEED), as fp32 / fp16 / bf16; the bar is about
# 10x that, because the worst ratio moves by a small factor from seed to seed.
BAR_GEMM = 50.0        # worst 5.00 / 0.29 / 0.10
BAR_GEMM_STATS = 18.0  # worst 1.78 / 1.24 / 0.96
BAR_DW = 26.0          # worst 2.64 / 1.08 / 0.18
BAR_DW_POOL = 21.0     # worst, slab 1.09 / 0.54 / 0.00, totals 2.10 / 1.63 / 0.93
BAR_CONV = 49.0        # worst 4.87 / 0.50 / 0.19
BAR_CONV_STATS = 17.0  # worst 1.67 / 1.54 / 1.15
BAR_ATTN = 20.0        # worst 2.04 / 0.00 / 0.06
BAR_ATTN_KV = 160.0    # worst 15.83 / 10.75 / 10.31 (spans of 256 and 384 positions summed one after the other; 2.6 at N = 25)
BAR_GN = 30.0          # worst, scale 2.16, shift 3.00 (fp32 tables only)
BAR_SE = 20.0          # worst, mean 0.00, hidden 0.62, gate 1.96 (the same for every weight type)
# the head, tail and boundary kernels: worst over all cases of tests/test_gpu_boundary_kernels.py and seeds 0, 1, 2, as fp32 / fp16 / bf16
BAR_INIT = 49.0           # worst 4.81 / 0.64 / 0.67 (all VALU kernel; MFMA kernel 0.42 fp16, 0.27 bf16)
BAR_INIT_STATS = 26.0     # worst 1.29 / 2.54 / 1.93
BAR_FINAL = 26.0          # worst 0.75 / 2.59 / 2.15 (2-byte: the MFMA kernel, 2.59 with the fused step, 1.98 / 2.15 without; VALU kernel 0.77 / 0.82)
BAR_STEP = 23.0           # worst, prev 2.25 / 1.52, clamped 1.61 / 1.49 (fp16 / bf16: the step exists in the MFMA kernel alone)
BAR_SE_GATE = 17.0        # worst, path 0 gate 0.64 / 0.66 / 0.56; path 1 hidden 0.31, gate 1.36; path 2 pre 0.29, gate 1.63 / 1.32
BAR_AFFINE = 2.0          # worst 0.00 / 0.00 / 0.00: always inside the ulp of the stored value.  Not measured but reasoned: after the
                          # mirrored fma the kernel rounds twice more in fp32 at most (the residual add; the shift, were the fma not
                          # contracted), each by at most 2^-24 of the absolute sum
BAR_AFFINE_STATS = 22.0   # worst 1.73 / 2.15 / 1.17
BAR_CONVERT_STATS = 78.0  # worst 5.76 / 7.77 / 4.78, all at P = 192: nchw_to_nhwc_kernel adds a tile's 64 pixels one after the other in one
                          # thread, where the other producers add 16 per lane and then combine lanes and waves as a tree
BAR_GEMM_DOT = 9.0        # worst 0.84 / 0.57 / 0.37 (the output itself, under BAR_GEMM: 4.25 / 0.15 / 0.05)
# the depthwise input gradient and the backward pass's glue: worst over all cases of the tests of tests/test_gpu_backward_kernels.py
# named beside each and seeds 0, 1, 2, as fp32 / fp16 / bf16
BAR_DW_BWD = 32.0         # dz, worst 3.25 / 0.24 / 0.00 (test_dwconv3x3_backward_vs_float64; strip heights 2.40 / 0.11 / 0.00; norm2 site 2.95 / - / 0.16)
BAR_DW_BWD_STATS = 11.0   # slab, worst 1.11 / 0.80 / 0.56 (strip heights 0.85 / 0.80 / 0.62)
BAR_BIAS_GRAD = 3.6       # worst 0.36 / 0.32 / 0.18
BAR_PW_BWD = 6.7          # worst, sigmoid' 0.67, SiLU' 0.55 (fp32 kernels)
BAR_TIME_EMBED = 6.8      # worst, temb 0.68, silu_temb 0.53 (fp32 kernel)
BAR_SIN_EMBED = 2.0       # worst 0.00: always inside the ulp of the stored value.  Not measured but reasoned: the device library's cosf and
                          # sinf are accurate to 2 ulp of a result that is at most 1, one of which is the slack, the other at most 2^-24
# the expand GEMM, the Gram statistics, their finalize and FiLM: worst over all cases of tests/test_gpu_expand_gram_kernels.py, as fp16 /
# bf16 (there is no fp32 form), each the worst of seeds 0, 1, 2 (per seed in profiles/r31/README.md); the bar is ten times the worst
BAR_PWX = 4.3             # worst 0.42 / 0.27 (seeds 0, 1, 2: fp16 0.35, 0.42, 0.40; bf16 0.27, 0.13, 0.18)
BAR_PWX_STATS = 17.0      # worst 1.69 / 1.54 (fp16 1.56, 1.42, 1.69; bf16 1.51, 1.54, 1.23)
BAR_GRAM = 30.0           # G, worst 2.39 / 2.94 (fp16 2.21, 2.39, 2.22; bf16 2.88, 2.82, 2.94)
BAR_GRAM_M = 20.0         # m, worst 1.78 / 1.93 (fp16 1.78, 1.50, 1.40; bf16 1.78, 1.62, 1.93)
BAR_GRAM_FIN = 20.0       # worst, scale 2.00 / 1.96, shift 1.91 / 1.84 (the weights' type; the tables are fp32)
BAR_FILM = 9.0            # worst, film 0.86 (seeds: 0.83, 0.86, 0.75), silu_rows 0.53 (fp32 kernels)
