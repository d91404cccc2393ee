"""Plain float64 references of the kernels behind the C ABI's per-kernel entry points, and the comparison helpers of the kernel
tests (tests/test_gpu_forward_kernels.py, tests/test_gpu_boundary_kernels.py, tests/test_forward_refs_host.py,
tests/test_gpu_backward_kernels.py).

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


# ------------------------------------------------------------------------------------------------ llie_init_conv (conv.hip)
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


# ------------------------------------------------------------------------------------------------ llie_final_conv (conv.hip)
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
