"""Float64 restatement of StandardAttention's core (the reference's efficient_unet.py:336-357 after the projections) and of its
gradient, with the error model of the fused kernels of csrc/softattn.hip, for tests/test_gpu_softattn_kernels.py and
tests/test_softattn_host.py.  Method and helpers: tests/kernel_refs.py.

Layout: qkv [B][N][3 * 32 heads] of T (q | k | v, each head-major), out / dout [B][N][32 heads] of T, lse [B][heads][N] fp32.
q, k, v and dout are read as stored in T; everything else is float64.

An entry passes when |out - ref| - slack < BAR * 2^-24 * abssum.  What the kernels round, and where it is granted:
  * S = q . k and dP = dout . v accumulate in fp32 (MFMA), the logit scale * S - m goes through one fp32 exp2.  An fp32 error in a
    logit is a RELATIVE error in p, so every p_ij carries the weight e_ij = scale sum_d |q_id k_jd| + |s_ij| + |m_i| (m_i: the row
    maximum; in the backward pass the given lse_i) next to its own 1.
  * P (and dS in the backward pass) is rounded once to T as the operand of the second product, under a running maximum that a
    reference cannot mirror entry by entry: granted analytically in `slack`, u_T * sum_j p_ij |v_jd| with u_T = 0 / 2^-11 / 2^-8,
    plus for fp16 the subnormal quantum 2^-25 per term whose operand can fall below 2^-14.
  * the stored value: one ulp of T at ref, in `slack`.
abssum per output (all terms non-negative):
  out_id   sum_j p_ij |v_jd| (1 + e_ij)  +  (sum_j p_ij |v_jd|) (1 + sum_k p_ik e_ik)      -- numerator; row sum l_i
  lse_i    1 + |m_i| + |lse_i| + sum_k p_ik e_ik
  dv_jd    sum_i p_ij |dout_id| (1 + e_ij)
  dS_ij    p_ij (|dP_ij - delta_i| (1 + e_ij) + sum_d |dout_id v_jd| + sum_d |dout_id out_id|)  =: a_ij
  dq_id    scale sum_j a_ij |k_jd|;   dk_jd   scale sum_i a_ij |q_id|

BAR_* (house rule: about ten times the worst ratio measured on the MI355X over every case of
tests/test_gpu_softattn_kernels.py, three dtypes, seeds 0, 1 and 2).  Measured worst ratios, fp32 / fp16 / bf16:
  out   0.94 / 0 / 0      (N = 81, hot; the 2-byte results stay inside the slack of the P operand)       bar 10
  lse   1.15 / 0.73 / 0.66 (N = 200, hot; N = 1024, gauss)                                               bar 12
  dqkv  2.37 / 0.92 / 0.63 (N = 200 and 1024, hot)                                                       bar 24
"""
import torch

from kernel_refs import EMIN_T, EPS_T, TDT, U, _rt, _ulp  # noqa: F401

SCALE = 32.0 ** -0.5
U_T = {0: 0.0, 1: 2.0 ** -11, 2: 2.0 ** -8}   # half an ulp of T, relative: one rounding of an MFMA operand
BAR_SOFTATTN_OUT = 10.0
BAR_SOFTATTN_LSE = 12.0
BAR_SOFTATTN_DQKV = 24.0
BLOCK = 64  # keys per streamed block of the kernels (the defects below restate block effects)

DEFECTS = ("drop_last_key", "pad_zero_logits", "no_scale", "swap_heads_kv", "rowsum_before_rescale", "no_delta")


def split_heads(qkv, heads):
    """qkv [B][N][3 * 32 heads] -> q, k, v [B][heads][N][32] float64"""
    B, N, _ = qkv.shape
    return tuple(z.double().view(B, N, heads, 32).permute(0, 2, 1, 3) for z in qkv.split(32 * heads, dim=2))


def rows(t):
    """[B][heads][N][32] -> [B][N][32 heads]"""
    B, h, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, h * 32)


def _sub_slack(p, w, dtype):
    """fp16 only: operands below 2^-14 keep absolute steps of 2^-24 (error 2^-25 each).  p [..i][j] the operand's magnitude bound,
    w the other factor's |.| [..j][d] -> [..i][d]"""
    if dtype != 1:
        return 0.0
    return 2.0 ** -25 * torch.einsum("bhij,bhjd->bhid", (p < 2.0 ** -14).double(), w)


def softattn_ref(qkv, heads, dtype, defect=None):
    """-> dict(out, out_abssum, out_slack [B][N][32 heads]; lse, lse_abssum, lse_slack [B][heads][N]).  `defect`: one of DEFECTS
    (forward ones), the restatement with that mistake built in -- only `out` / `lse` then mean anything."""
    q, k, v = split_heads(qkv, heads)
    N = q.shape[2]
    scale = 1.0 if defect == "no_scale" else SCALE
    if defect == "swap_heads_kv":  # k and v of neighbouring heads exchanged (heads 0 <-> 1, 2 <-> 3, ...)
        perm = torch.arange(heads).view(-1, 2).flip(1).reshape(-1) if heads % 2 == 0 else torch.arange(heads).roll(1)
        k, v = k[:, perm], v[:, perm]
    if defect == "drop_last_key":
        k, v = k[:, :, :-1], v[:, :, :-1]
    if defect == "pad_zero_logits":  # keys past N of the last block admitted as zeros: logit 0, value 0
        pad = (-N) % BLOCK
        z = torch.zeros(k.shape[0], heads, pad, 32, dtype=torch.float64)
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
    s = scale * torch.einsum("bhid,bhjd->bhij", q, k)
    m = s.max(-1, keepdim=True).values
    pe = torch.exp(s - m)
    l = pe.sum(-1, keepdim=True)
    if defect == "rowsum_before_rescale":  # the last block's sum added to a running sum that missed its rescale
        nk = k.shape[2]
        last = (nk - 1) // BLOCK * BLOCK
        if last > 0:
            m0 = s[..., :last].max(-1, keepdim=True).values
            l = torch.exp(s[..., :last] - m0).sum(-1, keepdim=True) + pe[..., last:].sum(-1, keepdim=True)
    p = pe / l
    out = torch.einsum("bhij,bhjd->bhid", p, v)
    lse = (m + torch.log(l)).squeeze(-1)
    res = {"out": rows(out), "lse": lse}
    if defect is not None:
        return res
    e = scale * torch.einsum("bhid,bhjd->bhij", q.abs(), k.abs()) + s.abs() + m.abs()
    pav = torch.einsum("bhij,bhjd->bhid", p, v.abs())
    pe_row = (p * e).sum(-1, keepdim=True)
    res["out_abssum"] = rows(torch.einsum("bhij,bhjd->bhid", p * (1.0 + e), v.abs()) + pav * (1.0 + pe_row))
    # the operand is exp(s - running max) >= exp(s - m) = pe; the accumulated error is scaled by factors <= 1 and by 1 / l
    res["out_slack"] = _ulp(res["out"], dtype) + rows(U_T[dtype] * pav + _sub_slack(pe, v.abs(), dtype) / l)
    res["lse_abssum"] = 1.0 + m.squeeze(-1).abs() + lse.abs() + pe_row.squeeze(-1)
    res["lse_slack"] = _ulp(lse, 0)
    return res


def softattn_bwd_ref(qkv, out, dout, lse, heads, dtype, defect=None):
    """Gradient of the core w.r.t. qkv given dout, with P recomputed from the given `lse` (fp32) and delta from the given `out`
    (T), as the kernels do.  -> dict(dqkv, abssum, slack [B][N][3 * 32 heads]).  defect "no_delta": delta omitted."""
    q, k, v = split_heads(qkv, heads)
    B, N = qkv.shape[0], qkv.shape[1]
    do = dout.double().view(B, N, heads, 32).permute(0, 2, 1, 3)
    oo = out.double().view(B, N, heads, 32).permute(0, 2, 1, 3)
    L = lse.double()[..., None]
    s = SCALE * torch.einsum("bhid,bhjd->bhij", q, k)
    p = torch.exp(s - L)
    delta = (do * oo).sum(-1, keepdim=True)
    if defect == "no_delta":
        delta = torch.zeros_like(delta)
    dP = torch.einsum("bhid,bhjd->bhij", do, v)
    dS = p * (dP - delta)
    dv = torch.einsum("bhij,bhid->bhjd", p, do)
    dq = SCALE * torch.einsum("bhij,bhjd->bhid", dS, k)
    dk = SCALE * torch.einsum("bhij,bhid->bhjd", dS, q)
    res = {"dqkv": torch.cat([rows(dq), rows(dk), rows(dv)], 2)}
    if defect is not None:
        return res
    e = SCALE * torch.einsum("bhid,bhjd->bhij", q.abs(), k.abs()) + s.abs() + L.abs()
    a = p * ((dP - delta).abs() * (1.0 + e) + torch.einsum("bhid,bhjd->bhij", do.abs(), v.abs()) + (do * oo).abs().sum(-1, keepdim=True))
    T = lambda t: t.transpose(2, 3)  # noqa: E731
    dv_a = torch.einsum("bhij,bhid->bhjd", p * (1.0 + e), do.abs())
    dq_a = SCALE * torch.einsum("bhij,bhjd->bhid", a, k.abs())
    dk_a = SCALE * torch.einsum("bhij,bhid->bhjd", a, q.abs())
    u = U_T[dtype]
    dv_s = u * torch.einsum("bhij,bhid->bhjd", p, do.abs()) + _sub_slack(T(p), do.abs(), dtype)
    dq_s = SCALE * (u * torch.einsum("bhij,bhjd->bhid", dS.abs(), k.abs()) + _sub_slack(dS.abs(), k.abs(), dtype))
    dk_s = SCALE * (u * torch.einsum("bhij,bhid->bhjd", dS.abs(), q.abs()) + _sub_slack(T(dS.abs()), q.abs(), dtype))
    res["abssum"] = torch.cat([rows(dq_a), rows(dk_a), rows(dv_a)], 2)
    res["slack"] = _ulp(res["dqkv"], dtype) + torch.cat([rows(dq_s), rows(dk_s), rows(dv_s)], 2)
    return res


# ------------------------------------------------------------------------------------------------ input families
def make_qkv(family, B, N, heads, dtype, gen):
    """qkv [B][N][3 * 32 heads] rounded to T.  gauss: N(0, 0.8^2).  rising: q > 0 and keys growing with their index, so every
    block raises every row's maximum; falling: the same keys in reverse, the maximum sits in the first block.  hot: Gaussian q and
    k scaled so that the scaled logits reach +-100 (an unshifted fp32 exp overflows at 88.7)."""
    inner = 32 * heads
    x = torch.randn(B, N, 3 * inner, generator=gen) * 0.8
    if family in ("rising", "falling"):
        ramp = torch.arange(N, dtype=torch.float32) if family == "rising" else torch.arange(N - 1, -1, -1, dtype=torch.float32)
        x[:, :, :inner] = x[:, :, :inner].abs() + 0.25
        x[:, :, inner:2 * inner] = (0.1 + 1.5 * ramp / max(N - 1, 1))[None, :, None] + 0.02 * x[:, :, inner:2 * inner]
    elif family == "hot":
        q, k, _ = split_heads(x, heads)
        peak = (SCALE * torch.einsum("bhid,bhjd->bhij", q, k)).abs().max().item()
        x[:, :, :2 * inner] *= (100.0 / peak) ** 0.5
    else:
        assert family == "gauss"
    return _rt(x, dtype)
