"""Cases, float64 reference, storage twin and bars of the whole-network backward tests in the half engines
(tests/test_gpu_backward_decisive_net.py, tests/test_backward_decisive_net_host.py).  Method, module twins, rounding operators and
constants: tests/decisive_refs.py -- nothing of it is copied here.

tests/decisive_refs.py holds llie_module_backward to storage-rounding level, one module at a time.  What only the assembled network
runs -- the tape of Run::unet and the backward walk over it, the split of the decoder's cat([h, skip]) gradient and its sum with the
encoder-side gradient, the sum of dfilm over all blocks into time_mlp, the input conv's weight gradient, final_norm / SiLU /
final_conv backwards, llie_unet_backward_dx, every kernel at the layer shapes of the real network -- was judged by cosine >= 0.98
alone in the 2-byte engines.  The decisive construction extends to the network because GroupNorm normalises whatever reaches it:
every block takes the decisive parameters of decisive_refs.build_case (gammas 0.15 .. 0.25, the beta pattern, a small FiLM, the SE
bias pattern behind a small fc1), the rest of the network keeps its ordinary draws, and every ReLU6 pre-activation of all blocks
stays MARGIN_NORM / MARGIN_SE from 0 and 6 (tests/test_backward_decisive_net_host.py).

Storage points of the network, read from Run::unet (forward.cpp) and Back::unet (backward.cpp), in the notation of decisive_refs.py
(`R` rounds the value forward and the gradient backward, `W` the value only, `G` the gradient only); the modules' own points are
listed there and compose unchanged, two consecutive R on a tensor already in T being idempotent:
  lat, cond      W  fp32 NCHW inputs; init_conv_mfma_kernel rounds them to T as its operand and pack_planes rounds them to T as the
                    weight gradient's operand; d(lat) / d(cond) are fp32 outputs of init_conv_dgrad, not rounded
  init_conv      W  forward on the T copy (init_wp); the data gradient (init_conv_dgrad) reads the fp32 weights: the value comes from
                    W(w), d(lat) / d(cond) from w itself; bias fp32; weight gradient: wgrad on T(x) and the stored g0, bias gradient:
                    column sums of g0
  h0             R  init_conv's output is stored in T; its gradient g0 is stored in T by encoder_blocks.0.0's norm1 site
  time embedding    sinusoidal embedding, time_mlp, silu(temb), every FiLM row, dfilm, d(silu(temb)) and the time_mlp backward: fp32
  skips 0 .. 2   R  the level's last output, in T, read by the downsample conv and by the decoder's first block.  Backward: the decoder
                    block's norm1 site stores the skip half's gradient in T (g1); the downsample's input gradient dsrc is stored in T;
                    add_into sums the two T values and stores the sum in T: both rounded first, the sum rounded once more
  skip 3         R  aliases mid_block1's input.  Backward: decoder_blocks.0.0 stores g1 in T; mid_block1's norm1 site adds it (a1_0) to
                    its own fp32 input gradient and rounds once: only the decoder's part is rounded before the sum
  cat([h, skip])    virtual: the first block of a decoder level reads both tensors in place (x0 = h, x1 = skip, both in T) and its norm1
                    site writes g0 and g1 apart, each rounded once
  upsamplers     -  as decisive_refs.up_twin (the training forward keeps the up-sampled tensor in T)
  final_norm     G  on norm(h): gn_site_bwd stores dz = da silu'(z) in T before the norm's backward reads it
  silu(norm(h))  R  rounded to T as final_conv_mfma_kernel's operand; final_bwd_data stores da in T
  final_conv     W  forward on the T copy (fin_wp); final_bwd_data reads the fp32 weights and the fp32 cotangent; the weight and bias
                    gradients read the cotangent packed to T (pack_planes): G on the prediction for those two alone
  prediction        fp32, not rounded
The twin leaves out what decisive_refs.py's leaves out.  With Twin(None) it is oracle.unet_ref.unet_forward on .double() tensors,
both with the sinusoidal embedding of `embedding` below (the engine's frequency table; the function says why).

Cases, the smallest frames the engine takes (frame_shape_ok: H, W >= 64, multiples of 8), module tree of image_size = 64:
  small 64 x 64, B = 2, t = (500, 37)            every level on whole tiles, 8 x 8 at the bottleneck
  small 72 x 88, B = 2, t = (999, 0)             72 x 88, 36 x 44, 18 x 22, 9 x 11: ragged at every level, H != W, both schedule ends
  small 64 x 64, B = 2, use_linear_attention=False   StandardAttention (softattn_twin).  oracle.unet_forward has no softmax attention:
                                                 for this case the twin with Twin(None) is the reference (its softattn_twin is
                                                 checked against torch's scaled_dot_product_attention in
                                                 tests/test_backward_decisive_host.py, the rest of it against the oracle by the two
                                                 cases above)
  large 64 x 64, B = 1 is left out.  Its float64 reference and two twins take 33 s together on 16 CPU threads, within the minute it
  was allowed, and its margins hold (1.68 / 2.16 / 1.04 over its 30 blocks), but it misses the range condition on the cases
  (test_gradient_range): 1.14 % of the non-zero entries of the gradients of decoder level 3's four outputs lie below fp16's smallest
  normal, 6.1e-5, where fewer than 1 % are allowed -- an fp16 engine would need a loss scale there, which these tests do not use.
  LARGE_CASE keeps it for measurements.
"""
import contextlib
import os
import re
import sys
from collections import namedtuple

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
from decisive_refs import (FACTOR, FILM_SCALE, SE_FC1_SCALE, SEED0, Twin, _gn, _pattern, down_twin, irb_twin, linattn_twin,  # noqa: E402,F401
                           rel_err, softattn_twin, up_twin)
from kernel_refs import seeded, sin_freqs  # noqa: E402
from oracle import unet_ref  # noqa: E402

SIZE = 64  # image_size of every model here: it fixes the module tree (attention at levels 2 and 3)

# variant; H, W: the frame; B; t: one timestep per sample; linear: use_linear_attention
NetCase = namedtuple("NetCase", "variant H W B t linear")
NET_CASES = [
    NetCase("small", 64, 64, 2, (500, 37), True),
    NetCase("small", 72, 88, 2, (999, 0), True),
    NetCase("small", 64, 64, 2, (500, 37), False),
]
LARGE_CASE = NetCase("large", 64, 64, 1, (500,), True)  # not among the cases: see the module docstring


def case_id(c):
    return f"{c.variant}-{c.H}x{c.W}-B{c.B}" + ("" if c.linear else "-softmax")


def spec_of(c):
    return oracle.make_spec(c.variant, SIZE)


# ------------------------------------------------------------------------------------------------ state dict
def _blocks(spec):
    plan = oracle.block_plan(spec)
    return [b for lvl in plan["enc"] for b in lvl] + list(plan["mid"]) + [b for lvl in plan["dec"] for b in lvl]


def net_shapes(spec, linear=True):
    """key -> shape under the model's own keys (EfficientUNet.state_dict()); StandardAttention has to_out.weight and no to_out.1"""
    out = {}
    for k, s in oracle.param_shapes(spec, prefix="").items():
        if not linear and ".to_out.1." in k:
            continue
        out[k if linear else k.replace(".to_out.0.weight", ".to_out.weight")] = s
    return out


def build_net(variant, seed0=None, linear=True):
    """The decisive state dict of a whole network (fp32, EfficientUNet's keys): oracle.synth_state_dict draws, every block with the
    decisive parameters of decisive_refs.build_case -- norm1 / norm2 gammas in 0.15 .. 0.25 and betas in the pattern, se.fc1.bias in
    the pattern, time_mlp.1 scaled by FILM_SCALE (its bias to 0.02), se.fc1.weight by SE_FC1_SCALE.  The network's time_mlp,
    init_conv, attention modules, samplers, final_norm and final_conv stay ordinary draws.  LLIE_FWD_TEST_SEED shifts every seed."""
    seed = SEED0 if seed0 is None else seed0
    spec = oracle.make_spec(variant, SIZE)
    sd = oracle.synth_state_dict(net_shapes(spec, linear), seed)
    for b in _blocks(spec):
        if b[0] != "irb":
            continue
        pre = b[1]
        g = seeded(seed, "decisive-net", variant, pre)
        ru = lambda lo, hi, n: lo + (hi - lo) * torch.rand(n, generator=g)  # noqa: E731
        cin, hid, sq = b[2], sd[pre + ".expand.weight"].shape[0], sd[pre + ".se.fc1.bias"].shape[0]
        sd[pre + ".norm1.weight"], sd[pre + ".norm1.bias"] = ru(0.15, 0.25, cin), _pattern(cin, g)
        sd[pre + ".norm2.weight"], sd[pre + ".norm2.bias"] = ru(0.15, 0.25, hid), _pattern(hid, g)
        sd[pre + ".se.fc1.weight"] = SE_FC1_SCALE * sd[pre + ".se.fc1.weight"]
        sd[pre + ".se.fc1.bias"] = _pattern(sq, g)
        sd[pre + ".time_mlp.1.weight"] = FILM_SCALE * sd[pre + ".time_mlp.1.weight"]
        sd[pre + ".time_mlp.1.bias"] = 0.2 * sd[pre + ".time_mlp.1.bias"]
    return sd


def build_inputs(c, seed0=None):
    """-> (lat, cond, t, cot): the two input halves [B][3][H][W], the timesteps, the cotangent of the prediction.  The cotangent is
    uniform in (-0.5, 1.5), for the reason decisive_refs.build_case gives."""
    g = seeded(SEED0 if seed0 is None else seed0, "decisive-net-in", *c)
    ru = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)  # noqa: E731
    lat, cond = ru(-2, 2, c.B, 3, c.H, c.W), ru(-1, 1, c.B, 3, c.H, c.W)
    return lat, cond, torch.tensor(c.t), ru(-0.5, 1.5, c.B, 3, c.H, c.W)


# ------------------------------------------------------------------------------------------------ the network, float64
class _SwapSplit(torch.autograd.Function):
    """cat([h, skip]) whose gradient halves change places (equal channel counts): a wrong backward of the host test"""

    @staticmethod
    def forward(ctx, h, s):
        ctx.c = h.shape[1]
        return torch.cat([h, s], 1)

    @staticmethod
    def backward(ctx, g):
        return g[:, ctx.c:], g[:, :ctx.c]


def _two_path(val, *paths):
    """the value `val` (detached) with the gradients of `paths`, whose values cancel exactly"""
    out = val.detach()
    for q in paths:
        out = out + (q - q.detach())
    return out


def embedding(t, dim, dtype=torch.float64):
    """SinusoidalPosEmb (efficient_unet.py:68-76) from the frequency table as the engine tabulates it (kernel_refs.sin_freqs: the
    fp32 chain of the reference, its exp correctly rounded) and the fp32 argument t * f, cos / sin in float64.  oracle.
    sinusoidal_embedding takes torch's vectorised fp32 exp, which on some CPUs returns a frequency one ulp off (dim = 64: entry 3
    on one machine, entry 11 on another); at t = 500 that moves an entry of the embedding by 1.4e-5, which the fp32 engine's bars
    (1e-5 of time_mlp.1.weight's largest entry) would charge to the engine.  The engine's own embedding is within 5e-8 of this one
    (measured on the MI355X for both table sizes)."""
    arg = (t.float()[:, None] * sin_freqs(dim)[None, :]).double()
    return torch.cat([arg.cos(), arg.sin()], 1).to(dtype)


@contextlib.contextmanager
def oracle_embedding(dtype):
    """oracle.unet_forward with the embedding above, handed on in `dtype` (float64 weights do not accept the oracle's fp32 one)"""
    orig = unet_ref.sinusoidal_embedding
    unet_ref.sinusoidal_embedding = lambda t, dim, max_period=10000.0: embedding(t, dim, dtype)
    try:
        yield
    finally:
        unet_ref.sinusoidal_embedding = orig


MUTATIONS = ("skip_detached", "split_swapped", "film_block_missing", "dcond_from_lat")
# The block whose FiLM contribution "film_block_missing" keeps out of d(temb).  A block's share of d(temb) differs: in small at 64 x 64
# this one's absence moves time_mlp.1.* by 0.25 and time_mlp.3.* by 0.29 of their largest entries, a bottleneck block's (mid_block1,
# decoder_blocks.0.0) by 0.11 .. 0.12 and 0.14 .. 0.17 -- above every bar but bf16's time_mlp.1.* (0.16), which the spread rule set.
FILM_MISSING_BLOCK = "decoder_blocks.3.2"


def net_twin(tw, spec, p, lat, cond, t, mut=None, info=None):
    """oracle.unet_ref.unet_forward (EfficientUNet.forward, efficient_unet.py:532-606) composed from the module twins, with the
    roundings of `tw` at the network's storage points (module docstring).  p: leaves by the model's keys; lat, cond: the two halves
    of the input; t: int64 timesteps.  info (dict): receives "margins" {block: (norm1, norm2, se)}, "film" (largest |FiLM| entry) and
    "acts" [(name, tensor)], every inter-module tensor.  mut: one of MUTATIONS, a wrong backward pass with the right forward --
      skip_detached       the encoder skips' gradients are dropped
      split_swapped       the two halves of the gradient of decoder level 0's cat([h, skip]) change places
      film_block_missing  FILM_MISSING_BLOCK's FiLM contribution is missing from d(temb)
      dcond_from_lat      d(cond) is taken from the latent channels of init_conv.weight"""
    R, W, G = tw.R, tw.W, tw.G
    plan, heads = oracle.block_plan(spec), spec.num_attention_heads
    soft = "mid_attn.to_out.weight" in p
    sub = {}
    for k, v in p.items():
        m = re.match(r"((?:encoder_blocks|decoder_blocks)\.\d+\.\d+|mid_block[12]|mid_attn|downsamplers\.\d+|upsamplers\.\d+)\.(.*)", k)
        if m:
            sub.setdefault(m.group(1), {})[m.group(2)] = v
    acts, margins, films = [], {}, []

    def note(name, h):
        acts.append((name, h))
        return h

    def run(blocks, h):
        for b in blocks:
            if b[0] == "irb":
                inf = {}
                te = temb.detach() if (mut == "film_block_missing" and b[1] == FILM_MISSING_BLOCK) else temb
                h = irb_twin(tw, sub[b[1]], h, te, info=inf)
                margins[b[1]] = (inf["norm1"], inf["norm2"], inf["se"])
                films.append(F.linear(F.silu(temb), sub[b[1]]["time_mlp.1.weight"], sub[b[1]]["time_mlp.1.bias"]).abs().max().item())
                last_x[0] = inf["x"]
            else:
                h = (softattn_twin if soft else linattn_twin)(tw, sub[b[1]], h, heads)
            note(b[1], h)
        return h

    last_x = [None]
    # time embedding: fp32 in the engine, nothing rounded
    emb = embedding(t, spec.base_channels, lat.dtype)
    hidden = F.silu(F.linear(emb, p["time_mlp.1.weight"], p["time_mlp.1.bias"]))
    temb = F.linear(hidden, p["time_mlp.3.weight"], p["time_mlp.3.bias"])
    # input conv
    x = W(torch.cat([lat, cond], 1))
    w0 = p["init_conv.weight"]
    wd = w0.detach()
    if mut == "dcond_from_lat":
        half = lat.shape[1]
        wd = torch.cat([wd[:, :half], wd[:, :half]], 1)
    conv1 = lambda a, w: F.conv2d(a, w, padding=1)  # noqa: E731
    b0 = p["init_conv.bias"][None, :, None, None]
    h = _two_path(conv1(x, W(w0)) + b0, conv1(x.detach(), w0) + b0, conv1(x, wd))
    h = note("init_conv", R(h))
    # encoder
    skips = []
    for lvl, blocks in enumerate(plan["enc"]):
        h = run(blocks, h)
        skips.append(h)
        if lvl < len(plan["enc"]) - 1:
            h = note(f"downsamplers.{lvl}", down_twin(tw, sub[f"downsamplers.{lvl}"], h))
    # middle: mid_block1's stored input is the last skip; the decoder's gradient of it joins mid_block1's own before the one rounding
    h = run(plan["mid"][:1], h)
    skips[-1] = last_x[0]
    h = run(plan["mid"][1:], h)
    if mut == "skip_detached":
        skips = [s.detach() for s in skips]
    # decoder
    for lvl, blocks in enumerate(plan["dec"]):
        if lvl > 0:
            h = note(f"upsamplers.{lvl - 1}", up_twin(tw, sub[f"upsamplers.{lvl - 1}"], h))
        s = skips.pop()
        h = _SwapSplit.apply(h, s) if (mut == "split_swapped" and lvl == 0) else torch.cat([h, s], 1)
        h = run(blocks, h)
    # output head
    a = R(F.silu(G(_gn(h, p["final_norm.weight"], p["final_norm.bias"]))))
    wf, bf = p["final_conv.weight"], p["final_conv.bias"][None, :, None, None]
    pred = _two_path(conv1(a, W(wf)) + bf, conv1(a, wf.detach()), G(conv1(a.detach(), wf) + bf))
    if info is not None:
        info.update(margins=margins, film=max(films), acts=acts)
    return pred


def _leaves(c, seed0, dtype=torch.float64):
    sd = build_net(c.variant, seed0, c.linear)
    lat, cond, t, cot = build_inputs(c, seed0)
    p = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    return p, lat.to(dtype).requires_grad_(True), cond.to(dtype).requires_grad_(True), t, cot.to(dtype)


def _collect(p, lat, cond, pred):
    out = {k: v.grad for k, v in p.items()}
    out["lat"], out["cond"], out["pred"] = lat.grad, cond.grad, pred.detach()
    return out


def net_grads(c, cd=None, seed0=None, mut=None, info=None):
    """The float64 gradients of sum(pred * cot): {parameter key: gradient, "lat": .., "cond": .., "pred": the prediction itself}.
    cd None: the reference; "bf16" / "fp16": the storage twin.  info: see net_twin; also receives "dacts" {name: gradient of that
    inter-module tensor}."""
    p, lat, cond, t, cot = _leaves(c, seed0)
    info = {} if info is None else info
    pred = net_twin(Twin(cd), spec_of(c), p, lat, cond, t, mut, info)
    for _, h in info["acts"]:
        h.retain_grad()
    (pred * cot).sum().backward()
    info["dacts"] = {n: h.grad for n, h in info.pop("acts")}
    return _collect(p, lat, cond, pred)


def cpu32_grads(c, seed0=None):
    """The same gradients from a float32 evaluation on the CPU: oracle.unet_forward with autograd, or (the softmax network, which the
    oracle cannot express) the twin without a type on float32 tensors.  The yardstick of the fp32 engine's bars."""
    p, lat, cond, t, cot = _leaves(c, seed0, torch.float32)
    if c.linear:
        with oracle_embedding(torch.float32):
            pred = oracle.unet_forward(p, spec_of(c), torch.cat([lat, cond], 1), t, prefix="")
    else:
        pred = net_twin(Twin(None), spec_of(c), p, lat, cond, t)
    (pred * cot).sum().backward()
    return _collect(p, lat, cond, pred)


# ------------------------------------------------------------------------------------------------ classes and bars
def tensor_class(key):
    """-> (class, level): (module kind, parameter key) and the resolution level (0: the frame, 3: the bottleneck; None for the
    tensors outside the levels).  Both attention kinds are "attn": a network has one of them."""
    m = re.match(r"(encoder_blocks|decoder_blocks)\.(\d+)\.\d+\.(.*)", key)
    if m:
        lvl = int(m.group(2)) if m.group(1) == "encoder_blocks" else 3 - int(m.group(2))
        kind = "irb" if (m.group(3).startswith(("norm1", "norm2", "expand", "depthwise", "se.", "project", "time_mlp", "skip"))) else "attn"
        return f"{kind}.{m.group(3)}", lvl
    m = re.match(r"mid_block[12]\.(.*)", key)
    if m:
        return "irb." + m.group(1), 3
    m = re.match(r"mid_attn\.(.*)", key)
    if m:
        return "attn." + m.group(1), 3
    m = re.match(r"downsamplers\.(\d+)\.(.*)", key)
    if m:
        return "downsamplers." + m.group(2), int(m.group(1))
    m = re.match(r"upsamplers\.(\d+)\.(.*)", key)
    if m:
        return "upsamplers." + m.group(2), 2 - int(m.group(1))
    return key, None  # time_mlp.{1,3}.*, init_conv.*, final_norm.*, final_conv.*, lat, cond, pred


def twin_errors(cd, seed0, cases=None):
    """{(class, level): worst rel_err of the twin against the float64 reference over the cases} for one seed; the softmax network's
    attention classes are kept apart ("softattn....")"""
    worst = {}
    for c in (NET_CASES if cases is None else cases):
        ref, tw = net_grads(c, None, seed0), net_grads(c, cd, seed0)
        for k in ref:
            cl, lvl = class_of(c, k)
            worst[(cl, lvl)] = max(worst.get((cl, lvl), 0.0), rel_err(tw[k], ref[k]))
    return worst


def class_of(c, key):
    cl, lvl = tensor_class(key)
    if not c.linear and cl.startswith("attn."):
        cl = "soft" + cl
    return cl, lvl


def form_table(per_seed):
    """The rule of the table from twin_errors of the seeds: a class whose worst value differs by more than 2x between levels is split
    by level ("class@level"); each entry is (twin's worst over the seeds, bar) with bar = FACTOR x worst, or 1.5 x spread x worst
    where the worst value moves by more than 2x between the seeds (spread = largest / smallest).  -> {name: (worst, bar, per-seed)}"""
    classes = sorted({cl for e in per_seed for cl, _ in e})
    table = {}
    for cl in classes:
        levels = sorted({lvl for e in per_seed for c2, lvl in e if c2 == cl}, key=lambda v: -1 if v is None else v)
        by_level = {lvl: [e[(cl, lvl)] for e in per_seed] for lvl in levels}
        tops = [max(v) for v in by_level.values()]
        groups = {f"{cl}@{lvl}": v for lvl, v in by_level.items()} if max(tops) > 2 * min(tops) else \
            {cl: [max(v[i] for v in by_level.values()) for i in range(len(per_seed))]}
        for name, v in groups.items():
            spread = max(v) / max(min(v), 1e-300)
            table[name] = (max(v), max(v) * (1.5 * spread if spread > 2 else FACTOR), v)
    return table


# One bar per (dtype, class) on rel_err = max |g - g_ref| / max |g_ref|, formed by form_table from the twin's errors against the
# float64 reference over NET_CASES and seeds 0, 1, 2 -- from the reference side alone (tests/test_backward_decisive_net_host.py
# recomputes seed 0 by default, all three and the rule itself with LLIE_DECISIVE_ALL_SEEDS=1).  Each entry: (twin's worst, bar),
# both rounded up to two digits; "class@level" where the twin's error differs by more than 2x between the levels; the comments carry
# the spread where it set the bar, and the worst value measured on the MI355X over the cases of
# tests/test_gpu_backward_decisive_net.py (seed 0).
#
# upsamplers.conv.bias@0 carries no information and its bar says so: level 0 has 32 channels in 32 groups, every GroupNorm there
# (final_norm included) normalises each channel alone and the residuals hand a constant on unchanged, so a constant added to a channel
# of upsamplers.2's output reaches the prediction only through decoder_blocks.3.0's norm1 over the 96 concatenated channels (groups of
# three).  The gradient cancels to about 1e-5 of its terms: the float32 CPU evaluation itself is 0.7 % off.
NET_BARS = {
    "bf16": {
        # MI355X, worst over the three cases (largest share of a bar: 0.44, init_conv.weight in the softmax network):
        # attn.norm.bias 0.036, attn.norm.weight 0.032, attn.to_out.0.weight@2 0.045, attn.to_out.0.weight@3 0.029,
        # attn.to_out.1.bias 0.016, attn.to_out.1.weight 0.02, attn.to_qkv.weight 0.034, cond 0.022, downsamplers.down.bias 0.013,
        # downsamplers.down.weight 0.017, final_conv.bias 4.2e-05, final_conv.weight 0.0038, final_norm.bias 0.0017,
        # final_norm.weight 0.0022, init_conv.bias 0.012, init_conv.weight 0.025, irb.depthwise.weight 0.018,
        # irb.expand.weight 0.05, irb.norm1.bias 0.024, irb.norm1.weight@0 0.042, irb.norm1.weight@1 0.033,
        # irb.norm1.weight@2 0.02, irb.norm1.weight@3 0.034, irb.norm2.bias 0.042, irb.norm2.weight 0.034,
        # irb.project.weight 0.021, irb.se.fc1.bias@0 0.016, irb.se.fc1.bias@1 0.017, irb.se.fc1.bias@2 0.024,
        # irb.se.fc1.bias@3 0.02, irb.se.fc1.weight@0 0.017, irb.se.fc1.weight@1 0.019, irb.se.fc1.weight@2 0.024,
        # irb.se.fc1.weight@3 0.019, irb.se.fc2.bias 0.029, irb.se.fc2.weight 0.029, irb.skip.weight 0.023,
        # irb.time_mlp.1.bias 0.043, irb.time_mlp.1.weight 0.047, lat 0.02, pred 0.024 (inference forward: 0.024), softattn.norm.bias
        # 0.018, softattn.norm.weight 0.022, softattn.to_out.weight 0.014, softattn.to_qkv.weight 0.017, time_mlp.1.bias 0.013,
        # time_mlp.1.weight 0.013, time_mlp.3.bias 0.018, time_mlp.3.weight 0.02, upsamplers.conv.bias@0 5.7,
        # upsamplers.conv.bias@1 0.014, upsamplers.conv.bias@2 0.0096, upsamplers.conv.weight 0.016
        "attn.norm.bias": (0.083, 0.35),  # seeds 0.03 .. 0.083, spread 2.73: 1.5 x spread
        "attn.norm.weight": (0.071, 0.26),  # seeds 0.03 .. 0.07, spread 2.36: 1.5 x spread
        "attn.to_out.0.weight@2": (0.14, 0.67),  # seeds 0.041 .. 0.13, spread 3.18: 1.5 x spread
        "attn.to_out.0.weight@3": (0.043, 0.13),
        "attn.to_out.1.bias": (0.038, 0.12),
        "attn.to_out.1.weight": (0.04, 0.13),  # seeds 0.019 .. 0.039, spread 2.10: 1.5 x spread
        "attn.to_qkv.weight": (0.067, 0.21),
        "cond": (0.028, 0.084),
        "downsamplers.down.bias": (0.043, 0.18),  # seeds 0.016 .. 0.042, spread 2.73: 1.5 x spread
        "downsamplers.down.weight": (0.034, 0.11),
        "final_conv.bias": (4.3e-05, 0.00013),
        "final_conv.weight": (0.0076, 0.023),
        "final_norm.bias": (0.0018, 0.0057),  # seeds 0.00082 .. 0.0017, spread 2.10: 1.5 x spread
        "final_norm.weight": (0.0064, 0.027),  # seeds 0.0023 .. 0.0064, spread 2.75: 1.5 x spread
        "init_conv.bias": (0.027, 0.081),
        "init_conv.weight": (0.019, 0.057),
        "irb.depthwise.weight": (0.041, 0.13),
        "irb.expand.weight": (0.061, 0.19),
        "irb.norm1.bias": (0.057, 0.19),  # seeds 0.026 .. 0.057, spread 2.20: 1.5 x spread
        "irb.norm1.weight@0": (0.055, 0.17),
        "irb.norm1.weight@1": (0.05, 0.15),
        "irb.norm1.weight@2": (0.089, 0.42),  # seeds 0.028 .. 0.089, spread 3.13: 1.5 x spread
        "irb.norm1.weight@3": (0.039, 0.12),
        "irb.norm2.bias": (0.052, 0.16),
        "irb.norm2.weight": (0.07, 0.21),
        "irb.project.weight": (0.035, 0.11),
        "irb.se.fc1.bias@0": (0.059, 0.34),  # seeds 0.016 .. 0.059, spread 3.75: 1.5 x spread
        "irb.se.fc1.bias@1": (0.029, 0.087),
        "irb.se.fc1.bias@2": (0.035, 0.11),
        "irb.se.fc1.bias@3": (0.039, 0.12),
        "irb.se.fc1.weight@0": (0.06, 0.35),  # seeds 0.016 .. 0.059, spread 3.79: 1.5 x spread
        "irb.se.fc1.weight@1": (0.029, 0.087),
        "irb.se.fc1.weight@2": (0.037, 0.12),
        "irb.se.fc1.weight@3": (0.041, 0.13),
        "irb.se.fc2.bias": (0.069, 0.29),  # seeds 0.025 .. 0.069, spread 2.71: 1.5 x spread
        "irb.se.fc2.weight": (0.069, 0.29),  # seeds 0.025 .. 0.069, spread 2.71: 1.5 x spread
        "irb.skip.weight": (0.042, 0.14),  # seeds 0.019 .. 0.042, spread 2.15: 1.5 x spread
        "irb.time_mlp.1.bias": (0.056, 0.17),
        "irb.time_mlp.1.weight": (0.053, 0.16),
        "lat": (0.031, 0.093),
        "pred": (0.026, 0.078),
        "softattn.norm.bias": (0.018, 0.054),
        "softattn.norm.weight": (0.028, 0.084),
        "softattn.to_out.weight": (0.021, 0.063),
        "softattn.to_qkv.weight": (0.025, 0.075),
        "time_mlp.1.bias": (0.04, 0.16),  # seeds 0.016 .. 0.039, spread 2.54: 1.5 x spread
        "time_mlp.1.weight": (0.04, 0.16),  # seeds 0.016 .. 0.039, spread 2.54: 1.5 x spread
        "time_mlp.3.bias": (0.028, 0.084),
        "time_mlp.3.weight": (0.03, 0.09),
        "upsamplers.conv.bias@0": (7.0, 43.0),  # seeds 1.7 .. 7, spread 4.01: 1.5 x spread (cancels: see above)
        "upsamplers.conv.bias@1": (0.024, 0.087),  # seeds 0.0099 .. 0.024, spread 2.41: 1.5 x spread
        "upsamplers.conv.bias@2": (0.023, 0.086),  # seeds 0.0092 .. 0.023, spread 2.47: 1.5 x spread
        "upsamplers.conv.weight": (0.027, 0.081),
    },
    "fp16": {
        # MI355X, worst over the three cases (largest share of a bar: 0.34, irb.se.fc1.bias@1 in the softmax network):
        # attn.norm.bias@2 0.0037, attn.norm.bias@3 0.0025, attn.norm.weight@2 0.0039, attn.norm.weight@3 0.003,
        # attn.to_out.0.weight@2 0.0056, attn.to_out.0.weight@3 0.0028, attn.to_out.1.bias 0.0025, attn.to_out.1.weight 0.0034,
        # attn.to_qkv.weight@2 0.0033, attn.to_qkv.weight@3 0.0027, cond 0.003, downsamplers.down.bias 0.0024,
        # downsamplers.down.weight 0.0027, final_conv.bias 5.5e-06, final_conv.weight 0.00043, final_norm.bias 8.1e-05,
        # final_norm.weight 0.00029, init_conv.bias 0.0022, init_conv.weight 0.0023, irb.depthwise.weight 0.0026,
        # irb.expand.weight@0 0.003, irb.expand.weight@1 0.0032, irb.expand.weight@2 0.0029, irb.expand.weight@3 0.0036,
        # irb.norm1.bias@0 0.0029, irb.norm1.bias@1 0.0026, irb.norm1.bias@2 0.0025, irb.norm1.bias@3 0.0032,
        # irb.norm1.weight 0.0053, irb.norm2.bias 0.0042, irb.norm2.weight 0.0045, irb.project.weight 0.0028,
        # irb.se.fc1.bias@0 0.0026, irb.se.fc1.bias@1 0.0024, irb.se.fc1.bias@2 0.0028, irb.se.fc1.bias@3 0.0032,
        # irb.se.fc1.weight@0 0.0026, irb.se.fc1.weight@1 0.0023, irb.se.fc1.weight@2 0.0029, irb.se.fc1.weight@3 0.0032,
        # irb.se.fc2.bias 0.0039, irb.se.fc2.weight 0.0039, irb.skip.weight 0.0026, irb.time_mlp.1.bias 0.004,
        # irb.time_mlp.1.weight 0.0039, lat 0.003, pred 0.0029 (inference forward: 0.0031), softattn.norm.bias 0.0021,
        # softattn.norm.weight 0.0025, softattn.to_out.weight 0.0018, softattn.to_qkv.weight 0.002, time_mlp.1.bias 0.0015,
        # time_mlp.1.weight 0.0015, time_mlp.3.bias 0.0024, time_mlp.3.weight 0.0024, upsamplers.conv.bias@0 0.95,
        # upsamplers.conv.bias@1 0.0018, upsamplers.conv.bias@2 0.0021, upsamplers.conv.weight 0.0019
        "attn.norm.bias@2": (0.022, 0.19),  # seeds 0.0037 .. 0.021, spread 5.70: 1.5 x spread
        "attn.norm.bias@3": (0.0046, 0.014),
        "attn.norm.weight@2": (0.014, 0.065),  # seeds 0.0045 .. 0.014, spread 3.06: 1.5 x spread
        "attn.norm.weight@3": (0.0045, 0.014),
        "attn.to_out.0.weight@2": (0.026, 0.21),  # seeds 0.0049 .. 0.026, spread 5.21: 1.5 x spread
        "attn.to_out.0.weight@3": (0.0047, 0.015),
        "attn.to_out.1.bias": (0.004, 0.012),
        "attn.to_out.1.weight": (0.0042, 0.013),
        "attn.to_qkv.weight@2": (0.016, 0.12),  # seeds 0.0033 .. 0.016, spread 4.66: 1.5 x spread
        "attn.to_qkv.weight@3": (0.0036, 0.011),
        "cond": (0.003, 0.009),
        "downsamplers.down.bias": (0.004, 0.012),
        "downsamplers.down.weight": (0.003, 0.009),
        "final_conv.bias": (8.1e-06, 2.9e-05),  # seeds 3.4e-06 .. 8e-06, spread 2.32: 1.5 x spread
        "final_conv.weight": (0.00077, 0.0024),
        "final_norm.bias": (0.00035, 0.0024),  # seeds 7.7e-05 .. 0.00035, spread 4.54: 1.5 x spread
        "final_norm.weight": (0.00046, 0.0014),
        "init_conv.bias": (0.0031, 0.0093),
        "init_conv.weight": (0.0028, 0.0084),
        "irb.depthwise.weight": (0.0042, 0.013),
        "irb.expand.weight@0": (0.0047, 0.015),
        "irb.expand.weight@1": (0.0035, 0.011),
        "irb.expand.weight@2": (0.0069, 0.028),  # seeds 0.0026 .. 0.0068, spread 2.68: 1.5 x spread
        "irb.expand.weight@3": (0.0072, 0.023),  # seeds 0.0035 .. 0.0071, spread 2.04: 1.5 x spread
        "irb.norm1.bias@0": (0.0079, 0.027),  # seeds 0.0036 .. 0.0079, spread 2.20: 1.5 x spread
        "irb.norm1.bias@1": (0.004, 0.012),
        "irb.norm1.bias@2": (0.0057, 0.018),
        "irb.norm1.bias@3": (0.0039, 0.012),
        "irb.norm1.weight": (0.0058, 0.018),
        "irb.norm2.bias": (0.006, 0.018),
        "irb.norm2.weight": (0.0061, 0.019),
        "irb.project.weight": (0.0039, 0.012),
        "irb.se.fc1.bias@0": (0.0053, 0.017),  # seeds 0.0025 .. 0.0052, spread 2.13: 1.5 x spread
        "irb.se.fc1.bias@1": (0.0024, 0.0072),
        "irb.se.fc1.bias@2": (0.0043, 0.013),
        "irb.se.fc1.bias@3": (0.0038, 0.012),
        "irb.se.fc1.weight@0": (0.0053, 0.018),  # seeds 0.0024 .. 0.0052, spread 2.18: 1.5 x spread
        "irb.se.fc1.weight@1": (0.0024, 0.0072),
        "irb.se.fc1.weight@2": (0.0043, 0.013),
        "irb.se.fc1.weight@3": (0.0039, 0.012),
        "irb.se.fc2.bias": (0.0065, 0.021),  # seeds 0.0032 .. 0.0065, spread 2.05: 1.5 x spread
        "irb.se.fc2.weight": (0.0065, 0.021),  # seeds 0.0032 .. 0.0065, spread 2.05: 1.5 x spread
        "irb.skip.weight": (0.0032, 0.0096),
        "irb.time_mlp.1.bias": (0.006, 0.018),
        "irb.time_mlp.1.weight": (0.006, 0.018),
        "lat": (0.0032, 0.0096),
        "pred": (0.0034, 0.011),  # seeds 0.0015 .. 0.0033, spread 2.14: 1.5 x spread
        "softattn.norm.bias": (0.0024, 0.0072),
        "softattn.norm.weight": (0.003, 0.009),
        "softattn.to_out.weight": (0.0024, 0.0072),
        "softattn.to_qkv.weight": (0.003, 0.009),
        "time_mlp.1.bias": (0.002, 0.006),
        "time_mlp.1.weight": (0.002, 0.006),
        "time_mlp.3.bias": (0.0027, 0.0081),
        "time_mlp.3.weight": (0.0028, 0.0084),
        "upsamplers.conv.bias@0": (1.3, 3.9),  # cancels: see above
        "upsamplers.conv.bias@1": (0.0019, 0.0057),
        "upsamplers.conv.bias@2": (0.0047, 0.022),  # seeds 0.0016 .. 0.0046, spread 2.98: 1.5 x spread
        "upsamplers.conv.weight": (0.0023, 0.0069),
    },
}


def bar(cd, c, key):
    cl, lvl = class_of(c, key)
    t = NET_BARS[cd]
    return t[f"{cl}@{lvl}"][1] if f"{cl}@{lvl}" in t else t[cl][1]


def bar_name(cd, c, key):
    cl, lvl = class_of(c, key)
    return f"{cl}@{lvl}" if f"{cl}@{lvl}" in NET_BARS[cd] else cl


FP32_FACTOR, FP32_FLOOR = 8.0, 1e-6


def fp32_bars(c, ref, seed0=None):
    """The fp32 engine's bar per tensor (the rule of tests/test_gpu_x0loss.py): 8 x what the float32 CPU evaluation of the same network
    differs from the float64 reference, at least 1e-6, relative to the tensor's largest entry.  The 8 covers summation order and FMA
    contraction.  Computed, not tabulated.  MI355X: the fp32 engine's largest share of a bar is 0.90 (a block's norm2.weight in small
    at 64 x 64: 2.6e-5 of its largest entry), 0.55 at 72 x 88, 0.22 in the softmax network; the prediction is within 3.2e-6."""
    c32 = cpu32_grads(c, seed0)
    return {k: max(FP32_FACTOR * rel_err(c32[k], ref[k]), FP32_FLOOR) for k in ref}


def over_bar(bars, got, ref):
    """{tensor: (rel_err, bar)} of the tensors in `got` that miss their bar against `ref` (non-finite ones included), and the rel_err
    of every tensor.  bars: {tensor: bar}."""
    worst = {k: (rel_err(got[k], ref[k]) if torch.isfinite(got[k]).all() else float("inf")) for k in ref}
    return {k: (v, bars[k]) for k, v in worst.items() if not v < bars[k]}, worst


def half_bars(cd, c, ref):
    return {k: bar(cd, c, k) for k in ref}
