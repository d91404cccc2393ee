"""GPU parity at BASELINE's real shapes and the operator-level KATs added in round 2 (through the C ABI).

  * fp16 / bf16 small@256 against the reference-generated samples of tests/golden/enhance_small256.npz (config 2)
  * `large` against reference outputs (tests/golden/large_kat.npz, tools/make_golden_large.py) and at 512x512 bf16 B=8
    (config 4 per GPU); base@128 with 8 steps against the oracle and base@256 B=32 8 steps fp16 (config 3 per GPU)
  * training gradients at small@256 and at 192x192 with a ragged batch (config 5's network)
  * isolated SinusoidalPosEmb / time MLP and SqueezeExcitation KATs
  * the recompute-form kernels (irbx.hip) against the unfused pair and the oracle
  * in-place weight writes that bypass version counters, copy.deepcopy, out-of-range timesteps
  * the multi-rank bench.py path (two ranks rehearsed on the one GPU) and a plain run's headline-only line
"""
import copy
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import unet_ref
from oracle.weightgen import synth_tensor
from conftest import ROOT, max_abs, synth_input

pytestmark = pytest.mark.gpu
M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def psnr01(a, b):
    a = (torch.as_tensor(a).double().clamp(-1, 1) + 1) / 2
    b = (torch.as_tensor(b).double().clamp(-1, 1) + 1) / 2
    mse = ((a - b) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


_CACHE = {}


def model(variant, size, dev, **kw):
    key = (variant, size)
    if key not in _CACHE:
        unp = variant in ("tiny", "base")
        spec = oracle.make_spec(variant, size, allow_unpinned=unp)
        sd = oracle.synth_state_dict(oracle.param_shapes(spec))
        m = M.LowLightDiffusion(unet_variant=variant, image_size=size, num_inference_steps=4, allow_unpinned_groupnorm=unp)
        m.load_state_dict(sd)
        _CACHE[key] = (m.to(dev).eval(), sd, spec)
    return _CACHE[key]


def sampled(z):
    """The views tools/make_golden.py stored for the 256x256 run: stride-8 samples and the four 16x16 corners."""
    return {"_s8": z[:, :, ::8, ::8], "_c00": z[:, :, :16, :16], "_c11": z[:, :, -16:, -16:], "_c01": z[:, :, :16, -16:],
            "_c10": z[:, :, -16:, :16]}


# ------------------------------------------------------------------ config 2: reduced precision at the headline shape
@pytest.mark.parametrize("cd,min_psnr,max_rel", [("fp16", 42.0, 6e-3), ("bf16", 26.0, 5e-2)])
def test_small256_reduced_precision_vs_reference_golden(golden, dev, cd, min_psnr, max_rel):
    """The dtype the headline number is quoted in, at the headline image size, against outputs of the REFERENCE
    (B=1, CPU noise seed 123 in the reference's draw order).  fp16 / bf16 cannot meet 1e-3 (the reference's own autocast
    is 3.7e-3 / 3.3e-2 off), so: PSNR of the enhanced image on the stored samples, relative error of the
    first noise prediction, and then one row of a B=32 run must equal this B=1 run bit for bit."""
    g = golden("enhance_small256.npz")
    m, sd, spec = model("small", 256, dev)
    m.compute_dtype = cd
    try:
        low = synth_input("e2e256.low", (1, 3, 256, 256), -1.0, -0.4)
        torch.manual_seed(123)
        noise = torch.stack([torch.randn(1, 3, 256, 256) for _ in range(4)])
        out = m.enhance(low.to(dev), 4, noise=noise, return_intermediate=True, return_noise_pred=True)
        enh = out.enhanced.cpu()
        got = torch.cat([v.reshape(-1) for v in sampled(enh).values()])
        ref = torch.cat([torch.from_numpy(g["enhanced" + k]).reshape(-1) for k in sampled(enh)])
        p = psnr01(got, ref)
        np0 = out.noise_pred[0].cpu()
        rel = max(max_abs(v, g["noise_pred_0" + k]) for k, v in sampled(np0).items()) / float(g["noise_pred_0_mom"][2])
        print(f"small@256 {cd}: PSNR {p:.1f} dB on the reference's samples, first-forward rel err {rel:.2e}")
        assert p > min_psnr and rel < max_rel
        # the same image as row 5 of a 32-image batch (other rows: unrelated inputs)
        gen = torch.Generator().manual_seed(9)
        low32 = torch.rand(32, 3, 256, 256, generator=gen) * 2 - 1
        noise32 = torch.randn(4, 32, 3, 256, 256, generator=gen)
        low32[5], noise32[:, 5] = low[0], noise[:, 0]
        big = m.enhance(low32.to(dev), 4, noise=noise32.to(dev), return_intermediate=True)
        assert torch.equal(big.intermediate[-1][5:6], out.intermediate[-1])
    finally:
        m.compute_dtype = None


# ------------------------------------------------------------------ config 4: the `large` network
def test_large_variant_vs_reference_golden(golden, dev):
    """large@64: the reference's 4-step loop (all noise predictions and pre-clamp latents, fp32 <= 1e-3), bf16 by PSNR;
    large@128: one reference forward."""
    g = golden("large_kat.npz")
    m, sd, spec = model("large", 64, dev)
    low = synth_input("e2eL64.low", (1, 3, 64, 64), -1.0, -0.4)
    torch.manual_seed(int(g["seed"][0]))
    noise = torch.stack([torch.randn(1, 3, 64, 64) for _ in range(4)])
    m.compute_dtype = None
    out = m.enhance(low.to(dev), 4, noise=noise, return_intermediate=True, return_noise_pred=True)
    for i in range(4):
        assert max_abs(out.noise_pred[i].cpu(), g[f"noise_pred_{i}"]) < 1e-3
        assert max_abs(out.intermediate[i].cpu(), g[f"latents_{i}"]) < 1e-3
    assert max_abs(out.enhanced.cpu(), g["enhanced"]) < 1e-3
    m.compute_dtype = "bf16"
    try:
        o = m.enhance(low.to(dev), 4, noise=noise)
        p = psnr01(o.cpu(), g["enhanced"])
        print(f"large@64 bf16: PSNR {p:.1f} dB")
        assert p > 26.0
    finally:
        m.compute_dtype = None
    m128, _, _ = model("large", 128, dev)
    x = synth_input("large128.x", (1, 6, 128, 128), -1.5, 1.5).to(dev)
    y = m128.unet(x, torch.from_numpy(g["unet128_t"]).to(dev))
    assert max_abs(y.cpu(), g["unet128"]) < 1e-4 * max(1.0, np.abs(g["unet128"]).max())


def _properties(m, B, size, steps, cd, dev, sub):
    m.compute_dtype = cd
    try:
        gen = torch.Generator().manual_seed(77)
        low = (torch.rand(B, 3, size, size, generator=gen) * 2 - 1).to(dev)
        noise = torch.randn(steps, B, 3, size, size, generator=gen).to(dev)
        a = m.enhance(low, steps, noise=noise, return_intermediate=True)
        b = m.enhance(low, steps, noise=noise, return_intermediate=True)
        assert torch.equal(a.intermediate[-1], b.intermediate[-1])                      # bitwise reproducible
        assert torch.isfinite(a.intermediate[-1]).all()
        assert a.enhanced.min() >= -1 and a.enhanced.max() <= 1
        assert torch.equal(a.enhanced, a.intermediate[-1].clamp(-1, 1))
        s0, s1 = sub
        c = m.enhance(low[s0:s1], steps, noise=noise[:, s0:s1], return_intermediate=True)  # ragged sub-batch
        assert torch.equal(c.intermediate[-1], a.intermediate[-1][s0:s1])               # rows independent of batch mates
    finally:
        m.compute_dtype = None


def test_full_size_properties_large512_b8_bf16(dev):
    """BASELINE config 4's per-GPU shape (large, 512x512, 8 images per GPU, 4 steps, bf16)."""
    m, sd, spec = model("large", 512, dev)
    _properties(m, 8, 512, 4, "bf16", dev, (2, 5))
    del _CACHE[("large", 512)]
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ config 3: `base`, 8 steps (parity unpinned: no reference)
def test_base128_eight_steps_fp16_vs_oracle(dev):
    """`base` cannot be constructed by the reference (GroupNorm(32, 48)); the engine and the oracle share the documented
    deviation (groups = largest divisor <= 32).  Engine vs oracle only: fp32 <= 1e-3, fp16 by PSNR, 8 LCM steps."""
    m, sd, spec = model("base", 128, dev)
    gen = torch.Generator().manual_seed(3)
    low = torch.rand(1, 3, 128, 128, generator=gen) * 2 - 1
    noise = oracle.draw_noise(1, 128, 8, seed=31)
    ref = oracle.enhance_ref(sd, spec, low, 8, noise)
    m.compute_dtype = None
    out = m.enhance(low.to(dev), 8, noise=torch.stack(noise), return_intermediate=True)
    assert max(max_abs(a.cpu(), b) for a, b in zip(out.intermediate, ref["intermediate"])) < 1e-3
    m.compute_dtype = "fp16"
    try:
        o = m.enhance(low.to(dev), 8, noise=torch.stack(noise))
        p = psnr01(o.cpu(), ref["enhanced"])
        print(f"base@128 8 steps fp16: PSNR {p:.1f} dB vs oracle")
        assert p > 40.0
    finally:
        m.compute_dtype = None


@pytest.mark.parametrize("size,batch", [(96, 3), (160, 1), (224, 1), (72, 2), (104, 1), (200, 1)])
def test_image_sizes_that_are_not_multiples_of_64(dev, size, batch):
    """The reference builds any image_size its three stride-2 convolutions accept (efficient_unet.py:403-530, CLI
    `--image_size`, scripts/inference.py:30-62).  The engine takes every multiple of 8 from 64 on, like the reference: the lower levels'
    maps (12 x 12, 20 x 20, 28 x 28; 36 / 18 / 9, 52 / 26 / 13, 100 / 50 / 25) leave the GEMM / depthwise / 3x3 conv /
    attention / input- and output-conv tiles partly empty.  fp32 engine vs oracle <= 1e-3
    on the pre-clamp latents, fp16 by PSNR, sub-batch rows bit-equal."""
    m, sd, spec = model("small", size, dev)
    gen = torch.Generator().manual_seed(size)
    low = torch.rand(batch, 3, size, size, generator=gen) * 2 - 1
    noise = oracle.draw_noise(batch, size, 4, seed=size + 1)
    ref = oracle.enhance_ref(sd, spec, low, 4, noise)
    m.compute_dtype = None
    out = m.enhance(low.to(dev), 4, noise=torch.stack(noise), return_intermediate=True)
    err = max(max_abs(a.cpu(), b) for a, b in zip(out.intermediate, ref["intermediate"]))
    print(f"small@{size} B={batch} fp32: max-abs latent error {err:.2e}")
    assert err < 1e-3
    m.compute_dtype = "fp16"
    try:
        nz = torch.stack(noise).to(dev)
        o = m.enhance(low.to(dev), 4, noise=nz, return_intermediate=True)
        p = psnr01(o.enhanced.cpu(), ref["enhanced"])
        print(f"small@{size} fp16: PSNR {p:.1f} dB vs oracle")
        assert p > 40.0
        one = m.enhance(low[:1].to(dev), 4, noise=nz[:, :1], return_intermediate=True)
        assert torch.equal(o.intermediate[-1][:1], one.intermediate[-1])
    finally:
        m.compute_dtype = None


@pytest.mark.parametrize("variant,size", [("large", 96), ("base", 72)])
def test_ragged_sizes_other_variants(dev, variant, size):
    """The same at other topologies: `large` (wider channels) and the opt-in zero-padded `base` (pool-slab SE path)."""
    m, sd, spec = model(variant, size, dev)
    low = torch.rand(2, 3, size, size, generator=torch.Generator().manual_seed(size)) * 2 - 1
    noise = oracle.draw_noise(2, size, 4, seed=size + 7)
    ref = oracle.enhance_ref(sd, spec, low, 4, noise)
    m.compute_dtype = None
    out = m.enhance(low.to(dev), 4, noise=torch.stack(noise), return_intermediate=True)
    assert max(max_abs(a.cpu(), b) for a, b in zip(out.intermediate, ref["intermediate"])) < 1e-3


def test_unsupported_image_sizes_are_refused(dev):
    for size in (100, 60, 32):
        with pytest.raises(ValueError):
            mm = M.LowLightDiffusion(unet_variant="small", image_size=size).to(dev)
            mm.enhance(torch.zeros(1, 3, size, size, device=dev), 4)


def test_full_size_properties_base256_b32_n8_fp16(dev):
    """BASELINE config 3's per-GPU shape (base, 256x256, 32 images per GPU, 8 steps, fp16)."""
    m, sd, spec = model("base", 256, dev)
    _properties(m, 32, 256, 8, "fp16", dev, (11, 14))
    del _CACHE[("base", 256)]
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ config 5: training gradients at the real image size
def _grad_check(variant, size, B, dev, loss, max_l2, min_cos):
    from test_gpu_training import _ref_unet_grads, cosine
    m, sd, spec = model(variant, size, dev)
    m.compute_dtype = None
    m.train()
    try:
        gen = torch.Generator().manual_seed(size + B)
        low = torch.rand(B, 3, size, size, generator=gen) * 2 - 1
        normal = torch.rand(B, 3, size, size, generator=gen) * 2 - 1
        noise = torch.randn(B, 3, size, size, generator=gen)
        t = torch.randint(0, 1000, (B,), generator=gen)
        loss_ref, pred_ref, gref = _ref_unet_grads(sd, spec, low, normal, t, noise, loss=loss)
        m.zero_grad(set_to_none=True)
        out = m(low.to(dev), normal.to(dev), timesteps=t.to(dev), noise=noise.to(dev))
        lv = {"mse": torch.nn.functional.mse_loss, "l1": torch.nn.functional.l1_loss}[loss](out["noise_pred"], out["noise"])
        lv.backward()
        assert abs(lv.item() - loss_ref.item()) < 1e-5 * max(1.0, abs(loss_ref.item()))
        assert (out["noise_pred"].detach().cpu() - pred_ref).abs().max() < 1e-3
        bad, l2s = {}, []
        for k, p in m.named_parameters():
            a, b = p.grad.double().cpu(), gref[k].double()
            l2, cs = ((a - b).norm() / b.norm().clamp_min(1e-30)).item(), cosine(a, b)
            l2s.append(l2)
            if not (l2 < max_l2 and cs > min_cos):
                bad[k] = (l2, cs)
        print(f"{variant}@{size} B={B} gradients vs CPU autograd: median rel L2 {sorted(l2s)[len(l2s) // 2]:.2e}, worst {max(l2s):.2e}")
        assert not bad, f"{len(bad)} tensors off: {dict(list(bad.items())[:8])}"
    finally:
        m.zero_grad(set_to_none=True)
        m.eval()


def test_unet_backward_small256(dev):
    """All 321 parameter gradients of the network BASELINE config 5 trains, at its image size (B=1), vs CPU autograd."""
    _grad_check("small", 256, 1, dev, "mse", 2e-2, 0.9995)


def test_unet_backward_192_ragged_batch(dev):
    """192x192 (levels 192/96/48/24: none a power of two) with a batch of 3."""
    _grad_check("small", 192, 3, dev, "l1", 2e-2, 0.9995)


# ------------------------------------------------------------------ rows a5 / a7 on their own
def test_sinusoidal_embedding_and_time_mlp_kat(golden, dev):
    """SinusoidalPosEmb(32) against the reference's vectors ([cos | sin], t in {19, 739, 0, 999}); time_mlp against the
    oracle (efficient_unet.py:60-76, 412-417)."""
    g = golden("ops_kat.npz")
    m, sd, spec = model("small", 64, dev)
    t = torch.from_numpy(g["sinemb32_t"])
    emb, temb = m.unet.time_embedding(t.to(dev))
    assert emb.shape == (4, 32)
    assert max_abs(emb.cpu(), g["sinemb32"]) < 2e-6          # cosf / sinf of arguments up to 999
    e = torch.from_numpy(g["sinemb32"])
    h = torch.nn.functional.silu(e @ sd["unet.time_mlp.1.weight"].T + sd["unet.time_mlp.1.bias"])
    ref = h @ sd["unet.time_mlp.3.weight"].T + sd["unet.time_mlp.3.bias"]
    assert max_abs(temb.cpu(), ref) < 1e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("cd,tol", [(None, 1e-5), ("fp16", 4e-3)])
def test_squeeze_excitation_kat(golden, dev, cd, tol):
    """SqueezeExcitation(128) on the reference's vector (pool -> fc1 -> ReLU6 -> fc2 -> sigmoid -> x * s, :96-100)
    through the engine's own SE kernels (se_pool / se_fc1 / se_fc2)."""
    g = golden("ops_kat.npz")
    se = M.SqueezeExcitation(128)
    se.load_state_dict({k: synth_tensor("se128." + k, tuple(v.shape)) for k, v in se.state_dict().items()})
    se = se.to(dev)
    se.compute_dtype = cd
    with torch.no_grad():
        y = se(synth_input("se128.x", (2, 128, 8, 8), -2, 2).to(dev))
    assert max_abs(y.cpu(), g["se128"]) < tol * max(1.0, np.abs(g["se128"]).max())


# ------------------------------------------------------------------ recompute form (irbx.hip) vs unfused pair vs oracle
@pytest.mark.parametrize("cd,cap", [("fp16", 1.5e-3), ("bf16", 1.2e-2)])
@pytest.mark.parametrize("cin,cout,hw,b,split", [(32, 32, 16, 2, 0), (32, 64, 32, 3, 0), (64, 64, 32, 2, 0), (96, 32, 64, 2, 64),
                                                 (32, 32, 128, 1, 0)])
def test_recompute_block_front_vs_unfused_and_oracle(dev, cd, cap, cin, cout, hw, b, split):
    """expand_stats + expand_dw (h1 never stored) against the pw_gemm -> dwconv3x3 pair and against the CPU oracle:
    the fused form must be at least as close to the oracle as the unfused one (it rounds h1 once less)."""
    name = f"xi_{cin}_{cout}_{hw}"
    blk = M.InvertedResidualBlock(cin, cout, 128, concat_split=split)
    blk.load_state_dict({k: synth_tensor(name + "." + k, tuple(v.shape)) for k, v in blk.state_dict().items()})
    blk = blk.to(dev)
    blk.compute_dtype = cd
    sd = {name + "." + k: v.detach().cpu() for k, v in blk.state_dict().items()}
    x = synth_input(name + ".x", (b, cin, hw, hw), -2, 2)
    te = synth_input(name + ".temb", (b, 128), -1, 1)
    ref = unet_ref.irb_forward(sd, name, x, te)
    ys = []
    try:
        for v in (0, 1):
            N.check(N.lib().llie_tune(b"irbx", v))
            with torch.no_grad():
                ys.append(blk(x.to(dev), te.to(dev)).cpu())
    finally:
        N.check(N.lib().llie_tune(b"irbx", 1))
    r0 = ((ys[0] - ref).norm() / ref.norm()).item()
    r1 = ((ys[1] - ref).norm() / ref.norm()).item()
    assert not torch.equal(ys[0], ys[1])          # the two paths really are different kernels
    assert r1 < cap and r1 < 1.15 * r0 + 1e-5, (r0, r1)


def test_recompute_form_whole_network_properties(dev):
    """small@256 fp16 with the recompute form on (default) and off: close to each other, each bitwise reproducible, and
    the recompute form keeps sub-batches bit-identical (fixed per-tile partial sums, no atomics)."""
    m, sd, spec = model("small", 256, dev)
    m.compute_dtype = "fp16"
    try:
        gen = torch.Generator().manual_seed(4)
        low = (torch.rand(3, 3, 256, 256, generator=gen) * 2 - 1).to(dev)
        noise = torch.randn(4, 3, 3, 256, 256, generator=gen).to(dev)
        outs = []
        for v in (0, 1, 1):
            N.check(N.lib().llie_tune(b"irbx", v))
            o = m.enhance(low, 4, noise=noise, return_intermediate=True, return_noise_pred=True)
            outs.append((o.noise_pred[0].clone(), o.intermediate[-1].clone(), o.enhanced.clone()))
        rel = max_abs(outs[0][0].cpu(), outs[1][0].cpu()) / outs[0][0].abs().max().item()
        assert rel < 5e-3, rel
        assert psnr01(outs[0][2].cpu(), outs[1][2].cpu()) > 45.0
        assert torch.equal(outs[1][1], outs[2][1])
        one = m.enhance(low[1:2], 4, noise=noise[:, 1:2], return_intermediate=True).intermediate[-1]
        assert torch.equal(outs[1][1][1:2], one)
    finally:
        N.check(N.lib().llie_tune(b"irbx", 1))
        m.compute_dtype = None


def test_recompute_form_is_race_free_under_concurrency(dev):
    """Two engines run `enhance` on two streams at once (what the two half-batch graph branches do): every result must
    equal the solo result bit for bit, for the double- and the single-buffered depthwise stage.  This is the screen that
    caught a pool partial read before its LDS write had landed (common.h wg_barrier)."""
    import ctypes as C
    L = N.lib()
    B = 8
    spec = oracle.make_spec("small", 256)
    sd = oracle.synth_state_dict(oracle.param_shapes(spec))
    ms = []
    for _ in range(2):
        m = M.LowLightDiffusion(unet_variant="small", image_size=256, compute_dtype="fp16")
        m.load_state_dict(sd)
        ms.append(m.to(dev).eval())
    g = torch.Generator().manual_seed(1)
    ins = [((torch.rand(B, 3, 256, 256, generator=g) * 2 - 1).to(dev), torch.randn(4, B, 3, 256, 256, generator=g).to(dev)) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        for dbuf in (1, 0):
            N.check(L.llie_tune(b"irbx_dbuf", dbuf))
            solo = [m.enhance(x, 4, noise=nz, return_intermediate=True).intermediate[-1].clone() for m, (x, nz) in zip(ms, ins)]
            torch.cuda.synchronize()
            for _ in range(4):
                outs = []
                for m, (x, nz), st in zip(ms, ins, streams):
                    st.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(st):
                        outs.append(m.enhance(x, 4, noise=nz, return_intermediate=True).intermediate[-1])
                torch.cuda.synchronize()
                for o, s0 in zip(outs, solo):
                    assert torch.equal(o, s0), f"dbuf={dbuf}"
    finally:
        N.check(L.llie_tune(b"irbx_dbuf", 0))


def test_copy_probe_copies(dev):
    """bench.py's bandwidth probe is a real copy (ragged sizes included)."""
    for n16 in (1, 255, 1024, 4099, 256 * 8 * 1024 + 17):
        src = torch.randint(-2**31, 2**31 - 1, (n16 * 4,), dtype=torch.int32, device=dev)
        dst = torch.zeros_like(src)
        N.check(N.lib().llie_copy_probe(src.data_ptr(), dst.data_ptr(), n16 * 16, torch.cuda.current_stream().cuda_stream))
        assert torch.equal(src, dst)


# ------------------------------------------------------------------ weights changed behind PyTorch's back
def test_inplace_data_writes_are_noticed(dev):
    """`p.data.copy_(...)` leaves `_version` and `data_ptr()` unchanged -- the reference's EMA swaps weights exactly this way
    (trainer.py:104-117 apply_shadow / restore; low_light_diffusion.py:317-323 update_ema).  The engine's on-device content
    hash must notice: after the write the model has to behave like a fresh model built from the new weights."""
    spec = oracle.make_spec("small", 64)
    sd_a = oracle.synth_state_dict(oracle.param_shapes(spec))
    sd_b = {k: synth_tensor("other:" + k, tuple(v.shape)) for k, v in sd_a.items()}
    low = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    noise = torch.stack(oracle.draw_noise(2, 64, 4, seed=2)).to(dev)
    for cd in (None, "fp16"):
        m = M.LowLightDiffusion(unet_variant="small", image_size=64, compute_dtype=cd)
        m.load_state_dict(sd_a)
        m = m.to(dev).eval()
        ya = m.enhance(low, 4, noise=noise)
        versions = [p._version for p in m.parameters()]
        backup = {k: p.data.clone() for k, p in m.named_parameters()}
        for k, p in m.named_parameters():            # EMAModel.apply_shadow
            p.data.copy_(sd_b[k].to(dev))
        assert versions == [p._version for p in m.parameters()]     # PyTorch saw nothing
        yb = m.enhance(low, 4, noise=noise)
        fresh = M.LowLightDiffusion(unet_variant="small", image_size=64, compute_dtype=cd)
        fresh.load_state_dict(sd_b)
        yb_ref = fresh.to(dev).eval().enhance(low, 4, noise=noise)
        assert torch.equal(yb, yb_ref) and not torch.equal(yb, ya)
        for k, p in m.named_parameters():            # EMAModel.restore
            p.data.copy_(backup[k])
        assert torch.equal(m.enhance(low, 4, noise=noise), ya)
        # the single-forward entry point takes the same route
        t = torch.tensor([500, 37], device=dev)
        x = torch.cat([noise[0], low], 1)
        e1 = m.unet(x, t)
        for p in m.parameters():
            p.data.mul_(1.01)
        assert not torch.equal(m.unet(x, t), e1)


def test_deepcopy_after_first_forward(dev):
    """copy.deepcopy(model) is how the reference builds EMA / target networks (low_light_diffusion.py:312,
    lcm_scheduler.py:353); it must work once the model owns an engine handle, and the copy must be independent."""
    m, sd, spec = model("small", 64, dev)
    low = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(dev)
    noise = torch.stack(oracle.draw_noise(1, 64, 4, seed=5)).to(dev)
    y = m.enhance(low, 4, noise=noise)
    c = copy.deepcopy(m)
    assert torch.equal(c.enhance(low, 4, noise=noise), y)
    with torch.no_grad():
        for p in c.parameters():
            p.mul_(0.5)
    assert not torch.equal(c.enhance(low, 4, noise=noise), y)
    assert torch.equal(m.enhance(low, 4, noise=noise), y)        # the original is untouched


def test_out_of_range_timesteps(dev):
    """The reference indexes alphas_cumprod with the timesteps (lcm_scheduler.py:268): out of range raises.  Host-side
    timesteps raise IndexError here too; device-side ones cannot (asynchronous): the kernel refuses to index and the
    affected sample comes out NaN instead of reading past the table."""
    sch = M.LCMScheduler()
    x = torch.rand(2, 3, 8, 8, device=dev)
    nz = torch.randn(2, 3, 8, 8, device=dev)
    for bad in ([0, 1000], [5, -1001]):
        with pytest.raises(IndexError):
            sch.add_noise(x, nz, torch.tensor(bad))
    out = sch.add_noise(x, nz, torch.tensor([7, 1000], device=dev))
    assert torch.isfinite(out[0]).all() and torch.isnan(out[1]).all()
    ok = sch.add_noise(x, nz, torch.tensor([7, -1]))                 # negative index wraps like tensor indexing
    ref = sch.add_noise(x, nz, torch.tensor([7, 999], device=dev))
    assert torch.equal(ok, ref)
    v = sch.get_velocity(x, nz, torch.tensor([0, 999], device=dev))
    assert torch.isfinite(v).all()


# ------------------------------------------------------------------ the multi-rank bench path
def _bench(args, world):
    env = dict(os.environ, LLIE_BENCH_REHEARSAL="1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", "29731", os.path.join(ROOT, "bench.py"), "--gpus", str(world)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_inference(tmp_path):
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one rank per process, barrier + max over ranks,
    async all_gather of the outputs), rehearsed with both ranks on this box's one GPU over gloo."""
    line = _bench(["--steps", "2", "--warmup", "1", "--batch", "4", "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)], 2)
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 8 and line["scaling"] == "weak"
    assert line["value"] > 0 and line["steps"] == 2 and line["unit"] == "images/sec"
    assert abs(line["value"] - 8 * 2 / (line["ms_per_step"] * 2e-3)) / line["value"] < 1e-2
    assert line["roofline"]["frac"] > 0 and line["roofline"]["whole_path"]["frac"] > 0
    # --dump-outputs: the gathered batch of the last timed step, both ranks' shards
    enh = np.load(tmp_path / "enhanced.npy")
    assert enh.dtype == np.float32 and enh.shape == (8, 3, 256, 256)
    assert np.isfinite(enh).all() and np.abs(enh).max() <= 1.0 and not np.array_equal(enh[:4], enh[4:])


def test_bench_plain_run_is_the_headline_only(tmp_path):
    """Without --full, bench.py sets up, warms up, times, dumps and prints the headline line: no roofline passes, copy
    probe or CPU baseline after the timed region."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "fp16" and line["n_gpus"] == 1
    assert line["value"] > 0 and abs(line["value"] - 4 * 2 / (line["ms_per_step"] * 2e-3)) / line["value"] < 1e-2
    assert not {"roofline", "cpu_baseline", "quality"} & line.keys()
    enh = np.load(tmp_path / "enhanced.npy")
    assert enh.dtype == np.float32 and enh.shape == (4, 3, 256, 256) and np.isfinite(enh).all()


def test_bench_two_ranks_training():
    line = _bench(["--train", "--steps", "2", "--warmup", "1", "--batch", "2", "--dtype", "bf16", "--no-cpu-baseline"], 2)
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 4
    assert line["value"] > 0 and math.isfinite(line["final_loss"])
