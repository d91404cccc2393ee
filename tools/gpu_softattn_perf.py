#!/usr/bin/env python3
"""Softmax attention on the MI355X (argv: rounds, default 5).  Prints one JSON line with

  kernels   per (N, B) in (1024, 32), (4096, 32), (32400, 1), heads = 4, fp16 and bf16: device-event milliseconds (medians of
            `rounds` windows, every shape warmed up first) of llie_softattn (with lse) and llie_softattn_backward alone; the forward's
            achieved TFLOP/s by the 4 N^2 inner flop model (the backward: 10 N^2 inner, its five products) and that as a share of
            the 2.5 PFLOP/s dense MFMA peak; on the same tensors torch.nn.functional.scaled_dot_product_attention and the unfused
            three-op restatement softmax(q k^T scale) v (forward; N = 32400 unfused is skipped: its N x N matrix is 8.4 GB per
            head at fp32 accumulate and the comparison is about the shapes the network runs); and the two pass / fail comparisons'
            first: fused_not_slower_than_unfused at N >= 1024
  models    small@256, 4 steps: enhance at B = 32, fp16, and TrainStep at B = 8, bf16, with softmax against linear attention in
            the same run, alternating; the difference per call next to the kernel-alone time of the attention sites (the second
            comparison: the whole-model difference must not exceed what the kernels alone explain by more than the to_out / norm
            launches the linear form does not save either)
"""
import importlib
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda:0")
PEAK_TF = 2500.0
HEADS, INNER = 4, 128
L = N.lib()


def time_ms(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def med(fn, n):
    return statistics.median(time_ms(fn, n) for _ in range(rounds))


res = {"rounds": rounds, "heads": HEADS, "peak_tflops": PEAK_TF, "kernels": [], "models": {}}
for n, b in ((1024, 32), (4096, 32), (32400, 1)):
    for name, code, tdt in (("fp16", 1, torch.float16), ("bf16", 2, torch.bfloat16)):
        g = torch.Generator(device=dev).manual_seed(n + code)
        qkv = (torch.randn(b, n, 3 * INNER, device=dev, generator=g) * 0.8).to(tdt)
        dout = torch.randn(b, n, INNER, device=dev, generator=g).to(tdt)
        out, dqkv = torch.empty(b, n, INNER, device=dev, dtype=tdt), torch.empty_like(qkv)
        lse, scr = torch.empty(b, HEADS, n, device=dev), torch.empty(b * HEADS * n, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        iters = max(3, min(200, int(1e12 / (b * n * n * INNER))))

        def fwd():
            N.check(L.llie_softattn(code, qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), b, n, HEADS, st), "softattn")

        def bwd():
            N.check(L.llie_softattn_backward(code, qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                             scr.data_ptr(), scr.numel(), b, n, HEADS, st), "softattn_backward")

        q, k, v = (z.view(b, n, HEADS, 32).transpose(1, 2) for z in qkv.split(INNER, dim=2))  # [b][heads][n][32] views of the same tensor
        f_ms, b_ms = med(fwd, iters), med(bwd, iters)
        sdpa_ms = med(lambda: F.scaled_dot_product_attention(q, k, v), iters)
        unf_ms = None
        if n <= 4096:
            unf_ms = med(lambda: torch.softmax(q @ k.transpose(-1, -2) * (32.0 ** -0.5), -1) @ v, max(3, iters // 4))
        flops = 4.0 * b * n * n * INNER
        row = {"N": n, "B": b, "dtype": name, "iters": iters, "fwd_ms": round(f_ms, 4), "bwd_ms": round(b_ms, 4),
               "fwd_tflops": round(flops / f_ms / 1e9, 1), "fwd_share_of_peak": round(flops / f_ms / 1e9 / PEAK_TF, 4),
               "bwd_tflops": round(2.5 * flops / b_ms / 1e9, 1), "bwd_share_of_peak": round(2.5 * flops / b_ms / 1e9 / PEAK_TF, 4),
               "sdpa_fwd_ms": round(sdpa_ms, 4), "fused_over_sdpa": round(f_ms / sdpa_ms, 3),
               "unfused_fwd_ms": None if unf_ms is None else round(unf_ms, 4),
               "fused_not_slower_than_unfused": None if unf_ms is None else bool(f_ms <= unf_ms)}
        res["kernels"].append(row)
        del qkv, dout, out, dqkv, lse, scr, q, k, v
        torch.cuda.empty_cache()


def build(softmax):
    torch.manual_seed(0)
    unet = M.create_efficient_unet("small", 256, in_channels=6, use_linear_attention=not softmax)
    return M.LowLightDiffusion(unet=unet, image_size=256, num_inference_steps=4).to(dev)


# whole model: enhance, B = 32, fp16
models = {"linear": build(False).eval(), "softmax": build(True).eval()}
low = torch.rand(32, 3, 256, 256, device=dev) * 2 - 1
noise = torch.randn(4, 32, 3, 256, 256, device=dev)
enh = {k: [] for k in models}
for m in models.values():
    m.compute_dtype = "fp16"
for _ in range(rounds):  # alternate, so that drift on a shared host hits both
    for k, m in models.items():
        enh[k].append(time_ms(lambda: m.enhance(low, 4, noise=noise), 10))
e = {k: statistics.median(v) for k, v in enh.items()}
# attention sites of small@256: N = 256 (C = 128; two encoder, three decoder) and N = 1024 (C = 256; two encoder, mid, three decoder)
res["models"]["enhance_b32_fp16"] = {"linear_ms": round(e["linear"], 3), "softmax_ms": round(e["softmax"], 3),
                                     "difference_ms": round(e["softmax"] - e["linear"], 3),
                                     "linear_ms_rounds": [round(v, 3) for v in enh["linear"]], "softmax_ms_rounds": [round(v, 3) for v in enh["softmax"]]}
# the core alone at the network's own sites, B = 32, fp16, per 4-step call
core = 0.0
for n, sites in ((256, 5), (1024, 6)):
    qkv = (torch.randn(32, n, 3 * INNER, device=dev) * 0.8).half()
    out = torch.empty(32, n, INNER, device=dev, dtype=torch.float16)
    st = torch.cuda.current_stream(dev).cuda_stream
    core += 4 * sites * med(lambda: N.check(L.llie_softattn(1, qkv.data_ptr(), out.data_ptr(), None, 32, n, HEADS, st), "softattn"), 50)
res["models"]["enhance_b32_fp16"]["softattn_kernels_alone_ms"] = round(core, 3)
del low, noise

# whole model: TrainStep, B = 8, bf16
steps = {}
for k, m in models.items():
    m.train()
    m.compute_dtype = "bf16"
    steps[k] = M.TrainStep(m, M.FusedAdamW(m.parameters(), lr=1e-6, weight_decay=0.01, max_grad_norm=1.0))
kw = dict(low_light=torch.rand(8, 3, 256, 256, device=dev) * 2 - 1, normal_light=torch.rand(8, 3, 256, 256, device=dev) * 2 - 1,
          timesteps=torch.randint(0, 1000, (8,), device=dev), noise=torch.randn(8, 3, 256, 256, device=dev))
tr = {k: [] for k in models}
for _ in range(rounds):
    for k in models:
        tr[k].append(time_ms(lambda: steps[k](**kw), 8))
t = {k: statistics.median(v) for k, v in tr.items()}
res["models"]["train_step_b8_bf16"] = {"linear_ms": round(t["linear"], 3), "softmax_ms": round(t["softmax"], 3),
                                       "difference_ms": round(t["softmax"] - t["linear"], 3),
                                       "linear_ms_rounds": [round(v, 3) for v in tr["linear"]], "softmax_ms_rounds": [round(v, 3) for v in tr["softmax"]]}
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
