"""Everything the engine decides on the host, as text: parameter table, gradient offsets, workspace plans, byte / flop models.
Needs no GPU.  Usage: python plan_dump.py REPO_ROOT [knob=value ...] > out.txt   (knobs go to llie_tune first)"""
import importlib
import sys

root = sys.argv[1]
sys.path.insert(0, root)
M = importlib.import_module("cv-diffusion-model_amd")
N = importlib.import_module("cv-diffusion-model_amd._native")
U = importlib.import_module("cv-diffusion-model_amd.unet")

DT = (N.LLIE_F32, N.LLIE_F16, N.LLIE_BF16)
for kv in sys.argv[2:]:
    k, v = kv.split("=")
    assert N.lib().llie_tune(k.encode(), int(v)) == 0, kv


def row(*a):
    print("\t".join(str(x) for x in a))


def safe(f, *a):
    try:
        return f(*a)
    except Exception as e:  # refusals are part of the behaviour
        return "ERR:" + type(e).__name__ + ":" + str(e)[:80]


for variant, sizes, kw in (("small", (64, 72, 128, 200, 256), {}), ("large", (64, 72, 256, 512), {}),
                           ("tiny", (64, 128), {"allow_unpinned_groupnorm": True}),
                           ("base", (64, 128, 256), {"allow_unpinned_groupnorm": True})):
    for size in sizes:
        m = M.LowLightDiffusion(unet_variant=variant, image_size=size, **kw)
        for dt in DT:
            h = N.Handle(m.unet._make_cfg(dt))
            tag = f"{variant}@{size}/dt{dt}"
            if dt == N.LLIE_F32 and size == sizes[0]:
                for (k, shp), off in zip(h.params(), h.grad_offsets()):
                    row("param", tag, k, shp, off)
            row("grad_numel", tag, h.grad_numel())
            for b in (1, 2, 3, 8, 15, 16, 32):
                row("plan", tag, b, safe(h.workspace_bytes, b), safe(h.enhance_workspace_bytes, b, 4),
                    safe(h.train_workspace_bytes, b), safe(h.algorithmic_bytes, b), safe(h.path_bytes, b), safe(h.flops, b))
            h.close()

mods = [("irb", U._module_cfg(N.LLIE_IRB, 64, 64, 256)), ("irb_skip", U._module_cfg(N.LLIE_IRB, 64, 128, 256)),
        ("irb_cat", U._module_cfg(N.LLIE_IRB, 192, 64, 256, split=128)), ("irb_wide", U._module_cfg(N.LLIE_IRB, 256, 256, 256)),
        ("attn", U._module_cfg(N.LLIE_ATTN, 128, 128)), ("down", U._module_cfg(N.LLIE_DOWN, 64, 64)),
        ("up", U._module_cfg(N.LLIE_UP, 64, 64)), ("se", U._module_cfg(N.LLIE_SE, 256, 256))]
for name, cfg in mods:
    for dt in DT:
        cfg.compute_dtype = dt
        h = N.Handle(cfg)
        for (k, shp), off in zip(h.params(), h.grad_offsets()):
            row("mparam", name, dt, k, shp, off)
        for hw in (8, 16, 32, 64, 128, 256):
            for b in (1, 4):
                row("mplan", name, dt, hw, b, safe(h.workspace_bytes, b, hw, hw), safe(h.train_workspace_bytes, b, hw, hw))
        h.close()
