"""Device-resident data loader, the parts that need no GPU: the epoch plan, the NumPy twins of the two augmentation kernels
against a float64 restatement of their definition written here and against the reference's synthetic low-light bytes, the frame
store on PNG folders, and the argument checks of the C ABI."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

M = importlib.import_module("cv-diffusion-model_amd")
D = importlib.import_module("cv-diffusion-model_amd.data")
native = importlib.import_module("cv-diffusion-model_amd._native")

HFLIP, VFLIP, ROTATE = 1, 2, 4


def noise_frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(n)]


def one_row(low=0, high=1, y0=0, x0=0, flags=0, angle_deg=0.0, gamma=1.0, level=0.0, scale=(1.0, 1.0, 1.0)):
    row = np.zeros(1, dtype=D.PLAN_DTYPE)
    row["low_frame"], row["high_frame"], row["y0"], row["x0"], row["flags"] = low, high, y0, x0, flags
    row["ca"], row["sa"] = np.float32(math.cos(math.radians(angle_deg))), np.float32(math.sin(math.radians(angle_deg)))
    row["gamma"], row["level"], row["scale"] = gamma, level, scale
    return row


# ------------------------------------------------------------------ 1. the plan
def mixed_sizes(n, s, seed=0):
    rng = np.random.default_rng(seed)
    sizes = [(int(s + rng.integers(0, 90)), int(s + rng.integers(0, 140))) for _ in range(n)]
    sizes[0], sizes[1], sizes[2] = (s, s), (s, s + 7), (s + 5, s)  # no room at all, along one axis, along the other
    return sizes


@pytest.mark.parametrize("mode", ["train", "synthetic"])
def test_plan_crops_inside_and_reproducible(mode):
    s, n = 64, 203
    sizes = mixed_sizes(n, s)
    a = M.epoch_plan(sizes, s, mode, seed=3, epoch=5, batch_size=8)
    assert a.dtype == D.PLAN_DTYPE and len(a) == (n // 8) * 8
    hw = np.array(sizes)[a["low_frame"]]
    assert (a["y0"] >= 0).all() and (a["x0"] >= 0).all()
    assert (a["y0"] + s <= hw[:, 0]).all() and (a["x0"] + s <= hw[:, 1]).all()
    for i in (0, 1, 2):  # the frames without room are pinned to origin 0 along that axis
        sel = a["low_frame"] == i
        if sizes[i][0] == s:
            assert (a["y0"][sel] == 0).all()
        if sizes[i][1] == s:
            assert (a["x0"][sel] == 0).all()
    assert len(np.unique(a["low_frame"])) == len(a)  # a permutation: no pair twice
    assert np.array_equal(a["high_frame"], a["low_frame"] + (n if mode == "train" else 0))
    b = M.epoch_plan(sizes, s, mode, seed=3, epoch=5, batch_size=8)
    assert a.tobytes() == b.tobytes()
    c = M.epoch_plan(sizes, s, mode, seed=3, epoch=6, batch_size=8)
    assert not np.array_equal(a["low_frame"], c["low_frame"]) and a.tobytes() != c.tobytes()
    d = M.epoch_plan(sizes, s, mode, seed=4, epoch=5, batch_size=8)
    assert a.tobytes() != d.tobytes()


def within_5_sigma(count, n, p):
    return abs(count / n - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n)


def test_plan_distributions():
    """20 000 draws per mode: flag frequencies within 5 binomial sigma of the reference's probabilities, every value in its range,
    and both ends of every range approached."""
    s, n = 32, 20000
    sizes = mixed_sizes(n, s, seed=1)
    t = M.epoch_plan(sizes, s, "train", seed=0, epoch=0, batch_size=8)
    assert len(t) == n
    assert within_5_sigma(int((t["flags"] & HFLIP > 0).sum()), n, 0.5)
    assert within_5_sigma(int((t["flags"] & VFLIP > 0).sum()), n, 0.3)
    assert within_5_sigma(int((t["flags"] & ROTATE > 0).sum()), n, 0.3)
    rot = t["flags"] & ROTATE > 0
    ang = np.degrees(np.arctan2(t["sa"].astype(np.float64), t["ca"].astype(np.float64)))
    assert np.abs(ang).max() <= 15.0 + 1e-4 and ang[rot].min() < -14.5 and ang[rot].max() > 14.5
    assert np.allclose(t["ca"].astype(np.float64) ** 2 + t["sa"].astype(np.float64) ** 2, 1.0, atol=1e-6)
    assert (t["ca"][~rot] == 1.0).all() and (t["sa"][~rot] == 0.0).all()
    assert (t["scale"] == 1.0).all()
    # the origin is uniform over its whole range: both ends occur for a frame with room
    hw = np.array(sizes)[t["low_frame"]]
    assert ((t["y0"] == 0) & (hw[:, 0] > s)).any() and ((t["y0"] == hw[:, 0] - s) & (hw[:, 0] > s)).any()
    assert ((t["x0"] == 0) & (hw[:, 1] > s)).any() and ((t["x0"] == hw[:, 1] - s) & (hw[:, 1] > s)).any()

    y = M.epoch_plan(sizes, s, "synthetic", seed=0, epoch=0, batch_size=8, gamma_range=(2.0, 5.0), noise_level_range=(0.01, 0.05))
    assert len(y) == n
    assert within_5_sigma(int((y["flags"] & HFLIP > 0).sum()), n, 0.5)
    assert ((y["flags"] & ~HFLIP) == 0).all()
    shifted = (y["scale"] != 1.0).any(axis=1)
    assert within_5_sigma(int(shifted.sum()), n, 0.5)
    assert y["gamma"].min() >= 2.0 and y["gamma"].max() <= 5.0 and y["gamma"].min() < 2.01 and y["gamma"].max() > 4.99
    assert y["level"].min() >= 0.01 - 1e-9 and y["level"].max() <= 0.05 + 1e-9 and y["level"].min() < 0.0102 and y["level"].max() > 0.0498
    sc = y["scale"][shifted]
    assert sc.min() >= 0.8 - 1e-7 and sc.max() <= 1.0 and sc.min() < 0.801 and sc.max() > 0.999
    assert (y["ca"] == 1.0).all() and (y["sa"] == 0.0).all()


@pytest.mark.parametrize("mode", ["train", "synthetic"])
def test_plan_ranks_partition_the_permutation(mode):
    s, n, b = 16, 50, 4
    sizes = mixed_sizes(n, s, seed=2)
    full = M.epoch_plan(sizes, s, mode, seed=9, epoch=2, batch_size=1)  # batch 1, one rank: the whole permutation in order
    assert sorted(full["low_frame"].tolist()) == list(range(n))
    for world in (1, 2, 3):
        nb = n // (b * world)
        plans = [M.epoch_plan(sizes, s, mode, seed=9, epoch=2, batch_size=b, rank=r, world=world) for r in range(world)]
        seen = []
        for r, p in enumerate(plans):
            assert len(p) == nb * b and D.plan_batches(n, mode, b, r, world) == nb
            for k in range(nb):
                want = full[k * b * world + r * b: k * b * world + (r + 1) * b]
                assert p[k * b:(k + 1) * b].tobytes() == want.tobytes(), (world, r, k)  # the same samples with the same draws
            seen += p["low_frame"].tolist()
        assert len(set(seen)) == len(seen)  # disjoint
        assert sorted(seen) == sorted(full["low_frame"][:nb * b * world].tolist())  # the permutation minus the dropped tail


def test_plan_val():
    s, n, b = 16, 23, 4
    sizes = mixed_sizes(n, s, seed=3)
    v = M.epoch_plan(sizes, s, "val", seed=1, epoch=7, batch_size=b)
    assert len(v) == n and D.plan_batches(n, "val", b) == 6  # the last partial batch is kept
    assert np.array_equal(v["low_frame"], np.arange(n)) and np.array_equal(v["high_frame"], np.arange(n) + n)
    assert np.array_equal(v["y0"], [(h - s) // 2 for h, _ in sizes]) and np.array_equal(v["x0"], [(w - s) // 2 for _, w in sizes])
    assert (v["flags"] == 0).all() and (v["ca"] == 1.0).all() and (v["sa"] == 0.0).all()
    assert v.tobytes() == M.epoch_plan(sizes, s, "val", seed=2, epoch=0, batch_size=b).tobytes()  # nothing is drawn
    for world in (2, 3):
        parts = [M.epoch_plan(sizes, s, "val", 0, 0, b, rank=r, world=world) for r in range(world)]
        for r, p in enumerate(parts):
            lo, hi = M.shard_range(n, r, world)
            assert np.array_equal(p["low_frame"], np.arange(lo, hi))
        assert np.concatenate(parts).tobytes() == v.tobytes()


def test_plan_refusals():
    with pytest.raises(ValueError, match="smaller"):
        M.epoch_plan([(64, 64), (63, 80)], 64, "train", 0, 0, 1)
    with pytest.raises(ValueError, match="mode"):
        M.epoch_plan([(64, 64)], 64, "test", 0, 0, 1)
    with pytest.raises(ValueError):
        M.epoch_plan([(64, 64)], 64, "train", 0, 0, 0)
    with pytest.raises(ValueError):
        M.epoch_plan([(64, 64)], 64, "train", 0, 0, 1, rank=2, world=2)
    with pytest.raises(ValueError):
        M.epoch_plan([], 64, "val", 0, 0, 1)


# ------------------------------------------------------------------ 2. the pair twin against float64
def pair_ref64(frame, y0, x0, flags, ca, sa, s):
    """uint8 [S,S,3] from the definition, in float64 on the plan's (ca, sa)."""
    k = np.arange(s)
    rows = y0 + (s - 1 - k if flags & VFLIP else k)
    cols = x0 + (s - 1 - k if flags & HFLIP else k)
    crop = frame[np.ix_(rows, cols)]
    if not flags & ROTATE:
        return crop
    ca, sa, c = float(ca), float(sa), (s - 1) * 0.5
    x, y = np.meshgrid(k.astype(np.float64), k.astype(np.float64))  # x[y][x] = x
    u, v = x - c, y - c
    xs, ys = ca * u + sa * v + c, -sa * u + ca * v + c
    xi, yi = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    fx, fy = (xs - xi)[:, :, None], (ys - yi)[:, :, None]

    def r(i):
        i = np.where(i < 0, -i, np.where(i >= s, 2 * (s - 1) - i, i))
        assert i.min() >= 0 and i.max() < s  # one reflection suffices up to 15 degrees
        return i

    p = crop.astype(np.float64)
    top = p[r(yi), r(xi)] * (1 - fx) + p[r(yi), r(xi + 1)] * fx
    bot = p[r(yi + 1), r(xi)] * (1 - fx) + p[r(yi + 1), r(xi + 1)] * fx
    out = top * (1 - fy) + bot * fy
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("s", [64, 72, 256])
def test_pair_twin_vs_float64(s):
    """All 8 flag combinations x angles +-15, 0.01 and 0 degrees on white-noise frames, the hardest input (neighbouring bytes
    are unrelated, so an error of the sampling position moves the value most).  fp32 rounding of the position (about 1e-5 of
    a pixel) and of the blend moves the value by about 1e-3 at most, which can flip round-half-up only next to a half: no
    byte differs by more than 1, and over the rotated cases of one size at most 1 byte in 1000 differs.  Without rotation, and at
    0 degrees (xs = x exactly, fx = 0), the twin is exact."""
    frames = noise_frames(2, s + 37, s + 50, seed=s)
    differ = total = 0
    for flags in range(8):
        for ang in (15.0, -15.0, 0.01, 0.0):
            row = one_row(0, 1, y0=(11 * flags) % 38, x0=(7 * flags + 3) % 51, flags=flags, angle_deg=ang)
            low, high, lo8, hi8 = M.augment_pairs_host(frames, row, s, return_bytes=True)
            assert low.dtype == np.float32 and low.shape == (1, 3, s, s) and lo8.dtype == np.uint8 and lo8.shape == (1, s, s, 3)
            for f32, got, frame in ((low, lo8, frames[0]), (high, hi8, frames[1])):
                want = pair_ref64(frame, int(row["y0"][0]), int(row["x0"][0]), flags, row["ca"][0], row["sa"][0], s)
                diff = np.abs(got[0].astype(np.int64) - want.astype(np.int64))
                assert diff.max() <= 1, (flags, ang)
                if not flags & ROTATE or ang == 0.0:
                    assert diff.max() == 0, (flags, ang)
                else:
                    differ, total = differ + int((diff > 0).sum()), total + diff.size
                # the normalisation of hostio.preprocess_array, in NCHW
                assert np.array_equal(f32[0], (got[0].astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(2, 0, 1))
    print(f"pair twin vs float64, S={s}: {differ} of {total} rotated bytes differ ({differ / total:.2e})")
    assert differ <= total / 1000


def test_pair_twin_rotation_is_a_rotation():
    """Guards the restatement itself: a smooth ramp rotated by +a and then by -a returns to itself away from the border, and
    a positive angle moves the image's top edge to the right (xs grows with y)."""
    s = 64
    y, x = np.mgrid[0:s, 0:s]
    ramp = np.stack([2 * x + 60, 2 * y + 60, x + y + 60], axis=-1).astype(np.uint8)
    fwd = M.augment_pairs_host([ramp, ramp], one_row(0, 1, flags=ROTATE, angle_deg=10.0), s, return_bytes=True)[2][0]
    back = M.augment_pairs_host([fwd, fwd], one_row(0, 1, flags=ROTATE, angle_deg=-10.0), s, return_bytes=True)[2][0]
    inner = slice(16, 48)
    assert np.abs(back[inner, inner].astype(int) - ramp[inner, inner].astype(int)).max() <= 2
    assert fwd[40, 32, 0] > ramp[40, 32, 0]  # below the centre the sample position lies further right: larger x ramp


# ------------------------------------------------------------------ 3. the synthetic twin against the reference's bytes
def test_synth_twin_vs_reference_golden():
    """SyntheticLowLightDataset._create_low_light on 12 inputs that hold every byte value (tools/make_golden_synth.py), fed with
    the draws it used: z = noise / level in fp32.  The reference adds the noise in float64; fp32 can flip the truncation only
    where n * 255 lies within about 1e-4 of an integer: no byte differs by more than 1 and at most 1 in 1000 differs."""
    g = np.load(os.path.join(GOLDEN, "synth_lowlight_kat.npz"))
    n, side = g["input"].shape[0], g["input"].shape[1]
    assert n == 12 and g["shift"].any() and not g["shift"].all()
    plan = np.concatenate([one_row(i, i, gamma=g["gamma"][i], level=g["level"][i], scale=g["scale"][i]) for i in range(n)])
    z = (g["noise"] / g["level"][:, None, None, None]).astype(np.float32)
    low, high, lo8, hi8 = M.augment_synth_host(list(g["input"]), plan, z, side, return_bytes=True)
    assert np.array_equal(hi8, g["input"])
    diff = np.abs(lo8.astype(np.int64) - g["output"].astype(np.int64))
    print(f"synthetic twin vs reference: {int((diff > 0).sum())} of {diff.size} bytes differ, max {int(diff.max())}")
    assert diff.max() <= 1
    assert (diff > 0).sum() <= diff.size / 1000
    assert np.array_equal(low, (lo8.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(0, 3, 1, 2))
    assert np.array_equal(high, (hi8.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(0, 3, 1, 2))
    # the crop and hflip of the synthetic path; vflip and rotate bits are ignored
    row = one_row(3, 3, y0=2, x0=5, flags=HFLIP | VFLIP | ROTATE, angle_deg=10.0, gamma=g["gamma"][3], level=0.0)
    hi = M.augment_synth_host(list(g["input"]), row, np.zeros((1, 16, 16, 3), np.float32), 16, return_bytes=True)[3]
    assert np.array_equal(hi[0], g["input"][3][2:18, 5:21][:, ::-1])


# ------------------------------------------------------------------ 4. the store
def write_pngs(folder, frames, prefix="im"):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(folder, f"{prefix}{i:03d}.png"))


def test_store_from_folder(tmp_path):
    low, high = noise_frames(4, 40, 56, seed=1), noise_frames(5, 40, 56, seed=2)
    low[2], high[2] = low[2][:33, :47].copy(), high[2][:33, :47].copy()  # mixed sizes, an odd width
    write_pngs(tmp_path / "a" / "low", low)
    write_pngs(tmp_path / "a" / "high", high)
    (tmp_path / "a" / "low" / "notes.txt").write_text("not an image")
    with pytest.warns(UserWarning, match="first 4"):
        st = M.DeviceFrameStore.from_folder(str(tmp_path / "a"), device="cpu", image_size=32)
    assert len(st) == 4 and st.paired and st.num_frames == 8 and st.names == [f"im{i:03d}.png" for i in range(4)]
    assert st.sizes == [(40, 56), (40, 56), (33, 47), (40, 56)]
    assert st.pool.dtype == torch.uint8 and st.table.dtype == torch.int64 and tuple(st.table.shape) == (8, 3)
    got = st.host_frames()
    for i in range(4):
        assert np.array_equal(got[i], low[i]) and np.array_equal(got[4 + i], high[i])
    offs = st.table[:, 0].tolist()
    assert offs[0] == 0 and all(b >= a + h * w * 3 for a, b, (h, w) in zip(offs, offs[1:], st.sizes + st.sizes))
    # the reference's alternate directory names
    write_pngs(tmp_path / "b" / "lowlight", low[:2])
    write_pngs(tmp_path / "b" / "normal", high[:2])
    alt = M.DeviceFrameStore.from_folder(str(tmp_path / "b"), device="cpu")
    assert len(alt) == 2 and np.array_equal(alt.host_frames()[3], high[1])
    # synthetic: normal-light frames in the root itself
    write_pngs(tmp_path / "c", high[:3])
    syn = M.DeviceFrameStore.from_folder(str(tmp_path / "c"), synthetic=True, device="cpu")
    assert len(syn) == 3 and not syn.paired and syn.num_frames == 3


def test_store_refusals(tmp_path):
    low, high = noise_frames(2, 40, 56, seed=1), noise_frames(2, 40, 56, seed=2)
    write_pngs(tmp_path / "a" / "low", low)
    write_pngs(tmp_path / "a" / "high", high)
    with pytest.raises(ValueError, match="smaller"):
        M.DeviceFrameStore.from_folder(str(tmp_path / "a"), device="cpu", image_size=41)
    st = M.DeviceFrameStore.from_folder(str(tmp_path / "a"), device="cpu")
    with pytest.raises(ValueError, match="smaller"):
        st.require(57)
    with pytest.raises(ValueError, match="smaller"):
        M.DevicePairLoader(st, 2, 64, "train")
    with pytest.raises(ValueError, match="frame store"):
        M.DevicePairLoader(st, 2, 32, "synthetic")
    with pytest.raises(ValueError):  # unequal pair
        M.DeviceFrameStore(low, [high[0], high[1][:39]], device="cpu")
    with pytest.raises(ValueError):  # unequal counts
        M.DeviceFrameStore(low, high[:1], device="cpu")
    with pytest.raises(ValueError):
        M.DeviceFrameStore([], device="cpu")
    with pytest.raises(ValueError):
        M.DeviceFrameStore([low[0].astype(np.float32)], device="cpu")
    os.makedirs(tmp_path / "e" / "low")
    os.makedirs(tmp_path / "e" / "high")
    with pytest.raises(ValueError, match="no images"):
        M.DeviceFrameStore.from_folder(str(tmp_path / "e"), device="cpu")
    os.makedirs(tmp_path / "f" / "low")
    with pytest.raises(FileNotFoundError):
        M.DeviceFrameStore.from_folder(str(tmp_path / "f"), device="cpu")
    with pytest.raises(FileNotFoundError):
        M.DeviceFrameStore.from_folder(str(tmp_path / "missing"), device="cpu")


def test_loader_length_and_refusal_without_a_device():
    st = M.DeviceFrameStore(noise_frames(11, 40, 40, 1), noise_frames(11, 40, 40, 2), device="cpu")
    assert len(M.DevicePairLoader(st, 4, 32, "train")) == 2 and len(M.DevicePairLoader(st, 4, 32, "val")) == 3
    assert len(M.DevicePairLoader(st, 2, 32, "train", rank=1, world=2)) == 2
    with pytest.raises(RuntimeError, match="HIP device"):
        next(iter(M.DevicePairLoader(st, 4, 32, "train")))
    with pytest.raises(RuntimeError, match="HIP device"):
        M.augment_pairs_device(st, M.epoch_plan(st.sizes, 32, "val", 0, 0, 4), 32)
    syn = M.DeviceFrameStore(noise_frames(3, 40, 40, 1), device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        next(iter(M.DevicePairLoader(syn, 2, 32, "synthetic")))


# ------------------------------------------------------------------ 5. the C ABI refuses before anything touches a device
def test_c_abi_argument_checks():
    lib = native.lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    ok_pair = dict(pool=p, table=p, N=1, plan=p, first=0, count=1, S=8, low=p, high=p, lo8=None, hi8=None)

    def pair(**kw):
        a = {**ok_pair, **kw}
        return lib.llie_aug_pair_u8(a["pool"], a["table"], a["N"], a["plan"], a["first"], a["count"], a["S"], a["low"], a["high"], a["lo8"],
                                    a["hi8"], None)

    def synth(z=p, **kw):
        a = {**ok_pair, **kw}
        return lib.llie_aug_synth_u8(a["pool"], a["table"], a["N"], a["plan"], a["first"], a["count"], a["S"], z, a["low"], a["high"],
                                     a["lo8"], a["hi8"], None)

    for bad in (dict(pool=None), dict(table=None), dict(plan=None), dict(low=None), dict(high=None), dict(S=0), dict(S=-4), dict(count=-1),
                dict(N=0), dict(first=-1)):
        assert pair(**bad) == native.ERR_ARG, bad
        assert synth(**bad) == native.ERR_ARG, bad
    assert synth(z=None) == native.ERR_ARG
    # count == 0 is accepted and launches nothing (this machine may have no device at all)
    assert pair(count=0) == 0 and synth(count=0) == 0
