"""Device-resident paired data loader: the training frames are decoded once and stay on the device as uint8; every batch is one
kernel launch (csrc/augment.hip) that crops, flips, rotates or degrades, and normalises them into the fp32 `[B,3,S,S]` pair
`TrainStep` takes.  It stands where the reference's `DataLoader` over `LowLightDataset` / `SyntheticLowLightDataset` stands
(src/training/dataset.py) and yields the same dictionary.

One definition serves the NumPy twins here, the kernels and the tests:

  store   one uint8 pool of HWC RGB frames with packed rows and a table int64 [N][3] = (byte offset, H, W).  A paired store of
          n pairs holds the low-light frames at 0 .. n-1 and the normal-light frames at n .. 2n-1; a synthetic store holds the
          normal-light frames only
  plan    one row per sample (PLAN_DTYPE == llie_aug_row): low_frame, high_frame, y0, x0, flags (HFLIP | VFLIP | ROTATE), ca, sa
          (cos and sin of the angle, computed in float64 and rounded to fp32 once, so kernel and twin use identical values),
          gamma, level, scale[3]
  crop    SH rows x SW columns (`image_size` = an int S: SH = SW = S; a pair (H, W): SH = H, SW = W, for frame-size training);
          crop(yy, xx) = frame[y0 + (vflip ? SH-1-yy : yy)][x0 + (hflip ? SW-1-xx : xx)]
  pair    no rotate: byte = crop(y, x).  rotate: cx = (SW-1)/2, cy = (SH-1)/2, u = x - cx, v = y - cy, xs = (ca*u + sa*v) + cx,
          ys = ((-sa)*u + ca*v) + cy; bilinear over floor / floor + 1 with reflect-101 borders, each axis with its own length,
          top = p00*(1-fx) + p01*fx, bot likewise, out = top*(1-fy) + bot*fy, byte = clip(floor(out + 0.5), 0, 255);
          every multiply and add is a separate fp32 operation
  synth   (SyntheticLowLightDataset._create_low_light) nb = crop(y, x) with hflip only; d = (nb / 255) ** gamma;
          n = clip(d + level * z, 0, 1); n = clip(n * scale[c], 0, 1); low byte = trunc(n * 255); normal byte = nb
  value   float(byte) / 127.5 - 1

The random draws of `epoch_plan` come from this module's own stream (a CPU `torch.Generator`), not from albumentations' or
NumPy's: the distributions are the reference's, the individual samples are not.  The geometric augmentation is pinned to the
twins here and to a float64 restatement in the tests, not to albumentations / cv2 (DESIGN.md has the details).  The device
functions have no CPU fallback.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N
from .sharding import shard_range

HFLIP, VFLIP, ROTATE = 1, 2, 4  # LLIE_AUG_* (include/llie.h)
PLAN_DTYPE = np.dtype([("low_frame", "<i4"), ("high_frame", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("flags", "<i4"), ("ca", "<f4"),
                       ("sa", "<f4"), ("gamma", "<f4"), ("level", "<f4"), ("scale", "<f4", (3,))])
assert PLAN_DTYPE.itemsize == 48
MODES = ("train", "synthetic", "val")
MAX_ANGLE_DEG = 15.0
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp")
_LOW_ALTERNATES, _HIGH_ALTERNATES = ("low", "lowlight", "dark"), ("high", "normal", "bright")


CropSize = Union[int, Tuple[int, int]]


def crop_hw(image_size: CropSize) -> Tuple[int, int]:
    """(SH, SW) of a crop given as an int S (square) or a pair (H, W)."""
    if isinstance(image_size, (tuple, list)):
        if len(image_size) != 2:
            raise ValueError(f"image_size must be an int or (H, W), got {image_size!r}")
        return int(image_size[0]), int(image_size[1])
    return int(image_size), int(image_size)


def _check_frame(f, what: str) -> np.ndarray:
    a = np.asarray(f)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{what} must be a uint8 RGB image [H, W, 3], got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


# ------------------------------------------------------------------ the frame store
class DeviceFrameStore:
    """Every frame of a data set as uint8 on `device`: `pool` (uint8 [bytes]) and `table` (int64 [N,3]) as the kernels read them.

    `low_frames` / `high_frames` are sequences of uint8 [H,W,3] arrays; the two frames of a pair must have one size.  With
    `high_frames=None` the store is synthetic: `low_frames` are then the normal-light frames and the low-light image is made
    from them on the device.  `image_size`, when given, refuses frames smaller than that crop at once (`require` does the same
    later).  `device="cpu"` keeps the arrays on the host, which serves the host twins; the kernels need a HIP device."""

    def __init__(self, low_frames: Sequence[np.ndarray], high_frames: Optional[Sequence[np.ndarray]] = None, device="cuda",
                 names: Optional[Sequence[str]] = None, image_size: Optional[CropSize] = None):
        low = [_check_frame(f, f"frame {i}") for i, f in enumerate(low_frames)]
        if not low:
            raise ValueError("a frame store needs at least one frame")
        self.paired = high_frames is not None
        frames = list(low)
        if self.paired:
            high = [_check_frame(f, f"normal-light frame {i}") for i, f in enumerate(high_frames)]
            if len(high) != len(low):
                raise ValueError(f"{len(low)} low-light frames but {len(high)} normal-light frames")
            for i, (a, b) in enumerate(zip(low, high)):
                if a.shape != b.shape:
                    raise ValueError(f"pair {i}: the low-light frame is {a.shape[0]}x{a.shape[1]}, the normal-light frame "
                                     f"{b.shape[0]}x{b.shape[1]}")
            frames += high
        self.num_pairs = len(low)
        self.names = [str(n) for n in names] if names is not None else [f"{i:06d}" for i in range(len(low))]
        if len(self.names) != len(low):
            raise ValueError(f"{len(self.names)} names for {len(low)} frames")
        self.sizes: List[Tuple[int, int]] = [(f.shape[0], f.shape[1]) for f in low]
        if image_size is not None:
            self.require(image_size)
        table = np.empty((len(frames), 3), dtype=np.int64)
        off = 0
        for i, f in enumerate(frames):
            table[i] = (off, f.shape[0], f.shape[1])
            off += (f.size + 15) // 16 * 16  # frames start on 16-byte boundaries
        pool = np.zeros(off, dtype=np.uint8)
        for f, (o, _, _) in zip(frames, table):
            pool[o:o + f.size] = f.reshape(-1)
        self.pool = torch.from_numpy(pool).to(torch.device(device))
        self.device = self.pool.device  # with its index, as tensors report it
        self.table = torch.from_numpy(table).to(self.device)
        self._host_table = table

    def __len__(self) -> int:
        return self.num_pairs

    @property
    def num_frames(self) -> int:
        return self._host_table.shape[0]

    def require(self, image_size: CropSize) -> None:
        """ValueError unless every frame holds an `image_size` crop (an int S, or (H, W))."""
        sh, sw = crop_hw(image_size)
        if sh < 1 or sw < 1:
            raise ValueError(f"image_size must be positive, got {image_size}")
        for name, (h, w) in zip(self.names, self.sizes):
            if h < sh or w < sw:
                raise ValueError(f"frame {name} is {h}x{w}: smaller than the {sh}x{sw} crop")

    def frame(self, index: int) -> torch.Tensor:
        """Frame `index` as a uint8 [H,W,3] view into the pool (no copy): low-light frames are 0 .. n-1, normal-light frames
        n .. 2n-1 in a paired store."""
        i = int(index)
        if not 0 <= i < self.num_frames:
            raise IndexError(f"frame {index} of a store of {self.num_frames} frames")
        o, h, w = (int(v) for v in self._host_table[i])
        return self.pool[o:o + h * w * 3].view(h, w, 3)

    def host_frames(self) -> List[np.ndarray]:
        """The frames as NumPy arrays, in table order (what the host twins take)."""
        pool = self.pool.cpu().numpy()
        return [pool[o:o + h * w * 3].reshape(h, w, 3) for o, h, w in self._host_table]

    @classmethod
    def from_folder(cls, root: str, low_dir: str = "low", high_dir: str = "high", extensions: Tuple[str, ...] = IMAGE_EXTENSIONS,
                    synthetic: bool = False, device="cuda", image_size: Optional[CropSize] = None) -> "DeviceFrameStore":
        """Decode a data set with PIL.  Paired: `root/low_dir` and `root/high_dir`, or the alternates lowlight / dark and
        normal / bright when `root/low_dir` does not exist; files sorted by name; the longer list is cut to the shorter one.
        `synthetic=True`: the normal-light images lie in `root` itself."""
        from PIL import Image

        def listing(path: str) -> List[str]:
            files = sorted(f for f in os.listdir(path)
                           if os.path.isfile(os.path.join(path, f)) and os.path.splitext(f)[1].lower() in extensions)
            if not files:
                raise ValueError(f"no images in {path} (extensions {extensions})")
            return [os.path.join(path, f) for f in files]

        def decode(paths: List[str]) -> List[np.ndarray]:
            return [np.array(Image.open(p).convert("RGB")) for p in paths]

        if not os.path.isdir(root):
            raise FileNotFoundError(f"data set root not found: {root}")
        if synthetic:
            files = listing(root)
            return cls(decode(files), None, device, [os.path.basename(p) for p in files], image_size)
        low_path, high_path = os.path.join(root, low_dir), os.path.join(root, high_dir)
        if not os.path.isdir(low_path):
            low_path = next((p for p in (os.path.join(root, d) for d in (low_dir,) + _LOW_ALTERNATES) if os.path.isdir(p)), low_path)
            high_path = next((p for p in (os.path.join(root, d) for d in (high_dir,) + _HIGH_ALTERNATES) if os.path.isdir(p)), high_path)
        for path, kind in ((low_path, "low-light"), (high_path, "normal-light")):
            if not os.path.isdir(path):
                raise FileNotFoundError(f"{kind} directory not found: {path}")
        low, high = listing(low_path), listing(high_path)
        if len(low) != len(high):
            n = min(len(low), len(high))
            warnings.warn(f"{len(low)} low-light but {len(high)} normal-light images under {root}: using the first {n} of each")
            low, high = low[:n], high[:n]
        return cls(decode(low), decode(high), device, [os.path.basename(p) for p in low], image_size)


# ------------------------------------------------------------------ the epoch plan
def _plan_seed(seed: int, epoch: int, rank: int = 0) -> int:
    return (int(seed) * 1000003 + int(epoch) * 8191 + int(rank) * 131 + 12345) % (2 ** 63 - 1)


def plan_batches(num_pairs: int, mode: str, batch_size: int, rank: int = 0, world: int = 1) -> int:
    """Batches one rank sees in an epoch."""
    if mode == "val":
        lo, hi = shard_range(num_pairs, rank, world)
        return -(-(hi - lo) // batch_size)
    return num_pairs // (batch_size * world)


def epoch_plan(sizes: Sequence[Tuple[int, int]], image_size: CropSize, mode: str, seed: int, epoch: int, batch_size: int, rank: int = 0,
               world: int = 1, gamma_range: Tuple[float, float] = (2.0, 5.0),
               noise_level_range: Tuple[float, float] = (0.01, 0.05)) -> np.ndarray:
    """The rows (PLAN_DTYPE) of one rank for one epoch, in the order its batches consume them: a pure function of the arguments.

    `sizes[i]` is the (H, W) of pair i; `image_size` the crop, an int S or (SH, SW) (S stands for the axis's own length below;
    an int gives the plan (S, S) gives).  Every rank draws the same global plan from a CPU generator seeded with (seed, epoch)
    and keeps its own rows, so the union over the ranks does not depend on the world size.

      "train"      shuffled; origin uniform over [0, H-S] x [0, W-S]; hflip p = 0.5, vflip p = 0.3, rotation p = 0.3 by an angle
                   uniform in [-15, 15] degrees (LowLightDataset with augment=True)
      "synthetic"  shuffled; origin as above; hflip p = 0.5; gamma and level uniform in their ranges; colour shift p = 0.5 with
                   scale uniform in [0.8, 1]^3 (SyntheticLowLightDataset)
      "val"        file order, centre crop, no flags (LowLightDataset with augment=False)

    "train" and "synthetic" drop the last partial global batch (drop_last=True): global batch k is perm[k B world : (k+1) B world]
    and rank r takes [r B, (r+1) B) of it.  "val" keeps every pair: rank r takes shard_range(n, r, world) of the file order.
    In a paired store the normal-light frame of pair i is frame n + i; "synthetic" reads frame i for both."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    (sh, sw), n, b = crop_hw(image_size), len(sizes), int(batch_size)
    if n < 1 or sh < 1 or sw < 1 or b < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_plan: {n} pairs, image_size {image_size}, batch_size {b}, rank {rank} of {world}")
    hw = np.asarray(sizes, dtype=np.int64).reshape(n, 2)
    small = hw < np.array([sh, sw], dtype=np.int64)
    if small.any():
        i = int(np.argmax(small.any(axis=1)))
        raise ValueError(f"pair {i} is {hw[i, 0]}x{hw[i, 1]}: smaller than the {sh}x{sw} crop")
    if mode == "val":
        lo, hi = shard_range(n, rank, world)
        plan = np.zeros(hi - lo, dtype=PLAN_DTYPE)
        idx = np.arange(lo, hi)
        plan["low_frame"], plan["high_frame"] = idx, idx + n
        plan["y0"], plan["x0"] = (hw[idx, 0] - sh) // 2, (hw[idx, 1] - sw) // 2
        plan["ca"], plan["gamma"], plan["scale"] = 1.0, 1.0, 1.0
        return plan
    g = torch.Generator().manual_seed(_plan_seed(seed, epoch))
    perm = torch.randperm(n, generator=g).numpy()
    nb = n // (b * world)
    u = torch.rand(n, 12, dtype=torch.float64, generator=g).numpy()  # a row of draws per position of the global order, whatever B and world
    rows = (np.arange(nb)[:, None] * (b * world) + rank * b + np.arange(b)[None, :]).reshape(-1)
    idx, u = perm[rows], u[rows]
    plan = np.zeros(rows.size, dtype=PLAN_DTYPE)
    plan["low_frame"] = idx
    plan["high_frame"] = idx if mode == "synthetic" else idx + n
    room_y, room_x = hw[idx, 0] - sh, hw[idx, 1] - sw
    plan["y0"] = np.minimum((u[:, 0] * (room_y + 1)).astype(np.int64), room_y)
    plan["x0"] = np.minimum((u[:, 1] * (room_x + 1)).astype(np.int64), room_x)
    flags = np.where(u[:, 2] < 0.5, HFLIP, 0)
    plan["ca"], plan["gamma"], plan["scale"] = 1.0, 1.0, 1.0
    if mode == "train":
        rot = u[:, 4] < 0.3
        flags = flags | np.where(u[:, 3] < 0.3, VFLIP, 0) | np.where(rot, ROTATE, 0)
        angle = np.where(rot, np.radians((2.0 * u[:, 5] - 1.0) * MAX_ANGLE_DEG), 0.0)
        plan["ca"], plan["sa"] = np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)
    else:
        plan["gamma"] = gamma_range[0] + u[:, 6] * (gamma_range[1] - gamma_range[0])
        plan["level"] = noise_level_range[0] + u[:, 7] * (noise_level_range[1] - noise_level_range[0])
        plan["scale"] = np.where((u[:, 8] < 0.5)[:, None], 0.8 + 0.2 * u[:, 9:12], 1.0)
    plan["flags"] = flags
    return plan


# ------------------------------------------------------------------ host twins (fp32 NumPy)
def _as_plan(plan) -> np.ndarray:
    plan = np.asarray(plan)
    if plan.dtype != PLAN_DTYPE or plan.ndim != 1:
        raise ValueError(f"a plan is a 1-d array of PLAN_DTYPE, got {plan.dtype} {plan.shape}")
    return plan


def _chunk(total: int, first: int, count: Optional[int]) -> int:
    count = total - first if count is None else count
    if first < 0 or count < 0 or first + count > total:
        raise ValueError(f"rows [{first}, {first + count}) lie outside the plan of {total} rows")
    return count


def _crop(frames: Sequence[np.ndarray], index: int, row, sh: int, sw: int, flags: int) -> np.ndarray:
    """uint8 [SH,SW,3]: crop(yy, xx) for all yy, xx, with the kernels' clamps of the frame index, the origin, rows and columns."""
    f = frames[min(max(int(index), 0), len(frames) - 1)]
    h, w = f.shape[:2]
    y0, x0 = max(min(int(row["y0"]), h - sh), 0), max(min(int(row["x0"]), w - sw), 0)
    ky, kx = np.arange(sh), np.arange(sw)
    yy = np.minimum(y0 + (sh - 1 - ky if flags & VFLIP else ky), h - 1)
    xx = np.minimum(x0 + (sw - 1 - kx if flags & HFLIP else kx), w - 1)
    return f[yy][:, xx]


def _reflect(i: np.ndarray, s: int) -> np.ndarray:
    i = np.where(i < 0, -i, np.where(i >= s, 2 * (s - 1) - i, i))
    return np.clip(i, 0, s - 1)


def _rotate(crop: np.ndarray, ca: np.float32, sa: np.float32) -> np.ndarray:
    """uint8 [SH,SW,3] -> uint8 [SH,SW,3]: the rotation of the module docstring, operation for operation in fp32."""
    sh, sw = crop.shape[:2]
    one, half = np.float32(1.0), np.float32(0.5)
    cx, cy = np.float32(sw - 1) * half, np.float32(sh - 1) * half
    u = (np.arange(sw, dtype=np.float32) - cx)[None, :]
    v = (np.arange(sh, dtype=np.float32) - cy)[:, None]
    xs = (ca * u + sa * v) + cx
    ys = ((-sa) * u + ca * v) + cy
    xf, yf = np.floor(xs), np.floor(ys)
    fx, fy = (xs - xf)[:, :, None], (ys - yf)[:, :, None]
    gx, gy = one - fx, one - fy
    with np.errstate(invalid="ignore"):
        xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    xa, xb, ya, yb = _reflect(xi, sw), _reflect(xi + 1, sw), _reflect(yi, sh), _reflect(yi + 1, sh)
    p = crop.astype(np.float32)
    top = p[ya, xa] * gx + p[ya, xb] * fx
    bot = p[yb, xa] * gx + p[yb, xb] * fx
    out = top * gy + bot * fy
    assert out.dtype == np.float32
    return np.clip(np.floor(out + half), 0, 255).astype(np.uint8)


def _normalise(u8: np.ndarray) -> np.ndarray:
    """uint8 [n,S,S,3] -> fp32 [n,3,S,S], hostio.preprocess_array's x / 127.5 - 1."""
    return np.ascontiguousarray((u8.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(0, 3, 1, 2))


def augment_pairs_host(frames: Sequence[np.ndarray], plan: np.ndarray, image_size: CropSize, first: int = 0,
                       count: Optional[int] = None, return_bytes: bool = False):
    """Host twin of aug_pair_u8 (aug_pair_u8_hw when `image_size` is (SH, SW)).  `frames` in table order
    (DeviceFrameStore.host_frames) -> (low, normal) fp32 [count,3,SH,SW] for plan rows [first, first + count); with `return_bytes`
    also the two uint8 [count,SH,SW,3] images before normalisation."""
    plan, (sh, sw) = _as_plan(plan), crop_hw(image_size)
    count = _chunk(len(plan), first, count)
    lo = np.empty((count, sh, sw, 3), dtype=np.uint8)
    hi = np.empty_like(lo)
    for j in range(count):
        row = plan[first + j]
        flags = int(row["flags"])
        for out, index in ((lo, row["low_frame"]), (hi, row["high_frame"])):
            crop = _crop(frames, index, row, sh, sw, flags)
            out[j] = _rotate(crop, row["ca"], row["sa"]) if flags & ROTATE else crop
    res = (_normalise(lo), _normalise(hi))
    return res + (lo, hi) if return_bytes else res


def augment_synth_host(frames: Sequence[np.ndarray], plan: np.ndarray, z: np.ndarray, image_size: CropSize, first: int = 0,
                       count: Optional[int] = None, return_bytes: bool = False):
    """Host twin of aug_synth_u8 (aug_synth_u8_hw when `image_size` is (SH, SW)).  `z`: fp32 [count,SH,SW,3] standard-normal
    draws.  Returns as augment_pairs_host."""
    plan, (sh, sw) = _as_plan(plan), crop_hw(image_size)
    count = _chunk(len(plan), first, count)
    z = np.asarray(z)
    if z.dtype != np.float32 or z.shape != (count, sh, sw, 3):
        raise ValueError(f"z must be fp32 [{count},{sh},{sw},3], got {z.dtype} {z.shape}")
    lo = np.empty((count, sh, sw, 3), dtype=np.uint8)
    hi = np.empty_like(lo)
    zero, one = np.float32(0.0), np.float32(1.0)
    for j in range(count):
        row = plan[first + j]
        nb = _crop(frames, row["high_frame"], row, sh, sw, int(row["flags"]) & HFLIP)
        with np.errstate(invalid="ignore"):
            lut = np.power(np.arange(256, dtype=np.float32) / np.float32(255.0), row["gamma"])
        n = np.clip(lut[nb] + row["level"] * z[j], zero, one)
        n = np.clip(n * row["scale"][None, None, :], zero, one)
        assert n.dtype == np.float32
        lo[j] = (n * np.float32(255.0)).astype(np.uint8)
        hi[j] = nb
    res = (_normalise(lo), _normalise(hi))
    return res + (lo, hi) if return_bytes else res


# ------------------------------------------------------------------ device functions
def plan_to_device(plan: np.ndarray, device) -> torch.Tensor:
    """PLAN_DTYPE rows -> int32 [rows, 12] on `device` (the floats keep their bits): llie_aug_row as the kernels read it."""
    words = np.ascontiguousarray(_as_plan(plan)).view(np.int32).reshape(-1, PLAN_DTYPE.itemsize // 4)
    return torch.from_numpy(words.copy()).to(device)


def _device_plan(store: DeviceFrameStore, plan) -> torch.Tensor:
    if isinstance(plan, np.ndarray):
        plan = plan_to_device(plan, store.device)
    if not isinstance(plan, torch.Tensor) or plan.dtype != torch.int32 or plan.dim() != 2 or plan.shape[1] != 12 or not plan.is_contiguous():
        raise ValueError("a device plan is a contiguous int32 [rows, 12] tensor (plan_to_device)")
    if plan.device != store.device:
        raise ValueError(f"the plan is on {plan.device}, the frame store on {store.device}")
    return plan


def _launch(store: DeviceFrameStore, plan, first: int, count: Optional[int], image_size: CropSize, z: Optional[torch.Tensor],
            return_bytes: bool, what: str):
    if store.device.type != "cuda":
        raise RuntimeError(f"{what} runs only on a HIP device (the frame store is on '{store.device}'); there is no CPU fallback")
    sh, sw = crop_hw(image_size)
    store.require((sh, sw))
    plan = _device_plan(store, plan)
    count = _chunk(plan.shape[0], first, count)
    dev = store.device
    low = torch.empty(count, 3, sh, sw, dtype=torch.float32, device=dev)
    high = torch.empty_like(low)
    lo8 = torch.empty(count, sh, sw, 3, dtype=torch.uint8, device=dev) if return_bytes else None
    hi8 = torch.empty_like(lo8) if return_bytes else None
    ptr8 = (lo8.data_ptr(), hi8.data_ptr()) if return_bytes else (None, None)
    L = N.lib()
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        head = (store.pool.data_ptr(), store.table.data_ptr(), store.num_frames, plan.data_ptr(), first, count, sh, sw)
        if z is None:
            N.check(L.llie_aug_pair_u8_hw(*head, low.data_ptr(), high.data_ptr(), *ptr8, st), what)
        else:
            if z.dtype != torch.float32 or tuple(z.shape) != (count, sh, sw, 3) or z.device != dev or not z.is_contiguous():
                raise ValueError(f"z must be a contiguous fp32 [{count},{sh},{sw},3] tensor on {dev}")
            N.check(L.llie_aug_synth_u8_hw(*head, z.data_ptr(), low.data_ptr(), high.data_ptr(), *ptr8, st), what)
    return (low, high, lo8, hi8) if return_bytes else (low, high)


def augment_pairs_device(store: DeviceFrameStore, plan, image_size: CropSize, first: int = 0, count: Optional[int] = None,
                         return_bytes: bool = False):
    """Device twin of augment_pairs_host: one launch of aug_pair_u8 for plan rows [first, first + count) on the current stream.
    `plan`: PLAN_DTYPE rows (uploaded here) or the tensor plan_to_device made (no copy)."""
    return _launch(store, plan, first, count, image_size, None, return_bytes, "aug_pair_u8")


def augment_synth_device(store: DeviceFrameStore, plan, z: torch.Tensor, image_size: CropSize, first: int = 0, count: Optional[int] = None,
                         return_bytes: bool = False):
    """Device twin of augment_synth_host: one launch of aug_synth_u8; `z` fp32 [count,SH,SW,3] on the store's device."""
    if not isinstance(z, torch.Tensor):
        raise ValueError(f"z must be a torch.Tensor, got {type(z).__name__}")
    return _launch(store, plan, first, count, image_size, z, return_bytes, "aug_synth_u8")


# ------------------------------------------------------------------ the loader
class DevicePairLoader:
    """Iterates one rank's batches of an epoch: dictionaries {"low_light", "normal_light", "filename"} as the reference's
    DataLoader yields them, the tensors fp32 [B,3,S,S], contiguous, on the store's device.  `image_size` may be (H, W): the
    batches are then [B,3,H,W] crops for frame-size training (`crop_size` reads the shape of either kind; `image_size` reads the
    side of a square loader and raises for a rectangular one, so code that assumes a square fails loudly).

    The epoch's plan is uploaded once when the iteration starts; after that a batch is one kernel launch on the current stream
    (plus one `randn` on the device in "synthetic" mode): no host-to-device copy and no synchronisation.  `set_epoch(e)` chooses
    the epoch; each started iteration then moves on to the next one, as a shuffling DataLoader does.  Same (seed, epoch, rank,
    world) gives the same batches; "synthetic" noise comes from a device generator seeded from (seed, epoch, rank)."""

    def __init__(self, store: DeviceFrameStore, batch_size: int, image_size: CropSize, mode: str, seed: int = 0, rank: int = 0, world: int = 1,
                 gamma_range: Tuple[float, float] = (2.0, 5.0), noise_level_range: Tuple[float, float] = (0.01, 0.05)):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        if (mode == "synthetic") == store.paired:
            raise ValueError(f"mode {mode!r} needs a {'synthetic (normal-light only)' if store.paired else 'paired'} frame store")
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"batch_size {batch_size}, rank {rank} of {world}")
        store.require(image_size)
        self.store, self.batch_size, self.mode = store, int(batch_size), mode
        # an int stays an int all the way down (a square loader is what it was); a pair is kept as (H, W), (S, S) included
        self._crop = crop_hw(image_size) if isinstance(image_size, (tuple, list)) else int(image_size)
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), 0
        self.gamma_range, self.noise_level_range = tuple(gamma_range), tuple(noise_level_range)

    def __len__(self) -> int:
        return plan_batches(len(self.store), self.mode, self.batch_size, self.rank, self.world)

    @property
    def crop_size(self) -> Tuple[int, int]:
        """(H, W) of the batches."""
        return crop_hw(self._crop)

    @property
    def image_size(self) -> int:
        """The side of a square loader; ValueError for a rectangular one (`crop_size` serves both)."""
        h, w = self.crop_size
        if h != w:
            raise ValueError(f"this loader yields {h}x{w} crops: it has no image_size, read crop_size")
        return h

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def plan(self, epoch: Optional[int] = None) -> np.ndarray:
        """The plan of `epoch` (default: the one the next iteration uses)."""
        return epoch_plan(self.store.sizes, self._crop, self.mode, self.seed, self.epoch if epoch is None else epoch, self.batch_size,
                          self.rank, self.world, self.gamma_range, self.noise_level_range)

    def noise_generator(self, epoch: int) -> torch.Generator:
        """The device generator "synthetic" mode draws an epoch's z from, batch by batch: seeded from (seed, epoch, rank)."""
        return torch.Generator(device=self.store.device).manual_seed(_plan_seed(self.seed, epoch, self.rank + 1))

    def __iter__(self) -> Iterator[Dict[str, object]]:
        dev, s, (sh, sw) = self.store.device, self._crop, self.crop_size
        if dev.type != "cuda":
            raise RuntimeError(f"DevicePairLoader runs only on a HIP device (the frame store is on '{dev}'); there is no CPU fallback")
        epoch = self.epoch
        self.epoch += 1
        plan = self.plan(epoch)
        plan_dev = plan_to_device(plan, dev)
        names = [self.store.names[i] for i in plan["low_frame"]]
        gen = self.noise_generator(epoch) if self.mode == "synthetic" else None
        for first in range(0, len(plan), self.batch_size):
            count = min(self.batch_size, len(plan) - first)
            if self.mode == "synthetic":
                z = torch.randn(count, sh, sw, 3, dtype=torch.float32, device=dev, generator=gen)
                low, high = augment_synth_device(self.store, plan_dev, z, s, first, count)
            else:
                low, high = augment_pairs_device(self.store, plan_dev, s, first, count)
            yield {"low_light": low, "normal_light": high, "filename": names[first:first + count]}


def create_device_dataloaders(train_root: str, val_root: Optional[str] = None, batch_size: int = 8, image_size: CropSize = 256,
                              use_synthetic: bool = False, device="cuda",
                              seed: int = 0) -> Tuple[DevicePairLoader, Optional[DevicePairLoader]]:
    """(train_loader, val_loader or None) as the reference's create_dataloaders: the training loader shuffles, augments and drops
    the last partial batch ("synthetic" over the images in `train_root` itself when `use_synthetic`), the validation loader
    centre-crops in file order.  `image_size` may be (H, W).  One process; under data parallelism build the loaders with their rank and world."""
    train_store = DeviceFrameStore.from_folder(train_root, synthetic=use_synthetic, device=device, image_size=image_size)
    train = DevicePairLoader(train_store, batch_size, image_size, "synthetic" if use_synthetic else "train", seed)
    val = None
    if val_root is not None:
        val = DevicePairLoader(DeviceFrameStore.from_folder(val_root, device=device, image_size=image_size), batch_size, image_size, "val", seed)
    return train, val
