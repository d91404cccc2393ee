"""Full-resolution enhancement: an image of any size is cut into overlapping S x S tiles (S = model.image_size), the tiles go
through `LowLightDiffusion.enhance` as batches, and the overlaps are blended with a feathered window.

One definition serves the NumPy twins here, the kernels (csrc/tiles.hip) and the tests:

  plan, per axis of length L, overlap v (0 <= v <= S/2): one tile at origin 0 if L <= S, else n = ceil((L - S) / (S - v)) + 1
      tiles at o_i = floor(i (L - S) / (n - 1)); tiles of an image are numbered row-major, t = iy * nx + ix
  gather   tile[t][c][y][x] = float(img[min(oy + y, H-1)][min(ox + x, W-1)][c]) / 127.5f - 1.0f
  noise    one canvas [steps][3][max(H,S)][max(W,S)] per image; tile t reads canvas[k][c][oy + y][ox + x], so overlapping
           tiles denoise the same noise where they overlap
  window   w[k] = min(k + 1, S - k, v) / v   (1 if v == 0)
  blend    per pixel and channel over the covering tiles in ascending t: g = w[Y - oy] * w[X - ox]; num += val * g; den += g
           (separate fp32 multiply and add); out = uint8(trunc(clip((num / den + 1) * 127.5, 0, 255)))

Frame mode (`enhance_frame_u8`) is the other route for images under the engine's size cap: no tiles, the network runs once at
the image's own size (`LowLightDiffusion.enhance_frame`), padded to sides the network takes:

  pad      frame_pad(L) = max(64, 8 * ceil(L / 8))
  load     out[c][y][x] = float(img[min(y, H-1)][min(x, W-1)][c]) / 127.5f - 1.0f   for y < frame_pad(H), x < frame_pad(W)
  store    img[y][x][c] = uint8(trunc(clip((x[c][y][x] + 1) * 127.5, 0, 255)))      for y < H, x < W

The device functions are bit-exact with the host twins.  There is no CPU fallback for `enhance_tiled` or `enhance_frame_u8`.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _native as N


def _check_plan(tile: int, overlap: int) -> None:
    if tile <= 0:
        raise ValueError(f"tile side must be positive, got {tile}")
    if overlap < 0 or 2 * overlap > tile:
        raise ValueError(f"overlap must lie in 0..{tile // 2} (half the tile side {tile}), got {overlap}")


def tile_origins(length: int, tile: int, overlap: int) -> List[int]:
    """Origins of the tiles along one axis of `length` pixels (see the module docstring)."""
    _check_plan(tile, overlap)
    if length <= 0:
        raise ValueError(f"length must be positive, got {length}")
    if length <= tile:
        return [0]
    n = -(-(length - tile) // (tile - overlap)) + 1
    return [i * (length - tile) // (n - 1) for i in range(n)]


def tile_window(tile: int, overlap: int) -> np.ndarray:
    """fp32 [tile]: the feathering weights of one axis."""
    _check_plan(tile, overlap)
    if overlap == 0:
        return np.ones(tile, dtype=np.float32)
    k = np.arange(tile)
    return np.minimum(np.minimum(k + 1, tile - k), overlap).astype(np.float32) / np.float32(overlap)


def _check_image(rgb_u8, what: str) -> Tuple[int, int]:
    if str(rgb_u8.dtype) not in ("uint8", "torch.uint8"):
        raise ValueError(f"{what} expects a uint8 image, got {rgb_u8.dtype}")
    if len(rgb_u8.shape) != 3 or rgb_u8.shape[2] != 3 or rgb_u8.shape[0] < 1 or rgb_u8.shape[1] < 1:
        raise ValueError(f"{what} expects an RGB image [H, W, 3], got {tuple(rgb_u8.shape)}")
    return int(rgb_u8.shape[0]), int(rgb_u8.shape[1])


# ------------------------------------------------------------------ host twins (fp32 NumPy)
def gather_tiles_array(rgb_u8: np.ndarray, tile: int, overlap: int) -> np.ndarray:
    """uint8 [H,W,3] -> fp32 [T,3,S,S] in [-1,1], T = ny * nx tiles in row-major order."""
    h, w = _check_image(rgb_u8, "gather_tiles_array")
    oys, oxs = tile_origins(h, tile, overlap), tile_origins(w, tile, overlap)
    out = np.empty((len(oys) * len(oxs), 3, tile, tile), dtype=np.float32)
    k = np.arange(tile)
    for iy, oy in enumerate(oys):
        rows = rgb_u8[np.minimum(oy + k, h - 1)]
        for ix, ox in enumerate(oxs):
            px = rows[:, np.minimum(ox + k, w - 1)]
            out[iy * len(oxs) + ix] = (px.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(2, 0, 1)
    return out


def blend_accumulate_array(tiles: np.ndarray, size: Tuple[int, int], overlap: int) -> np.ndarray:
    """fp32 [T,3,S,S] -> fp32 [H,W,3]: the blended image num / den before denormalisation (tile by tile, ascending t)."""
    h, w = int(size[0]), int(size[1])
    if tiles.ndim != 4 or tiles.shape[1] != 3 or tiles.shape[2] != tiles.shape[3]:
        raise ValueError(f"expected tiles [T,3,S,S], got {tiles.shape}")
    s = tiles.shape[2]
    oys, oxs = tile_origins(h, s, overlap), tile_origins(w, s, overlap)
    if tiles.shape[0] != len(oys) * len(oxs):
        raise ValueError(f"a {h}x{w} image has {len(oys) * len(oxs)} tiles of side {s} at overlap {overlap}, got {tiles.shape[0]}")
    tiles = tiles.astype(np.float32, copy=False)
    win = tile_window(s, overlap)
    num = np.zeros((h, w, 3), dtype=np.float32)
    den = np.zeros((h, w), dtype=np.float32)
    for iy, oy in enumerate(oys):
        th = min(s, h - oy)  # < S only where the image is smaller than a tile: the replicated rest is dropped
        for ix, ox in enumerate(oxs):
            tw = min(s, w - ox)
            g = win[:th, None] * win[None, :tw]
            val = tiles[iy * len(oxs) + ix, :, :th, :tw].transpose(1, 2, 0)
            num[oy:oy + th, ox:ox + tw] = num[oy:oy + th, ox:ox + tw] + val * g[:, :, None]
            den[oy:oy + th, ox:ox + tw] = den[oy:oy + th, ox:ox + tw] + g
    return num / den[:, :, None]


def blend_tiles_array(tiles: np.ndarray, size: Tuple[int, int], overlap: int) -> np.ndarray:
    """fp32 [T,3,S,S] -> uint8 [H,W,3]: feathered blend, then the reference's truncating denormalisation."""
    r = blend_accumulate_array(tiles, size, overlap)
    return np.clip((r + np.float32(1.0)) * np.float32(127.5), 0, 255).astype(np.uint8)


def frame_pad(length: int) -> int:
    """A side of `length` pixels as frame mode runs it: the next multiple of 8, at least 64."""
    if length <= 0:
        raise ValueError(f"length must be positive, got {length}")
    return max(64, -(-int(length) // 8) * 8)


def frame_load_array(rgb_u8: np.ndarray) -> np.ndarray:
    """uint8 [H,W,3] -> fp32 [3,Hp,Wp] in [-1,1], Hp / Wp = frame_pad(H / W); the edge is replicated into the padding."""
    h, w = _check_image(rgb_u8, "frame_load_array")
    px = rgb_u8[np.minimum(np.arange(frame_pad(h)), h - 1)][:, np.minimum(np.arange(frame_pad(w)), w - 1)]
    return np.ascontiguousarray((px.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(2, 0, 1))


def frame_store_array(x: np.ndarray, size: Tuple[int, int]) -> np.ndarray:
    """fp32 [3,Hp,Wp] -> uint8 [H,W,3]: the crop to `size`, then the reference's truncating denormalisation."""
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0 or x.ndim != 3 or tuple(x.shape) != (3, frame_pad(h), frame_pad(w)):
        raise ValueError(f"a {h}x{w} image is a frame [3,{frame_pad(max(h, 1))},{frame_pad(max(w, 1))}], got {tuple(x.shape)}")
    r = x.astype(np.float32, copy=False)[:, :h, :w].transpose(1, 2, 0)
    return np.clip((r + np.float32(1.0)) * np.float32(127.5), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ device wrappers
def _require_hip(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what} runs only on a HIP device (got '{where}'); there is no CPU fallback")


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _tile_total(h: int, w: int, tile: int, overlap: int) -> int:
    return len(tile_origins(h, tile, overlap)) * len(tile_origins(w, tile, overlap))


def _chunk(total: int, first: int, count: Optional[int]) -> int:
    count = total - first if count is None else count
    if first < 0 or count <= 0 or first + count > total:
        raise ValueError(f"tiles [{first}, {first + count}) lie outside the plan of {total} tiles")
    return count


def gather_tiles_device(rgb_u8: torch.Tensor, tile: int, overlap: int, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
    """Device twin of gather_tiles_array: uint8 [H,W,3] on a HIP device -> fp32 [count,3,S,S], tiles [first, first + count) of
    the plan (all of them by default)."""
    _require_hip(rgb_u8, "gather_tiles_device")
    h, w = _check_image(rgb_u8, "gather_tiles_device")
    count = _chunk(_tile_total(h, w, tile, overlap), first, count)
    img = rgb_u8.contiguous()
    out = torch.empty(count, 3, tile, tile, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        N.check(N.lib().llie_tile_gather_u8(img.data_ptr(), h, w, tile, overlap, first, count, out.data_ptr(), _stream(img.device)),
                "tile_gather_u8")
    return out


def gather_noise_device(canvas: torch.Tensor, size: Tuple[int, int], tile: int, overlap: int, first: int = 0,
                        count: Optional[int] = None) -> torch.Tensor:
    """fp32 canvas [steps,3,max(H,S),max(W,S)] on a HIP device -> [steps,count,3,S,S], the `noise=` of `enhance` for tiles
    [first, first + count) of an H x W image."""
    _require_hip(canvas, "gather_noise_device")
    h, w = int(size[0]), int(size[1])
    total = _tile_total(h, w, tile, overlap)
    if canvas.dtype != torch.float32 or canvas.dim() != 4 or tuple(canvas.shape[1:]) != (3, max(h, tile), max(w, tile)):
        raise ValueError(f"the noise canvas must be fp32 [steps,3,{max(h, tile)},{max(w, tile)}], got {canvas.dtype} {tuple(canvas.shape)}")
    count = _chunk(total, first, count)
    cv = canvas.contiguous()
    steps = cv.shape[0]
    out = torch.empty(steps, count, 3, tile, tile, dtype=torch.float32, device=cv.device)
    with torch.cuda.device(cv.device):
        N.check(N.lib().llie_tile_gather_f32(cv.data_ptr(), steps * 3, h, w, tile, overlap, first, count, out.data_ptr(), _stream(cv.device)),
                "tile_gather_f32")
    return out


def blend_tiles_device(tiles: torch.Tensor, size: Tuple[int, int], overlap: int) -> torch.Tensor:
    """Device twin of blend_tiles_array: fp32 [T,3,S,S] on a HIP device -> uint8 [H,W,3]."""
    _require_hip(tiles, "blend_tiles_device")
    h, w = int(size[0]), int(size[1])
    if tiles.dim() != 4 or tiles.shape[1] != 3 or tiles.shape[2] != tiles.shape[3]:
        raise ValueError(f"expected tiles [T,3,S,S], got {tuple(tiles.shape)}")
    s = tiles.shape[2]
    total = _tile_total(h, w, s, overlap)
    if tiles.shape[0] != total:
        raise ValueError(f"a {h}x{w} image has {total} tiles of side {s} at overlap {overlap}, got {tiles.shape[0]}")
    x = tiles.detach().float().contiguous()
    img = torch.empty(h, w, 3, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        N.check(N.lib().llie_tile_blend_u8(x.data_ptr(), h, w, s, overlap, img.data_ptr(), _stream(x.device)), "tile_blend_u8")
    return img


def frame_load_device(rgb_u8: torch.Tensor) -> torch.Tensor:
    """Device twin of frame_load_array: uint8 [H,W,3] on a HIP device -> fp32 [3,Hp,Wp]."""
    _require_hip(rgb_u8, "frame_load_device")
    h, w = _check_image(rgb_u8, "frame_load_device")
    img = rgb_u8.contiguous()
    out = torch.empty(3, frame_pad(h), frame_pad(w), dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        N.check(N.lib().llie_frame_load_u8(img.data_ptr(), h, w, out.data_ptr(), _stream(img.device)), "frame_load_u8")
    return out


def frame_store_device(x: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """Device twin of frame_store_array: fp32 [3,Hp,Wp] on a HIP device -> uint8 [H,W,3]."""
    _require_hip(x, "frame_store_device")
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0 or x.dim() != 3 or tuple(x.shape) != (3, frame_pad(h), frame_pad(w)):
        raise ValueError(f"a {h}x{w} image is a frame [3,{frame_pad(max(h, 1))},{frame_pad(max(w, 1))}], got {tuple(x.shape)}")
    x = x.detach().float().contiguous()
    img = torch.empty(h, w, 3, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        N.check(N.lib().llie_frame_store_u8(x.data_ptr(), h, w, img.data_ptr(), _stream(x.device)), "frame_store_u8")
    return img


# ------------------------------------------------------------------ the whole path
@torch.no_grad()
def enhance_frame_u8(model, rgb_u8: torch.Tensor, num_inference_steps: Optional[int] = None, *,
                     generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [H,W,3] on a HIP device -> enhanced uint8 [H,W,3] at the same resolution, by one run of the network at that size.

    The image is loaded into a frame [3,Hp,Wp] (Hp / Wp = frame_pad(H / W): the next multiple of 8, at least 64) with its edge
    replicated into the padding, goes through `model.enhance_frame` at B = 1, and is cropped and denormalised back.  Noise is
    drawn in `enhance`'s order at the frame's size; `noise=` supplies it as a canvas [steps,3,Hp,Wp] for a reproducible run.

    The replicated border is part of the frame the network sees: it takes part in the GroupNorm statistics (and in the global
    attention), so the result inside the image depends, slightly, on how much padding its size needs; an image whose sides are
    multiples of 8 and at least 64 has none.  Against `enhance_tiled` this gives the attention one field of view over the whole
    image and spends no work on overlaps; images past the engine's size cap (ValueError, naming it) remain with the tiles."""
    if not isinstance(rgb_u8, torch.Tensor):
        raise ValueError(f"enhance_frame_u8 expects a torch.Tensor, got {type(rgb_u8).__name__}")
    h, w = _check_image(rgb_u8, "enhance_frame_u8")
    _require_hip(rgb_u8, "enhance_frame_u8")
    hp, wp = frame_pad(h), frame_pad(w)
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or noise.dim() != 4 or tuple(noise.shape[1:]) != (3, hp, wp):
            raise ValueError(f"noise must be a canvas [steps,3,{hp},{wp}]")
        noise = noise.to(device=rgb_u8.device, dtype=torch.float32)[:, None]
    low = frame_load_device(rgb_u8)[None]
    out = model.enhance_frame(low, num_inference_steps, generator=generator, noise=noise)
    return frame_store_device(out[0], (h, w))



@torch.no_grad()
def enhance_tiled(model, rgb_u8: torch.Tensor, num_inference_steps: Optional[int] = None, *, overlap: Optional[int] = None,
                  tile_batch: int = 32, generator: Optional[torch.Generator] = None,
                  noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [H,W,3] on a HIP device -> enhanced uint8 [H,W,3] at the same resolution.

    The image is cut into S x S tiles (S = model.image_size) overlapping by `overlap` pixels (default S // 8, at most S // 2);
    `tile_batch` tiles at a time go through `model.enhance`; one launch blends all of them.  Noise is drawn once per image on a
    canvas [steps,3,max(H,S),max(W,S)] in `enhance`'s order (entry 0 with `generator`, the rest from the global generator) and
    every tile reads its window of it; `noise=` supplies the canvas for a reproducible run.

    Tiling removes the resize, not the model's field of view: each tile is denoised on its own (the global attention at the
    lowest level sees one tile), so brightness may drift between distant tiles; the shared canvas and the feathered blend keep
    neighbours consistent inside their overlap."""
    if not isinstance(rgb_u8, torch.Tensor):
        raise ValueError(f"enhance_tiled expects a torch.Tensor, got {type(rgb_u8).__name__}")
    h, w = _check_image(rgb_u8, "enhance_tiled")
    s = int(model.image_size)
    overlap = s // 8 if overlap is None else int(overlap)
    _check_plan(s, overlap)
    if tile_batch < 1:
        raise ValueError(f"tile_batch must be positive, got {tile_batch}")
    _require_hip(rgb_u8, "enhance_tiled")
    dev = rgb_u8.device
    nsteps = model.num_inference_steps if num_inference_steps is None else num_inference_steps
    model.scheduler.set_timesteps(nsteps, device=dev)
    steps = len(model.scheduler._timestep_list)
    hc, wc = max(h, s), max(w, s)
    if noise is None:
        canvas = torch.empty(steps, 3, hc, wc, dtype=torch.float32, device=dev)
        canvas[0].normal_(generator=generator)
        for i in range(1, steps):
            canvas[i].normal_()
    else:
        if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (steps, 3, hc, wc):
            raise ValueError(f"noise must be a canvas [{steps},3,{hc},{wc}]")
        canvas = noise.to(device=dev, dtype=torch.float32).contiguous()
    img = rgb_u8.contiguous()
    total = _tile_total(h, w, s, overlap)
    result = torch.empty(total, 3, s, s, dtype=torch.float32, device=dev)
    for first in range(0, total, tile_batch):
        count = min(tile_batch, total - first)
        low = gather_tiles_device(img, s, overlap, first, count)
        draws = gather_noise_device(canvas, (h, w), s, overlap, first, count)
        result[first:first + count].copy_(model.enhance(low, nsteps, noise=draws))
    return blend_tiles_device(result, (h, w), overlap)
