"""Full-resolution enhancement: an image of any size is cut into overlapping SH x SW tiles, the tiles go through the network as
batches, and the overlaps are blended with a feathered window.  By default the tile is S x S (S = model.image_size) and runs
through `LowLightDiffusion.enhance`; `enhance_tiled(tile=(TH, TW))` takes any frame the engine accepts and runs it through
`enhance_frame`, and `tile="auto"` picks the fewest such tiles (`auto_tile_plan`).

One definition serves the NumPy twins here, the kernels (csrc/tiles.hip) and the tests.  Each axis has its own tile side and
overlap: rows use (H, SH, vy), columns (W, SW, vx).  Wherever a function takes `tile` / `overlap`, an int means that value on
both axes and a pair means (rows, columns); below S and v stand for one axis's pair:

  plan, per axis of length L, overlap v (0 <= v <= S/2): one tile at origin 0 if L <= S, else n = ceil((L - S) / (S - v)) + 1
      tiles at o_i = floor(i (L - S) / (n - 1)); tiles of an image are numbered row-major, t = iy * nx + ix
  gather   tile[t][c][y][x] = float(img[min(oy + y, H-1)][min(ox + x, W-1)][c]) / 127.5f - 1.0f,  tiles [T][3][SH][SW]
  noise    one canvas [steps][3][max(H,SH)][max(W,SW)] per image; tile t reads canvas[k][c][oy + y][ox + x], so overlapping
           tiles denoise the same noise where they overlap
  window   w[k] = min(k + 1, S - k, v) / v   (1 if v == 0), per axis: wy from (SH, vy), wx from (SW, vx)
  blend    per pixel and channel over the covering tiles in ascending t: g = wy[Y - oy] * wx[X - ox]; num += val * g; den += g
           (separate fp32 multiply and add); out = uint8(trunc(clip((num / den + 1) * 127.5, 0, 255)))

  auto plan (`auto_tile_plan(size, max_pixels)`), per axis of length L cut into n tiles:
      T_1 = frame_pad(L);  T_n = frame_pad(ceil(8 L / (7 n + 1))) for n >= 2;  v_n = T_n // 8
      -- the smallest frame-legal tile side for which n tiles overlapping by an eighth cover the axis.  Among all (ny, nx) with
      TH * TW <= max_pixels: the smallest ny * nx, then the smallest max(TH, TW), then the smallest ny.

`enhance_tiled(sync="latents")` ties the tiles together at every step instead of once at the end: one latent canvas per image,
and the tiles' predictions are fused into it after each step (a MultiDiffusion-style loop).  With Hc = max(H,SH), Wc = max(W,SW)
-- the plan of (Hc, Wc) is the plan of (H, W), and its tiles cover the canvas exactly -- and the noise canvas [steps,3,Hc,Wc]
in `enhance`'s order (entry 0 the initial latents, entry k+1 the re-noising draw of step k):

  X = canvas[0]                                     # latent canvas, fp32 [3,Hc,Wc]
  for k, t in enumerate(timesteps):
      lat[j] = X[:, oy_j:oy_j+SH, ox_j:ox_j+SW]      # every tile j
      eps[j] = unet(lat[j], low[j], t)               # low[j] from gather, as above
      for every canvas pixel (Y, X) and channel c:   # sync step (tile_sync_step_kernel, csrc/tiles.hip)
          over the covering tiles in ascending j:  g = wy[Y-oy]*wx[X-ox];  num = num + eps*g;  den = den + g
          e  = eps of the one tile, if exactly one tile covers the pixel;  else num / den
          x0 = (x - sb*e) / sa  (epsilon)  |  sa*x - sb*e  (v);  clip to [-1,1] if clamp_x0;  p = x0 if is_last else sap*x0 + sbp*noise,
               with x = X[c][Y][X], noise = canvas[k+1][c][Y][X] and the scalars of `scheduler.step_coefficients(t)`: lcm_step_kernel
          X[c][Y][X] = p
          sampler="ddim" (coef.sampler == 1; ddim.py): no noise canvas past entry 0, and the predicted noise takes the draw's place,
               p = x0 if is_last else sap*x0 + sbp*z,  z = e (epsilon)  |  sa*e + sb*x (v);  not defined together with clamp_x0
  out[y][x][c] = uint8(trunc(clip((X[c][y][x] + 1) * 127.5, 0, 255)))  for y < H, x < W    # after the last step

Every multiply and add is a separate fp32 operation, in the order written.  A pixel under exactly one tile skips the weights and
so goes through lcm_step_kernel's arithmetic unchanged.  Blending eps rather than x0 is the same mathematics: x0 is affine in
eps, and all covering tiles share x at a pixel.

Frame mode (`enhance_frame_u8`) is the other route for images under the engine's size cap: no tiles, the network runs once at
the image's own size (`LowLightDiffusion.enhance_frame`), padded to sides the network takes:

  pad      frame_pad(L) = max(64, 8 * ceil(L / 8))
  load     out[c][y][x] = float(img[min(y, H-1)][min(x, W-1)][c]) / 127.5f - 1.0f   for y < frame_pad(H), x < frame_pad(W)
  store    img[y][x][c] = uint8(trunc(clip((x[c][y][x] + 1) * 127.5, 0, 255)))      for y < H, x < W

The device functions are bit-exact with the host twins.  There is no CPU fallback for `enhance_tiled` or `enhance_frame_u8`.
"""
from __future__ import annotations

import weakref
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _native as N
from .ddim import check_sampler
from .guidance import guidance_is_on, guided_keyword as _guided_kw


def _check_plan(tile: int, overlap: int) -> None:
    if tile <= 0:
        raise ValueError(f"tile side must be positive, got {tile}")
    if overlap < 0 or 2 * overlap > tile:
        raise ValueError(f"overlap must lie in 0..{tile // 2} (half the tile side {tile}), got {overlap}")


def _pair(value, what: str) -> Tuple[int, int]:
    """An int (both axes) or a pair (rows, columns) -> (rows, columns)."""
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError(f"{what} is an int or a pair (rows, columns), got {value!r}")
        return int(value[0]), int(value[1])
    return int(value), int(value)


def _plan(tile, overlap) -> Tuple[int, int, int, int]:
    """(SH, SW, vy, vx) of `tile` / `overlap` given as ints or pairs, each axis checked."""
    (sh, sw), (vy, vx) = _pair(tile, "tile"), _pair(overlap, "overlap")
    _check_plan(sh, vy)
    _check_plan(sw, vx)
    return sh, sw, vy, vx


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
def gather_tiles_array(rgb_u8: np.ndarray, tile, overlap) -> np.ndarray:
    """uint8 [H,W,3] -> fp32 [T,3,SH,SW] in [-1,1], T = ny * nx tiles in row-major order."""
    h, w = _check_image(rgb_u8, "gather_tiles_array")
    sh, sw, vy, vx = _plan(tile, overlap)
    oys, oxs = tile_origins(h, sh, vy), tile_origins(w, sw, vx)
    out = np.empty((len(oys) * len(oxs), 3, sh, sw), dtype=np.float32)
    ky, kx = np.arange(sh), np.arange(sw)
    for iy, oy in enumerate(oys):
        rows = rgb_u8[np.minimum(oy + ky, h - 1)]
        for ix, ox in enumerate(oxs):
            px = rows[:, np.minimum(ox + kx, w - 1)]
            out[iy * len(oxs) + ix] = (px.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(2, 0, 1)
    return out


def _tiles_plan(shape, size, overlap, what: str = "tiles") -> Tuple[int, int, int, int, int, int]:
    """(H, W, SH, SW, vy, vx) of a tile tensor [T,3,SH,SW] holding every tile of an H x W image."""
    h, w = int(size[0]), int(size[1])
    if len(shape) != 4 or shape[1] != 3:
        raise ValueError(f"expected {what} [T,3,SH,SW], got {tuple(shape)}")
    sh, sw, vy, vx = _plan((shape[2], shape[3]), overlap)
    total = _tile_total(h, w, (sh, sw), (vy, vx))
    if shape[0] != total:
        raise ValueError(f"a {h}x{w} image has {total} tiles of {sh}x{sw} at overlap ({vy}, {vx}), got {shape[0]}")
    return h, w, sh, sw, vy, vx


def blend_accumulate_array(tiles: np.ndarray, size: Tuple[int, int], overlap) -> np.ndarray:
    """fp32 [T,3,SH,SW] -> fp32 [H,W,3]: the blended image num / den before denormalisation (tile by tile, ascending t)."""
    h, w, sh, sw, vy, vx = _tiles_plan(tiles.shape, size, overlap)
    oys, oxs = tile_origins(h, sh, vy), tile_origins(w, sw, vx)
    tiles = tiles.astype(np.float32, copy=False)
    wy, wx = tile_window(sh, vy), tile_window(sw, vx)
    num = np.zeros((h, w, 3), dtype=np.float32)
    den = np.zeros((h, w), dtype=np.float32)
    for iy, oy in enumerate(oys):
        th = min(sh, h - oy)  # < SH only where the image is smaller than a tile: the replicated rest is dropped
        for ix, ox in enumerate(oxs):
            tw = min(sw, w - ox)
            g = wy[:th, None] * wx[None, :tw]
            val = tiles[iy * len(oxs) + ix, :, :th, :tw].transpose(1, 2, 0)
            num[oy:oy + th, ox:ox + tw] = num[oy:oy + th, ox:ox + tw] + val * g[:, :, None]
            den[oy:oy + th, ox:ox + tw] = den[oy:oy + th, ox:ox + tw] + g
    return num / den[:, :, None]


def blend_tiles_array(tiles: np.ndarray, size: Tuple[int, int], overlap) -> np.ndarray:
    """fp32 [T,3,SH,SW] -> uint8 [H,W,3]: feathered blend, then the reference's truncating denormalisation."""
    r = blend_accumulate_array(tiles, size, overlap)
    return np.clip((r + np.float32(1.0)) * np.float32(127.5), 0, 255).astype(np.uint8)


def frame_pad(length: int) -> int:
    """A side of `length` pixels as frame mode runs it: the next multiple of 8, at least 64."""
    if length <= 0:
        raise ValueError(f"length must be positive, got {length}")
    return max(64, -(-int(length) // 8) * 8)


def auto_tile_plan(size: Tuple[int, int], max_pixels: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """The fewest frame-legal tiles of at most `max_pixels` pixels that cover an H x W image at an overlap of one eighth:
    -> ((TH, TW), (vy, vx)), the `tile` / `overlap` of `enhance_tiled`.  Pure host arithmetic (module docstring): per axis
    T_1 = frame_pad(L), T_n = frame_pad(ceil(8 L / (7 n + 1))), v_n = T_n // 8, so n tiles of T_n always cover L and 2 v_n <= T_n;
    among the (ny, nx) whose tile fits, the smallest ny * nx, then the smallest max(TH, TW), then the smallest ny.  ValueError when
    not even a 64 x 64 tile fits."""
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0:
        raise ValueError(f"auto_tile_plan expects a positive image size, got {h}x{w}")
    max_pixels = int(max_pixels)
    if max_pixels < 64 * 64:
        raise ValueError(f"max_pixels = {max_pixels} is below the smallest frame, 64 x 64 = 4096 pixels")

    def sides(length: int) -> List[int]:  # T_n for n = 1, 2, ... down to the first 64: more tiles make none smaller
        out = [frame_pad(length)]
        while out[-1] > 64:
            out.append(frame_pad(-(-8 * length // (7 * (len(out) + 1) + 1))))
        return out

    best = None
    for ny, th in enumerate(sides(h), 1):
        for nx, tw in enumerate(sides(w), 1):
            if th * tw <= max_pixels:
                key = (ny * nx, max(th, tw), ny)
                if best is None or key < best[0]:
                    best = (key, th, tw)
                break  # a larger nx at this ny only adds tiles
    _, th, tw = best  # the 64 x 64 corner always fits
    return (th, tw), (th // 8, tw // 8)


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


def _step_scalars(coef):
    """The fp32 scalars and flags of one N.StepCoef, as the kernels get them."""
    f = np.float32
    return (f(coef.sqrt_alpha_t), f(coef.sqrt_beta_t), f(coef.sqrt_alpha_prev), f(coef.sqrt_beta_prev), bool(coef.is_last),
            bool(coef.v_prediction), bool(coef.clamp_x0), int(coef.sampler))


def _check_sync_shapes(eps_shape, size, overlap, canvas_shape, noise_shape) -> Tuple[int, int, int, int, int, int]:
    h, w, sh, sw, vy, vx = _tiles_plan(eps_shape, size, overlap, "eps tiles")
    want = (3, max(h, sh), max(w, sw))
    if tuple(canvas_shape) != want or (noise_shape is not None and tuple(noise_shape) != want):
        raise ValueError(f"the latent canvas and the noise of a {h}x{w} image are [3,{want[1]},{want[2]}], got {tuple(canvas_shape)}"
                         + ("" if noise_shape is None else f" and {tuple(noise_shape)}"))
    return h, w, sh, sw, vy, vx


def sync_step_array(eps_tiles: np.ndarray, size: Tuple[int, int], overlap, canvas: np.ndarray, noise: Optional[np.ndarray],
                    coef) -> np.ndarray:
    """One step of the shared latent canvas (module docstring): eps tiles fp32 [T,3,SH,SW], canvas and noise fp32 [3,Hc,Wc], `coef`
    an N.StepCoef -> the new canvas.  `noise` may be None on the last step, and on every step of the DDIM sampler (coef.sampler
    == 1), which reads none."""
    h, w, sh, sw, vy, vx = _check_sync_shapes(eps_tiles.shape, size, overlap, canvas.shape, None if noise is None else noise.shape)
    sa, sb, sap, sbp, last, vpred, clamp, sampler = _step_scalars(coef)
    if sampler not in (N.SAMPLER_LCM, N.SAMPLER_DDIM) or (sampler == N.SAMPLER_DDIM and clamp):
        raise ValueError("coef.sampler is 0 (LCM) or 1 (DDIM), and the DDIM step is not defined together with clamp_x0")
    if not last and not sampler and noise is None:
        raise ValueError("a step that is not the last needs its noise")
    hc, wc = canvas.shape[1:]
    oys, oxs = tile_origins(h, sh, vy), tile_origins(w, sw, vx)
    eps_tiles = eps_tiles.astype(np.float32, copy=False)
    g = tile_window(sh, vy)[:, None] * tile_window(sw, vx)[None, :]
    num, one = np.zeros((3, hc, wc), dtype=np.float32), np.zeros((3, hc, wc), dtype=np.float32)
    den, cover = np.zeros((hc, wc), dtype=np.float32), np.zeros((hc, wc), dtype=np.int32)
    for iy, oy in enumerate(oys):
        for ix, ox in enumerate(oxs):  # ascending tile number
            e = eps_tiles[iy * len(oxs) + ix]
            num[:, oy:oy + sh, ox:ox + sw] = num[:, oy:oy + sh, ox:ox + sw] + e * g
            den[oy:oy + sh, ox:ox + sw] = den[oy:oy + sh, ox:ox + sw] + g
            one[:, oy:oy + sh, ox:ox + sw] = e
            cover[oy:oy + sh, ox:ox + sw] += 1
    e = np.where(cover == 1, one, num / den)
    x = canvas.astype(np.float32, copy=False)
    x0 = sa * x - sb * e if vpred else (x - sb * e) / sa
    if clamp:
        x0 = np.minimum(np.maximum(x0, np.float32(-1.0)), np.float32(1.0))
    if last:
        return x0
    if sampler == N.SAMPLER_DDIM:
        return sap * x0 + sbp * (sa * e + sb * x if vpred else e)
    return sap * x0 + sbp * noise.astype(np.float32, copy=False)


def canvas_store_array(x: np.ndarray, size: Tuple[int, int]) -> np.ndarray:
    """fp32 canvas [3,Hc,Wc] -> uint8 [H,W,3]: the crop to `size`, then the reference's truncating denormalisation."""
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0 or x.ndim != 3 or x.shape[0] != 3 or x.shape[1] < h or x.shape[2] < w:
        raise ValueError(f"a {h}x{w} image needs a canvas [3,>={h},>={w}], got {tuple(x.shape)}")
    r = x.astype(np.float32, copy=False)[:, :h, :w].transpose(1, 2, 0)
    return np.clip((r + np.float32(1.0)) * np.float32(127.5), 0, 255).astype(np.uint8)


def enhance_tiled_sync_array(eps_fn, rgb_u8: np.ndarray, tile, overlap, coefs, timesteps, canvas: np.ndarray, *,
                             sampler: str = "lcm"):
    """The loop of `enhance_tiled(sync="latents")` on the host, the denoiser passed in: eps_fn(lat [T,3,SH,SW], low [T,3,SH,SW], t)
    -> fp32 [T,3,SH,SW].  `coefs[k]` is the N.StepCoef of `timesteps[k]`; `canvas` is the noise canvas [steps,3,Hc,Wc], or
    [1,3,Hc,Wc] with sampler="ddim" (the initial latents; `coefs` are then DDIM coefficients).
    -> (uint8 [H,W,3], the final fp32 canvas [3,Hc,Wc] before any clamp)."""
    h, w = _check_image(rgb_u8, "enhance_tiled_sync_array")
    sh, sw, vy, vx = _plan(tile, overlap)
    hc, wc = max(h, sh), max(w, sw)
    ddim = check_sampler(sampler) == "ddim"
    if sampler == "dpmpp_2m":
        raise ValueError('the shared-canvas loop is defined for sampler="lcm" and "ddim": its step keeps no history of x0 for "dpmpp_2m"')
    if any(int(c.sampler) != int(ddim) for c in coefs):
        raise ValueError(f'sampler="{sampler}" needs coefficients of that sampler on every step')
    draws = 1 if ddim else len(timesteps)
    if canvas.ndim != 4 or tuple(canvas.shape) != (draws, 3, hc, wc) or len(coefs) != len(timesteps):
        raise ValueError(f"{len(timesteps)} {sampler} steps of a {h}x{w} image need a canvas [{draws},3,{hc},{wc}] and "
                         f"{len(timesteps)} coefficients")
    low = gather_tiles_array(rgb_u8, (sh, sw), (vy, vx))
    origins = [(oy, ox) for oy in tile_origins(h, sh, vy) for ox in tile_origins(w, sw, vx)]
    x = canvas[0].astype(np.float32)
    for k, t in enumerate(timesteps):
        lat = np.stack([x[:, oy:oy + sh, ox:ox + sw] for oy, ox in origins])
        eps = np.asarray(eps_fn(lat, low, int(t)), dtype=np.float32)
        x = sync_step_array(eps, (h, w), (vy, vx), x, None if coefs[k].is_last or ddim else canvas[k + 1], coefs[k])
    return canvas_store_array(x, (h, w)), x


# ------------------------------------------------------------------ device wrappers
def _require_hip(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what} runs only on a HIP device (got '{where}'); there is no CPU fallback")


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _tile_total(h: int, w: int, tile, overlap) -> int:
    sh, sw, vy, vx = _plan(tile, overlap)
    return len(tile_origins(h, sh, vy)) * len(tile_origins(w, sw, vx))


def _chunk(total: int, first: int, count: Optional[int]) -> int:
    count = total - first if count is None else count
    if first < 0 or count <= 0 or first + count > total:
        raise ValueError(f"tiles [{first}, {first + count}) lie outside the plan of {total} tiles")
    return count


def gather_tiles_device(rgb_u8: torch.Tensor, tile, overlap, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
    """Device twin of gather_tiles_array: uint8 [H,W,3] on a HIP device -> fp32 [count,3,SH,SW], tiles [first, first + count) of
    the plan (all of them by default)."""
    sh, sw, vy, vx = _plan(tile, overlap)
    _require_hip(rgb_u8, "gather_tiles_device")
    h, w = _check_image(rgb_u8, "gather_tiles_device")
    count = _chunk(_tile_total(h, w, (sh, sw), (vy, vx)), first, count)
    img = rgb_u8.contiguous()
    out = torch.empty(count, 3, sh, sw, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        N.check(N.lib().llie_tile_gather_u8_hw(img.data_ptr(), h, w, sh, sw, vy, vx, first, count, out.data_ptr(),
                                               _stream(img.device)), "tile_gather_u8")
    return out


def gather_noise_device(canvas: torch.Tensor, size: Tuple[int, int], tile, overlap, first: int = 0,
                        count: Optional[int] = None) -> torch.Tensor:
    """fp32 canvas [steps,3,max(H,SH),max(W,SW)] on a HIP device -> [steps,count,3,SH,SW], the `noise=` of `enhance` /
    `enhance_frame` for tiles [first, first + count) of an H x W image."""
    sh, sw, vy, vx = _plan(tile, overlap)
    _require_hip(canvas, "gather_noise_device")
    h, w = int(size[0]), int(size[1])
    total = _tile_total(h, w, (sh, sw), (vy, vx))
    if canvas.dtype != torch.float32 or canvas.dim() != 4 or tuple(canvas.shape[1:]) != (3, max(h, sh), max(w, sw)):
        raise ValueError(f"the noise canvas must be fp32 [steps,3,{max(h, sh)},{max(w, sw)}], got {canvas.dtype} {tuple(canvas.shape)}")
    count = _chunk(total, first, count)
    cv = canvas.contiguous()
    steps = cv.shape[0]
    out = torch.empty(steps, count, 3, sh, sw, dtype=torch.float32, device=cv.device)
    with torch.cuda.device(cv.device):
        N.check(N.lib().llie_tile_gather_f32_hw(cv.data_ptr(), steps * 3, h, w, sh, sw, vy, vx, first, count, out.data_ptr(),
                                                _stream(cv.device)), "tile_gather_f32")
    return out


def blend_tiles_device(tiles: torch.Tensor, size: Tuple[int, int], overlap) -> torch.Tensor:
    """Device twin of blend_tiles_array: fp32 [T,3,SH,SW] on a HIP device -> uint8 [H,W,3]."""
    h, w, sh, sw, vy, vx = _tiles_plan(getattr(tiles, "shape", ()), size, overlap)
    _require_hip(tiles, "blend_tiles_device")
    x = tiles.detach().float().contiguous()
    img = torch.empty(h, w, 3, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        N.check(N.lib().llie_tile_blend_u8_hw(x.data_ptr(), h, w, sh, sw, vy, vx, img.data_ptr(), _stream(x.device)), "tile_blend_u8")
    return img


def sync_step_device(eps_tiles: torch.Tensor, size: Tuple[int, int], overlap, canvas: torch.Tensor, noise: Optional[torch.Tensor],
                     coef, *, out: Optional[torch.Tensor] = None, image: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device twin of sync_step_array: contiguous fp32 eps tiles [T,3,SH,SW], canvas and noise [3,Hc,Wc] on a HIP device -> the
    new canvas, written to `out` (a fresh tensor by default; `out=canvas` steps in place).  `image` (uint8 [H,W,3], contiguous)
    also takes the bytes of the new canvas, which is what the last step wants."""
    _require_hip(eps_tiles, "sync_step_device")
    h, w, sh, sw, vy, vx = _check_sync_shapes(eps_tiles.shape, size, overlap, canvas.shape, None if noise is None else noise.shape)
    out = torch.empty_like(canvas) if out is None else out
    for name, t in (("eps_tiles", eps_tiles), ("canvas", canvas), ("noise", noise), ("out", out)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != eps_tiles.device):
            raise ValueError(f"{name} must be a contiguous fp32 tensor on {eps_tiles.device}")
    if out.shape != canvas.shape:
        raise ValueError(f"out must have the canvas's shape {tuple(canvas.shape)}, got {tuple(out.shape)}")
    if image is not None and (image.dtype != torch.uint8 or tuple(image.shape) != (h, w, 3) or not image.is_contiguous()
                              or image.device != eps_tiles.device):
        raise ValueError(f"image must be a contiguous uint8 [{h},{w},3] tensor on {eps_tiles.device}")
    dev = eps_tiles.device
    with torch.cuda.device(dev):
        N.check(N.lib().llie_tile_sync_step_hw(eps_tiles.data_ptr(), h, w, sh, sw, vy, vx, canvas.data_ptr(),
                                               None if noise is None else noise.data_ptr(), coef, out.data_ptr(),
                                               None if image is None else image.data_ptr(), _stream(dev)), "tile_sync_step")
    return out


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
                     generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None,
                     sampler: str = "lcm", guidance_scale: Optional[float] = None,
                     guidance_rescale: Optional[float] = None) -> torch.Tensor:
    """uint8 [H,W,3] on a HIP device -> enhanced uint8 [H,W,3] at the same resolution, by one run of the network at that size.
    `sampler` is `enhance`'s: with "ddim" and "dpmpp_2m" the noise canvas is [1,3,Hp,Wp], the initial latents.  `guidance_scale` is `enhance`'s
    too (classifier-free guidance; None: off), and so is `guidance_rescale` (its statistic is taken over the padded frame).

    The image is loaded into a frame [3,Hp,Wp] (Hp / Wp = frame_pad(H / W): the next multiple of 8, at least 64) with its edge
    replicated into the padding, goes through `model.enhance_frame` at B = 1, and is cropped and denormalised back.  Noise is
    drawn in `enhance`'s order at the frame's size; `noise=` supplies it as a canvas [steps,3,Hp,Wp] for a reproducible run.

    The replicated border is part of the frame the network sees: it takes part in the GroupNorm statistics (and in the global
    attention), so the result inside the image depends, slightly, on how much padding its size needs; an image whose sides are
    multiples of 8 and at least 64 has none.  Against `enhance_tiled` this gives the attention one field of view over the whole
    image and spends no work on overlaps; images past the engine's size cap (ValueError, naming it) remain with the tiles:
    `enhance_tiled(tile="auto")` cuts them into the fewest frames under the cap."""
    if not isinstance(rgb_u8, torch.Tensor):
        raise ValueError(f"enhance_frame_u8 expects a torch.Tensor, got {type(rgb_u8).__name__}")
    check_sampler(sampler)
    guided = _guided_kw(guidance_scale, guidance_rescale)
    h, w = _check_image(rgb_u8, "enhance_frame_u8")
    _require_hip(rgb_u8, "enhance_frame_u8")
    hp, wp = frame_pad(h), frame_pad(w)
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or noise.dim() != 4 or tuple(noise.shape[1:]) != (3, hp, wp):
            raise ValueError(f"noise must be a canvas [steps,3,{hp},{wp}]")
        noise = noise.to(device=rgb_u8.device, dtype=torch.float32)[:, None]
    low = frame_load_device(rgb_u8)[None]
    out = model.enhance_frame(low, num_inference_steps, generator=generator, noise=noise, sampler=sampler, **guided)
    return frame_store_device(out[0], (h, w))




_RULE_HANDLES = weakref.WeakKeyDictionary()  # model -> its device-less context (not on the model: a deepcopy must not meet it)


def _frame_rule_handle(model) -> "N.Handle":
    """A device-less context of the model's network: it answers the host-only questions of the frame rule (llie_frame_shape_ok,
    llie_frame_max_pixels) without loading weights or touching a device."""
    h = _RULE_HANDLES.get(model)
    if h is None:
        h = _RULE_HANDLES[model] = N.Handle(model.unet._make_cfg(N.LLIE_F32))
    return h


def parse_tile_size(text: str):
    """The CLI's --tile_size: "auto", or "HxW" -> (H, W).  ValueError for anything else."""
    if text == "auto":
        return "auto"
    parts = str(text).lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError(f'--tile_size is "auto" or HxW (two positive integers, e.g. 1080x1920), got {text!r}')
    return int(parts[0]), int(parts[1])


def resolve_tile_plan(model, size: Tuple[int, int], tile=None, overlap=None, max_tile_pixels: Optional[int] = None):
    """(SH, SW, vy, vx) of `enhance_tiled`'s `tile` / `overlap` / `max_tile_pixels` for an H x W image: the checks and defaults of
    its docstring, on the host (no device is looked at)."""
    h, w = int(size[0]), int(size[1])
    s = int(model.image_size)
    frames = tile is not None
    if max_tile_pixels is not None and tile != "auto":
        raise ValueError('max_tile_pixels bounds the plan of tile="auto"; it has no meaning with any other tile')
    if isinstance(tile, str):
        if tile != "auto":
            raise ValueError(f'tile must be None, (TH, TW) or "auto", got {tile!r}')
        if overlap is not None:
            raise ValueError('tile="auto" chooses the overlap (an eighth of each tile side); do not pass overlap= with it')
        budget = _frame_rule_handle(model).frame_max_pixels(1)
        if max_tile_pixels is not None:
            budget = min(budget, int(max_tile_pixels))
        tile, overlap = auto_tile_plan((h, w), budget)
    if frames:
        sh, sw = _pair(tile, "tile")
        if sh < 64 or sw < 64 or sh % 8 or sw % 8:
            raise ValueError(f"tile {sh}x{sw}: a tile is a frame of the network, its height and width multiples of 8 and at least 64")
        vy, vx = (sh // 8, sw // 8) if overlap is None else _pair(overlap, "overlap")
    else:
        sh = sw = s
        vy = vx = s // 8 if overlap is None else int(overlap)
    _check_plan(sh, vy)
    _check_plan(sw, vx)
    return sh, sw, vy, vx


@torch.no_grad()
def enhance_tiled(model, rgb_u8: torch.Tensor, num_inference_steps: Optional[int] = None, *, overlap=None,
                  tile_batch: int = 32, generator: Optional[torch.Generator] = None,
                  noise: Optional[torch.Tensor] = None, sync: str = "none", return_canvas: bool = False, sampler: str = "lcm",
                  tile=None, max_tile_pixels: Optional[int] = None, guidance_scale: Optional[float] = None,
                  guidance_rescale: Optional[float] = None):
    """uint8 [H,W,3] on a HIP device -> enhanced uint8 [H,W,3] at the same resolution.

    The image is cut into S x S tiles (S = model.image_size) overlapping by `overlap` pixels (default S // 8, at most S // 2);
    `tile_batch` tiles at a time go through `model.enhance`; one launch blends all of them.  Noise is drawn once per image on a
    canvas [steps,3,max(H,S),max(W,S)] in `enhance`'s order (entry 0 with `generator`, the rest from the global generator) and
    every tile reads its window of it; `noise=` supplies the canvas for a reproducible run.

    Tiling removes the resize, not the model's field of view: each tile is denoised on its own (the global attention at the
    lowest level sees one tile), so brightness may drift between distant tiles; the shared canvas and the feathered blend keep
    neighbours consistent inside their overlap.

    sync="latents" couples the tiles at every step instead (the module docstring has the definition): the image keeps one latent
    canvas, every step denoises each tile's window of it (`tile_batch` tiles per `unet.forward_split`) and one launch fuses the
    predictions back into the canvas, so neighbours start every step from the same values where they overlap and the result is
    single-valued before any blending of pixels.  The attention is still per tile: only overlaps couple neighbours.  The noise
    canvas is read the same way; `return_canvas=True` returns (image, the final fp32 canvas [3,max(H,S),max(W,S)] before the clamp).

    sampler="ddim" runs the deterministic DDIM loop of `enhance` in either `sync` mode: any step count in 1..num_train_timesteps,
    and the canvas is [1,3,max(H,S),max(W,S)] -- the initial latents, drawn with `generator`; nothing else is drawn.
    sampler="dpmpp_2m" (DPM-Solver++ 2M, dpm.py) takes the same canvas and runs with sync="none" only: every tile's `enhance` /
    `enhance_frame` call keeps its own history; with sync="latents" it is a ValueError (the shared-canvas step keeps none).

    tile=(TH, TW) makes the tiles frames of that size instead of S x S squares: any frame the engine accepts (sides multiples of
    8 and at least 64, under the element cap; ValueError naming the rule otherwise, before anything is drawn or launched).  The
    tiles run through `model.enhance_frame` (`forward_split(frame=True)` with sync="latents"), `overlap` is an int or (vy, vx)
    and defaults to (TH // 8, TW // 8), and the canvases above are [..,3,max(H,TH),max(W,TW)].  Large tiles give the attention and
    the normalisation statistics a large field of view and spend less work on overlaps.  `tile_batch` is lowered to the largest
    batch of such frames the engine takes in one call; the result does not depend on it.  tile=(S, S) is tile=None, to the byte.
    tile="auto" plans the fewest tiles the engine can run (`auto_tile_plan` with the budget llie_frame_max_pixels, lowered to
    `max_tile_pixels` when that is given -- a bound on memory); it chooses the overlap, so `overlap=` with it is a ValueError.  An
    image under the cap becomes one tile: `enhance_frame_u8`'s result.

    guidance_scale=w (classifier-free guidance, `enhance`'s keyword) passes through to every tile's `enhance` / `enhance_frame`
    call with sync="none"; with sync="latents" a scale other than None / 1.0 is a ValueError (the shared-canvas loop has no
    guided form).  `guidance_rescale=phi` passes through with it.  The rescale's standard deviations are those of one network
    call, so with tiles they are taken per tile, not over the image: two tiles of one image may be scaled by different factors
    (the blend over the overlaps hides the seam, as it does for the tiles' separate GroupNorm statistics); an image that fits one
    frame has one statistic."""
    if not isinstance(rgb_u8, torch.Tensor):
        raise ValueError(f"enhance_tiled expects a torch.Tensor, got {type(rgb_u8).__name__}")
    if sync not in ("none", "latents"):
        raise ValueError(f'sync must be "none" or "latents", got {sync!r}')
    ddim = check_sampler(sampler) == "ddim"
    dpm = sampler == "dpmpp_2m"
    guided = _guided_kw(guidance_scale, guidance_rescale)
    if sync == "latents" and dpm:
        raise ValueError('enhance_tiled(sync="latents", sampler="dpmpp_2m") is not provided: the shared-canvas step keeps no history of '
                         'x0; use sync="none", or sampler="ddim"')
    if sync == "latents" and guidance_is_on(guidance_scale):
        raise ValueError('enhance_tiled(sync="latents", guidance_scale=...) is not provided: guidance runs with sync="none" only')
    if return_canvas and sync != "latents":
        raise ValueError('return_canvas needs sync="latents": the default path keeps no latent canvas')
    h, w = _check_image(rgb_u8, "enhance_tiled")
    frames = tile is not None  # tiles are frames of their own size, run by enhance_frame / forward_split(frame=True)
    sh, sw, vy, vx = resolve_tile_plan(model, (h, w), tile, overlap, max_tile_pixels)
    if tile_batch < 1:
        raise ValueError(f"tile_batch must be positive, got {tile_batch}")
    total = _tile_total(h, w, (sh, sw), (vy, vx))
    if frames:
        rule = _frame_rule_handle(model)
        try:
            rule.frame_shape_ok(1, sh, sw)
        except ValueError as e:
            raise ValueError(f'enhance_tiled: tile {sh}x{sw}: {e}; tile="auto" plans tiles under the cap') from None
        # the largest batch of such frames one call takes (the element cap counts the batch; 65535 frames per call)
        tile_batch = max(1, min(tile_batch, total, rule.frame_max_pixels(1) // (sh * sw), 65535))
    _require_hip(rgb_u8, "enhance_tiled")
    dev = rgb_u8.device
    nsteps = model.num_inference_steps if num_inference_steps is None else num_inference_steps
    if ddim:
        schedule = model.ddim_schedule(nsteps)
        steps = 1  # entries of the noise canvas: the initial latents
    elif dpm:
        model.dpm_schedule(nsteps)  # the schedule's ValueErrors, before anything is drawn; each tile's call builds its own
        schedule, steps = None, 1
    else:
        model.scheduler.set_timesteps(nsteps, device=dev)
        ts = model.scheduler._timestep_list
        schedule = (ts, [model.scheduler.step_coefficients(t) for t in ts]) if sync == "latents" else None
        steps = len(ts)
    hc, wc = max(h, sh), max(w, sw)
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
    plan = ((sh, sw), (vy, vx))
    if sync == "latents":
        out, x = _enhance_tiled_sync(model, img, plan, tile_batch, canvas, total, schedule, frames)
        return (out, x) if return_canvas else out
    run = model.enhance_frame if frames else model.enhance
    result = torch.empty(total, 3, sh, sw, dtype=torch.float32, device=dev)
    for first in range(0, total, tile_batch):
        count = min(tile_batch, total - first)
        low = gather_tiles_device(img, *plan, first, count)
        draws = gather_noise_device(canvas, (h, w), *plan, first, count)
        result[first:first + count].copy_(run(low, nsteps, noise=draws, sampler=sampler, **guided))
    return blend_tiles_device(result, (h, w), plan[1])


def _enhance_tiled_sync(model, img: torch.Tensor, plan, tile_batch: int, canvas: torch.Tensor, total: int, schedule, frames: bool = False):
    """The loop of enhance_tiled(sync="latents") after its checks: `plan` is ((SH, SW), (vy, vx)), `canvas` the noise canvas,
    `schedule` the (timesteps, coefficients) of the sampler; `frames`: the tiles are frames (forward_split(frame=True)).  Nothing
    inside the loop waits for the device or copies from the host."""
    (sh, sw), overlap = plan
    h, w = int(img.shape[0]), int(img.shape[1])
    dev = img.device
    ts, coefs = schedule
    t_dev = {}  # (timestep, count) -> device int64 [count], kept on the model like enhance's
    for t in ts:
        for count in {min(tile_batch, total), total % tile_batch} - {0}:
            key = ("tiles", int(t), count, dev.type, dev.index)
            cached = model._t_cache.get(key)
            if cached is None:
                if len(model._t_cache) > 64:
                    model._t_cache.clear()
                cached = model._t_cache[key] = torch.full((count,), int(t), dtype=torch.long).to(dev)
            t_dev[int(t), count] = cached
    x = canvas[0].clone()  # the latent canvas; `canvas` may be the caller's
    eps = torch.empty(total, 3, sh, sw, dtype=torch.float32, device=dev)
    out = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
    for k, t in enumerate(ts):
        for first in range(0, total, tile_batch):
            count = min(tile_batch, total - first)
            low = gather_tiles_device(img, (sh, sw), overlap, first, count)
            lat = gather_noise_device(x[None], (h, w), (sh, sw), overlap, first, count)[0]
            model.unet.forward_split(lat, low, t_dev[int(t), count], uniform_t=True, out=eps[first:first + count], frame=frames)
        last = bool(coefs[k].is_last)
        draw = None if last or coefs[k].sampler else canvas[k + 1]  # the DDIM step reads no noise
        sync_step_device(eps, (h, w), overlap, x, draw, coefs[k], out=x, image=out if last else None)
    return out, x
