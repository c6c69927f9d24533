"""float64 numpy restatement of the crop augmentation contract (``biu_augment_f32_crop``, ``include/biu.h``) -- TEST INFRASTRUCTURE, next to
``tests/augment_f32_oracle.py``, whose noise stages, blur and pair rotation it reuses.

A record is read through its LOGICAL fields (``rot_k``, ``angle``, ``scale``, the crop origin ``dx``, ``dy``, ``blur_k``, ``shot_s``, ``gauss_sigma``,
``alpha``, ``beta``) -- never through the matrix ``m`` or ``(cos_t, sin_t)``, which are what the kernel under test consumes.  The geometry and the
NaN rule are pinned to ``scipy.ndimage.rotate(mode='grid-wrap')`` and to a restated ``rotate_array`` by ``tests/test_augment_crop_host.py``.

An item is ``[P, h, w]``, a rendered tile ``[P, th, tw]``; the element index of a tile pixel in the noise counter is ``(p th + y) tw + x``.

The chain from a tile pixel ``(x, y)`` to the item, every step in float64:

1. crop origin:       ``X = x + ox``, ``Y = y + oy``: a pixel of the turned, rotated and scaled item;
2. scale:             about pixel centres, ``gx = (X + 0.5) / scale - 0.5``;
3. rotation:          by ``angle`` degrees (scipy's sense) about the centre of the TURNED item (``w x h`` for an odd ``rot_k``);
4. quarter turn:      ``np.rot90(item, rot_k)[gy, gx]`` as an index permutation into the item;

then every index wraps in the item's own ``(h, w)``.
"""
from __future__ import annotations

import numpy as np

from tests import augment_f32_oracle as FO

ROT, SCALE, BLUR, SHOT, GAUSS, BC = FO.ROT, FO.SCALE, FO.BLUR, FO.SHOT, FO.GAUSS, FO.BC
IMAGE, MASK, VECTOR = FO.IMAGE, FO.MASK, FO.VECTOR
TIE = 1e-6                                  # |w_nan - 0.5| below this: the NaN decision is not compared


def source_coords(item_hw, tile_hw, rot_k: int, angle: float, scale: float, ox: float, oy: float, halo: int = 0):
    """float64 item coordinates ``(sx, sy)`` of the tile pixels ``-halo .. th - 1 + halo`` x ``-halo .. tw - 1 + halo`` (module docstring)."""
    h, w = item_hw
    th, tw = tile_hw
    k = int(rot_k) % 4
    ht, wt = (w, h) if k % 2 else (h, w)
    y, x = np.meshgrid(np.arange(-halo, th + halo, dtype=np.float64), np.arange(-halo, tw + halo, dtype=np.float64), indexing="ij")
    s = np.float64(scale)
    gx, gy = (x + np.float64(ox) + 0.5) / s - 0.5, (y + np.float64(oy) + 0.5) / s - 0.5
    if angle != 0:
        t = np.deg2rad(np.float64(angle))
        c, sn = np.cos(t), np.sin(t)
        cx, cy = (wt - 1) / 2.0, (ht - 1) / 2.0
        u, v = gx - cx, gy - cy
        gx, gy = c * u - sn * v + cx, sn * u + c * v + cy
    if k == 0:
        return gx, gy
    if k == 1:                                   # rot90(item, 1)[y, x] = item[x, w - 1 - y]
        return (w - 1) - gy, gx
    if k == 2:
        return (w - 1) - gx, (h - 1) - gy
    return gy, (h - 1) - gx                      # rot90(item, 3)[y, x] = item[h - 1 - x, y]


def gather_bilinear_nan(f: np.ndarray, sx, sy):
    """-> (the bilinear value of the taps with NaN read as 0, ``w_nan``: the weight the NaN taps carry), both float64, per plane."""
    h, w = f.shape[-2:]
    g = f.astype(np.float64)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = np.mod(x0, w), np.mod(x0 + 1, w), np.mod(y0, h), np.mod(y0 + 1, h)
    taps = [(g[..., ya, xa], (1 - ax) * (1 - ay)), (g[..., ya, xb], ax * (1 - ay)), (g[..., yb, xa], (1 - ax) * ay), (g[..., yb, xb], ax * ay)]
    w_nan = sum(np.where(np.isnan(t), wt, 0.0) for t, wt in taps)
    z = [np.where(np.isnan(t), 0.0, t) for t, _ in taps]
    top = z[0] + ax * (z[1] - z[0])
    bot = z[2] + ax * (z[3] - z[2])
    return top + ay * (bot - top), w_nan


def geometry_of(rec):
    return int(rec["rot_k"]), float(rec["angle"]), float(rec["scale"]), float(rec["dx"]), float(rec["dy"])


def apply(item: np.ndarray, rec, kind: int, tile_hw, nan_to_val: float, seed: int, epoch: int, field_id: int, dtype=np.float64,
          shot_counts: bool = False):
    """One patch ``[P, th, tw]`` in ``dtype`` out of the item ``[P, h, w]`` (float32, NaN allowed in MASK and VECTOR items, or uint8) as the
    record ``rec`` describes it -> ``(patch, safe [P, th, tw] or [th, tw])``.  ``safe``: for nearest gathers the coordinate is farther than
    1e-3 from a rounding tie; for the bilinear MASK gather ``|w_nan - 0.5| > TIE`` (per plane).  ``shot_counts``: stop behind the Poisson
    draw and return the counts."""
    f = FO.widen(item)
    assert f.ndim == 3
    flags = int(rec["flags"])
    geo = geometry_of(rec)
    nv = dtype(np.float32(nan_to_val))
    sx, sy = source_coords(f.shape[1:], tile_hw, *geo)
    if kind == MASK and flags & ROT:
        val, w_nan = gather_bilinear_nan(f, sx, sy)
        return np.where(w_nan >= 0.5, nv, val.astype(dtype)), np.abs(w_nan - 0.5) > TIE
    g, safe = FO.gather_nearest(f, sx, sy)
    if kind == MASK:
        return np.where(np.isnan(g), nv, g.astype(dtype)), safe
    if kind == VECTOR:
        gone = np.repeat(np.isnan(g[0::2]) | np.isnan(g[1::2]), 2, axis=0)
        return np.where(gone, nv, FO.rotate_pairs(np.where(gone, np.float32(0), g), geo[0], geo[1], dtype)), safe
    g = g.astype(dtype)
    index = int(rec["index"])
    if flags & BLUR:
        k = int(rec["blur_k"])
        ex, ey = source_coords(f.shape[1:], tile_hw, *geo, halo=k // 2)
        g = FO.box_blur_gathered(FO.gather_nearest(f, ex, ey)[0], k, dtype)
    if flags & SHOT:
        g = FO.shot_noise(g, rec["shot_s"], seed, index, epoch, field_id, dtype, counts=shot_counts)
        if shot_counts:
            return g, safe
    if flags & GAUSS:
        g = FO.gauss_noise(g, rec["gauss_sigma"], seed, index, epoch, field_id, dtype)
    if flags & BC:
        g = FO.brightness_contrast(g, rec["alpha"], rec["beta"], dtype)
    return g, safe


def window_safe(item_hw, tile_hw, rec):
    """[th, tw] bool: every pixel of the blur window (1 x 1 without blur) of a tile pixel was gathered away from a rounding tie."""
    k = int(rec["blur_k"]) if int(rec["flags"]) & BLUR else 1
    ex, ey = source_coords(item_hw, tile_hw, *geometry_of(rec), halo=k // 2)
    safe = FO._nearest_index(ex, ey, item_hw[0], item_hw[1])[2]
    th, tw = tile_hw
    ok = np.ones((th, tw), dtype=bool)
    for dy in range(k):
        for dx in range(k):
            ok &= safe[dy:dy + th, dx:dx + tw]
    return ok


def rotate_array_restated(x: np.ndarray, angle: float, order: int = 1) -> np.ndarray:
    """The reference's rule for carrying NaN through a rotation, restated (without its final clip, which does not touch NaN): rotate the
    zero-filled array; rotate the uint8 NaN mask with the same order and test ``> 0.5``; put NaN back where the test holds."""
    from scipy.ndimage import rotate
    nan = np.isnan(x)
    out = rotate(np.where(nan, 0, x), angle, reshape=False, mode="grid-wrap", order=order).astype(np.float64)
    out[rotate(nan.astype(np.uint8), angle, reshape=False, mode="grid-wrap", order=order) > 0.5] = np.nan
    return out
