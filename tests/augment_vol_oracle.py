"""float64 numpy restatement of the volume augmentation contract (``biu_augment_vol_f32``, ``include/biu.h``) -- TEST INFRASTRUCTURE, next to
``tests/augment_f32_oracle.py``, whose Philox stream, samplers and ``source_coords`` it shares.

A record is read through its LOGICAL fields (``rot_k``, ``angle``, ``scale``, ``dx``, ``dy``, ``blur_k``, ``shot_s``, ``gauss_sigma``, ``alpha``,
``beta``) -- never through the matrix ``m`` or ``(cos_t, sin_t)``, which are what the kernel under test consumes.  The gathers and the blur are
pinned to ``scipy.ndimage`` by ``tests/test_augment_vol_host.py``.

Every stage takes ``dtype``: ``np.float64`` is the oracle; ``np.float32`` is the fp32 restatement of the same formulas that the GPU tests measure
against the oracle to derive their bounds.  Coordinates, weights and the interpolation itself are float64 in both, as the contract says; the
gathered value is then rounded to ``dtype``.

A field is ``[C, D, H, W]``; the element index of a voxel in the noise counter is ``((c D + z) H + y) W + x``.
"""
from __future__ import annotations

import numpy as np

from tests import augment_f32_oracle as FO

BLUR, SHOT, GAUSS, BC = FO.BLUR, FO.SHOT, FO.GAUSS, FO.BC
IMAGE, MASK, VECTOR = FO.IMAGE, FO.MASK, FO.VECTOR
REFLECT, CONSTANT = 0, 1
widen, source_coords = FO.widen, FO.source_coords


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    """``d c b | a b c d | c b a`` at any distance from the image."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def _take(f: np.ndarray, iy: np.ndarray, ix: np.ndarray, border: int) -> np.ndarray:
    """``f[..., iy, ix]`` under the border rule: reflected indices, or 0 for a tap outside the plane."""
    h, w = f.shape[-2:]
    if border == REFLECT:
        return f[..., reflect101(iy, h), reflect101(ix, w)]
    assert border == CONSTANT
    inside = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    return np.where(inside, f[..., np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)], f.dtype.type(0))


def gather_nearest(f: np.ndarray, sx, sy, border: int):
    """-> (``f`` gathered at ``floor(c + 0.5)``, ``safe``: the coordinate is farther than 1e-3 from a rounding boundary)."""
    ix, iy = np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64)
    dist = lambda a: np.abs(a - np.floor(a) - 0.5)
    return _take(f, iy, ix, border), (dist(sx) > 1e-3) & (dist(sy) > 1e-3)


def gather_bilinear(f: np.ndarray, sx, sy, border: int) -> np.ndarray:
    """float64; a tap outside the plane under CONSTANT reads 0 and keeps its weight."""
    g = f.astype(np.float64)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    v00, v01 = _take(g, y0, x0, border), _take(g, y0, x0 + 1, border)
    v10, v11 = _take(g, y0 + 1, x0, border), _take(g, y0 + 1, x0 + 1, border)
    top = v00 + ax * (v01 - v00)
    bot = v10 + ax * (v11 - v10)
    return top + ay * (bot - top)


def box_blur_reflect(g: np.ndarray, k: int, dtype=np.float64) -> np.ndarray:
    """``k x k`` box mean of the planes ``g [..., H, W]``; outside a plane lies its own reflect-101 (``cv2.blur``'s default border)."""
    h, w = g.shape[-2:]
    r = k // 2
    iy, ix = reflect101(np.arange(-r, h + r), h), reflect101(np.arange(-r, w + r), w)
    return FO.box_blur_gathered(g[..., iy[:, None], ix[None, :]], k, dtype)


def apply(field: np.ndarray, rec, kind: int, border: int, seed: int, epoch: int, field_id: int, dtype=np.float64, shot_counts: bool = False):
    """One sample's field ``[C, D, H, W]`` (float32 or uint8) through what the record ``rec`` describes -> (``[C, D, H, W]`` in ``dtype``,
    ``safe [H, W]``; all True where the gather is bilinear).  ``shot_counts``: stop behind the Poisson draw and return the counts."""
    f = widen(field)
    assert f.ndim == 4
    h, w = f.shape[-2:]
    flags = int(rec["flags"])
    geo = (int(rec["rot_k"]), float(rec["angle"]), float(rec["scale"]), float(rec["dx"]), float(rec["dy"]))
    sx, sy = source_coords(h, w, *geo)
    if kind != IMAGE:
        g, safe = gather_nearest(f, sx, sy, border)
        if kind == MASK:
            return g.astype(dtype), safe
        assert f.shape[0] % 2 == 0
        return FO.rotate_pairs(g, geo[0], geo[1], dtype), safe              # pairs are channels (2 j, 2 j + 1): axis 0
    g = gather_bilinear(f, sx, sy, border).astype(dtype)
    index = int(rec["index"])
    if flags & BC:
        g = FO.brightness_contrast(g, rec["alpha"], rec["beta"], dtype)
    if flags & BLUR:
        g = box_blur_reflect(g, int(rec["blur_k"]), dtype)
    every = np.ones((h, w), dtype=bool)
    if flags & SHOT:
        g = FO.shot_noise(g, rec["shot_s"], seed, index, epoch, field_id, dtype, counts=shot_counts)
        if shot_counts:
            return g, every
    if flags & GAUSS:
        g = FO.gauss_noise(g, rec["gauss_sigma"], seed, index, epoch, field_id, dtype)
    return g, every
