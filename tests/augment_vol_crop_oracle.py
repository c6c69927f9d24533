"""float64 numpy restatement of the whole-volume crop contract (``biu_augment_vol_f32_crop``, ``include/biu.h``) -- TEST INFRASTRUCTURE, built on
``tests/augment_vol_oracle.py`` (gathers, borders, blur) and ``tests/augment_f32_oracle.py`` (coordinates, Philox stream, samplers).

A record is read through its LOGICAL fields (``angle``, ``scale``, ``dx, dy`` = the crop origin ``(ox, oy)``, ``blur_k``, ``shot_s``,
``gauss_sigma``, ``alpha``, ``beta``) -- never through the matrix ``m`` or ``(cos_t, sin_t)``, which are what the kernel under test consumes.

It is literally the reference's order: shift-scale-rotate the WHOLE ``(h, w)`` plane of every channel and z-plane of the item about the plane's
centre, slice ``[z0:z0 + td, oy:oy + th, ox:ox + tw]`` (``RandomCrop3D``), then the intensity stages on the slice -- so the blur's border is the
reflect-101 of the slice and the noise element is the voxel's index in the slice.  NaN in a MASK or VECTOR item means "no label": the gathered
NaN becomes ``nan_to_val`` (VECTOR: in both planes of the pair when either is NaN, without rotation).  ``dtype=np.float32`` is the fp32
restatement the GPU tests derive their bounds from.  The gathers are pinned to ``scipy.ndimage`` by ``tests/test_augment_vol_crop_host.py``.
"""
from __future__ import annotations

import numpy as np

from tests import augment_f32_oracle as FO
from tests import augment_vol_oracle as VO

BLUR, SHOT, GAUSS, BC = VO.BLUR, VO.SHOT, VO.GAUSS, VO.BC
IMAGE, MASK, VECTOR = VO.IMAGE, VO.MASK, VO.VECTOR
REFLECT, CONSTANT = VO.REFLECT, VO.CONSTANT
widen = VO.widen


def plane_coords(rec, h: int, w: int):
    """float64 source coordinates ``(sx, sy) [h, w]`` of shift-scale-rotate applied to a whole ``(h, w)`` plane."""
    return FO.source_coords(h, w, 0, float(rec["angle"]), float(rec["scale"]), 0.0, 0.0)


def origin(rec):
    return int(rec["dx"]), int(rec["dy"])


def transform_whole(item: np.ndarray, rec, kind: int, border: int):
    """The item ``[C, D, H, W]`` (widened; NaN kept) with every plane transformed whole -> (``[C, D, H, W]`` float64 for IMAGE, the item's dtype
    otherwise, ``safe [H, W]``)."""
    f = widen(item)
    sx, sy = plane_coords(rec, *f.shape[-2:])
    if kind == IMAGE:
        return VO.gather_bilinear(f, sx, sy, border), np.ones(f.shape[-2:], dtype=bool)
    return VO.gather_nearest(f, sx, sy, border)


def apply(item: np.ndarray, rec, z0: int, tile, kind: int, border: int, nan_to_val: float, seed: int, epoch: int, field_id: int,
          dtype=np.float64, shot_counts: bool = False):
    """One patch ``[C, td, th, tw]`` in ``dtype`` out of the item ``[C, D, H, W]`` (float32 or uint8) -> (patch, ``safe [th, tw]``; all True
    where the gather is bilinear).  ``shot_counts``: stop behind the Poisson draw and return the counts."""
    assert item.ndim == 4
    td, th, tw = (int(v) for v in tile)
    ox, oy = origin(rec)
    assert 0 <= z0 and z0 + td <= item.shape[1]
    whole, safe = transform_whole(item[:, z0:z0 + td], rec, kind, border)
    g, safe = whole[..., oy:oy + th, ox:ox + tw], safe[oy:oy + th, ox:ox + tw]
    assert g.shape[1:] == (td, th, tw), "the crop leaves the transformed plane"
    if kind == MASK:
        return np.where(np.isnan(g), dtype(nan_to_val), g.astype(dtype)), safe
    if kind == VECTOR:
        assert g.shape[0] % 2 == 0
        none = np.repeat(np.isnan(g[0::2]) | np.isnan(g[1::2]), 2, axis=0)
        rot = FO.rotate_pairs(np.where(none, g.dtype.type(0), g), 0, float(rec["angle"]), dtype)
        return np.where(none, dtype(nan_to_val), rot), safe
    g = g.astype(dtype)
    flags, index = int(rec["flags"]), int(rec["index"])
    if flags & BC:
        g = FO.brightness_contrast(g, rec["alpha"], rec["beta"], dtype)
    if flags & BLUR:
        g = VO.box_blur_reflect(g, int(rec["blur_k"]), dtype)
    if flags & SHOT:
        g = FO.shot_noise(g, rec["shot_s"], seed, index, epoch, field_id, dtype, counts=shot_counts)
        if shot_counts:
            return g, safe
    if flags & GAUSS:
        g = FO.gauss_noise(g, rec["gauss_sigma"], seed, index, epoch, field_id, dtype)
    return g, safe
