"""float64 numpy restatement of the cubic-spline crop contract (``biu_spline_prefilter_items`` + ``biu_augment_f32_crop_cubic``,
``include/biu.h``) -- TEST INFRASTRUCTURE.  It is made of ``tests/augment_crop_oracle.py`` (the chain from a tile pixel to the item, read
through the record's LOGICAL fields, never through ``m``) and ``tests/augment_cubic_oracle.py`` (the periodic prefilter, its truncated fp32
restatement, the 4 x 4 gather, the reference's clip rule); ``tests/test_augment_crop_cubic_host.py`` pins it to scipy and to the restated
``rotate_array`` at ``order=3``.

The rule (``multi_output_unet/data.py:213-242``): the spline through the item with NaN read as 0; the same spline through ``isnan(item)`` as
0 / 1, ``w_nan``; ``nan_to_val`` where ``w_nan >= 0.5`` (scipy rounds the rotated uint8 indicator half up before the reference's ``> 0.5``);
elsewhere the value, clipped to the item's own ``[nanmin, nanmax]`` over all planes iff that range lies in [0, 1].

``dtype=np.float64`` is the oracle (exact periodic prefilter); ``dtype=np.float32`` restates what the kernels are asked to do (sum cut at
``R``, fp32 taps, weights and sums, the kernel's order); the geometry is float64 in both.
"""
from __future__ import annotations

import numpy as np

from tests import augment_crop_oracle as CO
from tests import augment_cubic_oracle as QO
from tests import augment_f32_oracle as FO

TIE = CO.TIE


def item_range(item: np.ndarray):
    """``(lo, hi)`` of the loaded values over all planes, NaN aside, as float32 -- the table's row; nothing but NaN: ``(+inf, -inf)``."""
    f = FO.widen(item)
    if np.isnan(f).all():
        return np.float32(np.inf), np.float32(-np.inf)
    return np.float32(np.nanmin(f)), np.float32(np.nanmax(f))


def coefficients(item: np.ndarray, dtype=np.float64):
    """-> (value coefficients of the zero-filled item, indicator coefficients of ``isnan(item)``), both ``[P, h, w]`` in ``dtype``."""
    f = FO.widen(item)
    nan = np.isnan(f)
    pre = QO.prefilter_periodic if dtype == np.float64 else (lambda a: QO.prefilter_truncated(a, QO.R, dtype))
    return pre(np.where(nan, np.float32(0), f)), pre(nan.astype(np.float32))


def apply(item: np.ndarray, rec, tile_hw, nan_to_val: float, dtype=np.float64):
    """One patch ``[P, th, tw]`` in ``dtype`` of the MASK item ``[P, h, w]`` (float32 with NaN, or uint8) -> ``(patch, safe, w_nan)``, all
    ``[P, th, tw]``.  ``safe``: ``|w_nan - 0.5| > TIE`` under an arbitrary angle; off a rounding tie for the nearest gather of the other
    records, whose ``w_nan`` is the 0 / 1 indicator of the gathered pixel."""
    f = FO.widen(item)
    assert f.ndim == 3
    nv = dtype(np.float32(nan_to_val))
    if not int(rec["flags"]) & CO.ROT:
        patch, safe = CO.apply(item, rec, CO.MASK, tile_hw, nan_to_val, 0, 0, 0, dtype=dtype)
        sx, sy = CO.source_coords(f.shape[1:], tile_hw, *CO.geometry_of(rec))
        w_nan = np.isnan(FO.gather_nearest(f, sx, sy)[0]).astype(dtype)
        return patch, np.broadcast_to(safe, patch.shape), w_nan
    sx, sy = CO.source_coords(f.shape[1:], tile_hw, *CO.geometry_of(rec))
    cv, ci = coefficients(item, dtype)
    val, w_nan = QO.gather_cubic(cv, sx, sy, dtype), QO.gather_cubic(ci, sx, sy, dtype)
    if not np.isnan(f).all():
        rng = QO.clip_range(f)
        if rng is not None:
            val = np.clip(val, dtype(rng[0]), dtype(rng[1]))
    return np.where(w_nan >= 0.5, nv, val), np.abs(w_nan.astype(np.float64) - 0.5) > TIE, w_nan


def reference_rotate_array(x: np.ndarray, angle: float) -> np.ndarray:
    """The reference's ``rotate_array(x, angle, order=3)`` restated in float64: ``CO.rotate_array_restated`` followed by its clip."""
    out = CO.rotate_array_restated(x, angle, order=3)
    if not np.isnan(x).all() and np.nanmin(x) >= 0 and np.nanmax(x) <= 1:
        out = np.clip(out, np.nanmin(x), np.nanmax(x))                              # NaN stays NaN
    return out
