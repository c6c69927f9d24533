"""float64 numpy restatement of the cubic-spline MASK path (``biu_spline_prefilter_f32`` + ``biu_augment_f32_cubic``, ``include/biu.h``) --
TEST INFRASTRUCTURE, next to ``tests/augment_f32_oracle.py``, whose geometry it uses unchanged.

``scipy.ndimage.rotate(order=3, mode='grid-wrap')`` is a prefilter and an interpolation.  With ``grid-wrap`` scipy does not pre-pad, so the
prefilter along an axis of length ``n`` is the cyclic convolution ``c[k] = sum_j sqrt(3) z^|j| s[(k - j) mod n]`` over all integers ``j``,
``z = sqrt(3) - 2``; the interpolation sums 4 x 4 coefficients with the cubic B-spline's weights and wrapped indices.
``tests/test_augment_cubic_host.py`` pins both to scipy's own calls.

``dtype=np.float64`` is the oracle (the exact periodic sum); ``dtype=np.float32`` is the fp32 restatement of what the kernels are asked to do
-- the sum cut at ``|j| <= R`` with fp32 taps, the kernel's order of additions, fp32 weights and sums -- which the GPU tests measure against
the oracle to derive their bounds.  The geometry is float64 in both, as the contract says.
"""
from __future__ import annotations

import numpy as np

from tests import augment_f32_oracle as FO

R = 16                                   # include/biu.h: BIU_SPLINE_R
POLE = np.sqrt(3.0) - 2.0
GAIN = np.sqrt(3.0)                      # 6 (-z) / (1 - z^2): scipy's gain of 6 per axis on the two-sided exponential


def _periodic_matrix(n: int) -> np.ndarray:
    """``C[k, i]`` = the sum of ``sqrt(3) z^|j|`` over all ``j = k - i (mod n)``: ``sqrt(3) (z^m + z^(n - m)) / (1 - z^n)``, ``m = (k - i) mod n``."""
    m = np.mod(np.arange(n)[:, None] - np.arange(n)[None, :], n).astype(np.float64)
    return GAIN * (POLE ** m + POLE ** (n - m)) / (1.0 - POLE ** n)


def prefilter_periodic(f: np.ndarray, dtype=np.float64) -> np.ndarray:
    """Coefficients of the periodic cubic B-spline through ``f [..., H, W]``: the exact cyclic sum, in float64, along x, then along y."""
    g = np.asarray(f, dtype=np.float64)
    g = g @ _periodic_matrix(g.shape[-1]).T
    g = np.swapaxes(np.swapaxes(g, -1, -2) @ _periodic_matrix(g.shape[-2]).T, -1, -2)
    return g.astype(dtype)


def _truncated_axis(g: np.ndarray, r: int, dtype) -> np.ndarray:
    """Along the last axis: ``s[k - d] + s[k + d]`` first, terms added from ``d = r`` inwards, the centre tap last (the kernel's order)."""
    n = g.shape[-1]
    k = np.arange(n)
    taps = [dtype(GAIN * POLE ** d) for d in range(r + 1)]
    acc = np.zeros(g.shape, dtype=dtype)
    for d in range(r, 0, -1):
        acc = acc + taps[d] * (g[..., np.mod(k - d, n)] + g[..., np.mod(k + d, n)])
    return acc + taps[0] * g


def prefilter_truncated(f: np.ndarray, r: int = R, dtype=np.float64) -> np.ndarray:
    """The same sum cut at ``|j| <= r`` (indices still wrap as often as needed), taps, products and sums in ``dtype``; x, then y."""
    g = _truncated_axis(np.asarray(f).astype(dtype), r, dtype)
    return np.swapaxes(_truncated_axis(np.swapaxes(g, -1, -2), r, dtype), -1, -2)


def _weights(t: np.ndarray, dtype):
    """Cubic B-spline weights of the taps ``floor(c) - 1 .. floor(c) + 2`` at the fraction ``t``: float64, rounded once to ``dtype``."""
    return [((1.0 - t) ** 3 / 6.0).astype(dtype), ((3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0).astype(dtype),
            ((-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0).astype(dtype), (t ** 3 / 6.0).astype(dtype)]


def gather_cubic(c: np.ndarray, sx, sy, dtype=np.float64) -> np.ndarray:
    """``c [..., H, W]`` coefficients -> the spline at ``(sx, sy)``: 4 x 4 coefficients with wrapped indices, rows first, sums in ``dtype``."""
    h, w = c.shape[-2:]
    c = c.astype(dtype)
    x0, y0 = np.floor(sx), np.floor(sy)
    wx, wy = _weights(sx - x0, dtype), _weights(sy - y0, dtype)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    out = np.zeros(c.shape[:-2] + sx.shape, dtype=dtype)
    for i in range(4):
        yi = np.mod(y0 - 1 + i, h)
        row = wx[0] * c[..., yi, np.mod(x0 - 1, w)]
        for j in range(1, 4):
            row = row + wx[j] * c[..., yi, np.mod(x0 - 1 + j, w)]
        out = out + wy[i] * row
    return out


def clip_range(f: np.ndarray):
    """The reference's rule over the whole target array, NaN aside: ``(lo, hi)`` to clip the rotated result to if ``lo >= 0`` and ``hi <= 1``
    (a bool array counts as [0, 1]), else None: no clip."""
    f = np.asarray(f)
    if f.dtype == bool:
        return 0.0, 1.0
    lo, hi = float(np.nanmin(f)), float(np.nanmax(f))
    return (lo, hi) if lo >= 0.0 and hi <= 1.0 else None


def apply_mask_cubic(field: np.ndarray, rec, dtype=np.float64):
    """One sample's MASK field ``[P, H, W]`` (float32 or uint8) through what the record ``rec`` describes, read through its logical fields as
    ``FO.apply`` does -> (``[P, H, W]`` in ``dtype``, ``safe [H, W]``).  Under an arbitrary angle: the cubic spline and the clip (``safe`` is all
    True: the interpolant is continuous); otherwise ``FO.apply``'s nearest gather."""
    if not int(rec["flags"]) & FO.ROT:
        return FO.apply(field, rec, FO.MASK, 0, 0, 0, dtype=dtype)
    f = FO.widen(field)
    assert f.ndim == 3
    _, h, w = f.shape
    sx, sy = FO.source_coords(h, w, int(rec["rot_k"]), float(rec["angle"]), float(rec["scale"]), float(rec["dx"]), float(rec["dy"]))
    c = prefilter_periodic(f) if dtype == np.float64 else prefilter_truncated(f, R, dtype)
    g = gather_cubic(c, sx, sy, dtype)
    rng = clip_range(f)
    if rng is not None:
        g = np.clip(g, dtype(rng[0]), dtype(rng[1]))
    return g, np.ones((h, w), dtype=bool)
