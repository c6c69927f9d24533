"""float64 numpy restatement of the float augmentation contract (``biu_augment_f32``, ``include/biu.h``) -- TEST INFRASTRUCTURE, next to
``tests/augment_oracle.py``.

A record is read through its LOGICAL fields (``rot_k``, ``angle``, ``scale``, ``dx``, ``dy`` in pixels, ``blur_k``, ``shot_s``, ``gauss_sigma``,
``alpha``, ``beta``) -- never through the matrix ``m`` or ``(cos_t, sin_t)``, which are what the kernel under test consumes.  The geometric core
is pinned to the reference's own library call by ``tests/test_augment_f32_host.py`` (``scipy.ndimage.rotate(mode='grid-wrap')``).

Every stage takes ``dtype``: ``np.float64`` is the oracle; ``np.float32`` is the fp32 restatement of the same formulas (numpy's correctly
rounded ``log`` / ``cos`` / ``exp2``) that the GPU tests measure against the oracle to derive their bounds.  The geometry is float64 in both, as
the contract says.

A field is ``[P, H, W]``; the element index of a pixel in the noise counter is ``(p H + y) W + x``.
"""
from __future__ import annotations

import numpy as np

from tests.augment_oracle import philox4x32_10, uniform24

ROT, SCALE, BLUR, SHOT, GAUSS, BC = 1, 2, 4, 8, 16, 32
IMAGE, MASK, VECTOR = 0, 1, 2
STAGE_SHOT, STAGE_GAUSS = 3, 4
POISSON_CAP = 128


def widen(field: np.ndarray) -> np.ndarray:
    """The kernel's load: float32 as it is, uint8 as the correctly rounded fp32 quotient byte / 255 (``TileStore.__getitem__``'s value)."""
    f = np.asarray(field)
    if f.dtype == np.uint8:
        return f.astype(np.float32) / np.float32(255.0)
    assert f.dtype == np.float32
    return f


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def source_coords(h: int, w: int, rot_k: int, angle: float, scale: float, dx: float, dy: float, halo: int = 0):
    """float64 source coordinates ``(sx, sy)`` of the output pixels ``-halo .. h - 1 + halo`` x ``-halo .. w - 1 + halo`` for
    shift-scale-rotate applied to ``np.rot90(src, rot_k)``: rotation by ``angle`` degrees (scipy's sense: +90 equals ``np.rot90(x, 1)``) and
    scale about the tile centre, then a shift by ``(dx, dy)`` pixels; the quarter turns are then undone as an index permutation."""
    t = np.deg2rad(np.float64(angle))
    c, s = np.cos(t), np.sin(t)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    y, x = np.meshgrid(np.arange(-halo, h + halo, dtype=np.float64), np.arange(-halo, w + halo, dtype=np.float64), indexing="ij")
    u, v = x - cx - np.float64(dx), y - cy - np.float64(dy)
    gx, gy = (c * u - s * v) / np.float64(scale) + cx, (s * u + c * v) / np.float64(scale) + cy      # coordinates in rot90(src, rot_k)
    k = int(rot_k) % 4
    if k == 0:
        return gx, gy
    assert k == 2 or h == w
    if k == 1:                                   # rot90(src, 1)[y, x] = src[x, W - 1 - y]
        return (w - 1) - gy, gx
    if k == 2:
        return (w - 1) - gx, (h - 1) - gy
    return gy, (h - 1) - gx


def _nearest_index(sx, sy, h, w):
    ix, iy = np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64)
    dist = lambda a: np.abs(a - np.floor(a) - 0.5)
    return np.mod(iy, h), np.mod(ix, w), (dist(sx) > 1e-3) & (dist(sy) > 1e-3)


def gather_nearest(f: np.ndarray, sx, sy):
    """-> (``f`` gathered at ``floor(c + 0.5)`` with wrap-around indices, ``safe``: the coordinate is farther than 1e-3 from a rounding boundary)."""
    iy, ix, safe = _nearest_index(sx, sy, f.shape[-2], f.shape[-1])
    return f[..., iy, ix], safe


def gather_bilinear(f: np.ndarray, sx, sy) -> np.ndarray:
    h, w = f.shape[-2:]
    g = f.astype(np.float64)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = np.mod(x0, w), np.mod(x0 + 1, w), np.mod(y0, h), np.mod(y0 + 1, h)
    top = g[..., ya, xa] + ax * (g[..., ya, xb] - g[..., ya, xa])
    bot = g[..., yb, xa] + ax * (g[..., yb, xb] - g[..., yb, xa])
    return top + ay * (bot - top)


def rotate_pairs(g: np.ndarray, rot_k: int, angle: float, dtype=np.float64) -> np.ndarray:
    """``(c, s) -> (c cos t + s sin t, s cos t - c sin t)`` on plane pairs, ``t = rot_k pi / 2 + radians(angle)``: ``phi - t``.  Quarter
    turns swap and negate.  ``cos t`` and ``sin t`` are the fp32 numbers a record carries."""
    a = np.deg2rad(np.float64(angle))
    ca, sa = (np.cos(a), np.sin(a)) if angle != 0 else (1.0, 0.0)
    qc, qs = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(rot_k) % 4]
    ct, st = dtype(np.float32(qc * ca - qs * sa)), dtype(np.float32(qs * ca + qc * sa))
    g = g.astype(dtype)
    out = np.empty_like(g)
    c, s = g[0::2], g[1::2]
    out[0::2] = c * ct + s * st
    out[1::2] = s * ct - c * st
    return out


# ---- intensity stages -----------------------------------------------------------------------------------------------------------------
def box_blur_gathered(ext: np.ndarray, k: int, dtype=np.float64) -> np.ndarray:
    """``ext``: the gathered image with a halo of ``k // 2`` on every side -> ``k x k`` box mean: sums of k along x, then of k along y, times
    ``1 / k^2`` (the kernel's order; in float64 the order does not matter at the precision compared)."""
    e = ext.astype(dtype)
    h, w = e.shape[-2] - (k - 1), e.shape[-1] - (k - 1)
    rows = np.zeros(e.shape[:-1] + (w,), dtype=dtype)
    for d in range(k):
        rows = rows + e[..., :, d:d + w]
    acc = np.zeros(e.shape[:-2] + (h, w), dtype=dtype)
    for d in range(k):
        acc = acc + rows[..., d:d + h, :]
    return acc * (dtype(1.0) / dtype(k * k))


def stage_uniforms(n_elem: int, seed: int, index: int, epoch: int, field_id: int, stage: int):
    """``(u1, u2)`` of elements ``0 .. n_elem - 1`` as float64 (exact multiples of 2^-24): two neighbouring elements share a Philox block."""
    e = np.arange(n_elem, dtype=np.uint64)
    ctr = np.zeros((n_elem, 4), dtype=np.uint32)
    ctr[:, 0] = (e >> np.uint64(1)).astype(np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = index & 0xFFFFFFFF, epoch & 0xFFFFFFFF, (field_id * 16 + stage) & 0xFFFFFFFF
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    o = (e & np.uint64(1)).astype(np.int64) * 2
    rows = np.arange(n_elem)
    return uniform24(r[rows, o]), uniform24(r[rows, o + 1])


def normal(u1, u2, dtype=np.float64):
    u1, u2 = u1.astype(dtype), u2.astype(dtype)
    return np.sqrt(dtype(-2.0) * np.log(dtype(1.0) - u1)) * np.cos(dtype(2.0 * np.pi) * u2)


def poisson(lam, u1, u2, dtype=np.float64) -> np.ndarray:
    """The contract's sampler: ``lambda < 32``: inversion by sequential search with the one uniform ``u1``; otherwise the rounded normal
    approximation ``max(0, floor(lambda + sqrt(lambda) z + 0.5))``."""
    lam = np.asarray(lam, dtype=dtype)
    u1d = u1.astype(dtype)
    small = lam < dtype(32.0)
    # inversion
    ls = np.where(small, lam, dtype(1.0))
    p = np.exp(-ls)
    cdf = p.copy()
    k = np.zeros(lam.shape, dtype=np.int64)
    active = np.ones(lam.shape, dtype=bool)
    for _ in range(POISSON_CAP):
        active = active & (u1d >= cdf) & ((k.astype(dtype) < ls) | (p > dtype(2.0 ** -32)))
        if not active.any():
            break
        k = np.where(active, k + 1, k)
        p = np.where(active, p * (ls / np.maximum(k, 1).astype(dtype)), p)
        cdf = np.where(active, cdf + p, cdf)
    # normal approximation
    lb = np.where(small, dtype(32.0), lam)
    big = np.maximum(dtype(0.0), np.floor(lb + np.sqrt(lb) * normal(u1, u2, dtype) + dtype(0.5)))
    return np.where(small, k.astype(dtype), big)


def shot_noise(g, s, seed, index, epoch, field_id, dtype=np.float64, counts: bool = False):
    u1, u2 = (u.reshape(g.shape) for u in stage_uniforms(g.size, seed, index, epoch, field_id, STAGE_SHOT))
    g, s = g.astype(dtype), dtype(np.float32(s))
    with np.errstate(divide="ignore"):
        lin = np.exp2(dtype(np.float32(2.2)) * np.log2(g))
        n = poisson(lin / s, u1, u2, dtype)
        if counts:
            return n
        return np.exp2(np.log2(np.clip(n * s, dtype(0.0), dtype(1.0))) / dtype(np.float32(2.2)))


def gauss_noise(g, sigma, seed, index, epoch, field_id, dtype=np.float64):
    u1, u2 = (u.reshape(g.shape) for u in stage_uniforms(g.size, seed, index, epoch, field_id, STAGE_GAUSS))
    return np.clip(g.astype(dtype) + dtype(np.float32(sigma)) * normal(u1, u2, dtype), dtype(0.0), dtype(1.0))


def brightness_contrast(g, alpha, beta, dtype=np.float64):
    return np.clip(g.astype(dtype) * dtype(np.float32(alpha)) + dtype(np.float32(beta)), dtype(0.0), dtype(1.0))


# ---- one sample ----------------------------------------------------------------------------------------------------------------------
def apply(field: np.ndarray, rec, kind: int, seed: int, epoch: int, field_id: int, dtype=np.float64, shot_counts: bool = False):
    """One sample's field ``[P, H, W]`` (float32 or uint8) through what the record ``rec`` describes -> (``[P, H, W]`` in ``dtype``, ``safe [H, W]``;
    ``safe`` is all True where the gather is bilinear).  ``shot_counts``: stop behind the Poisson draw and return the counts."""
    f = widen(field)
    assert f.ndim == 3
    _, h, w = f.shape
    flags = int(rec["flags"])
    geo = (int(rec["rot_k"]), float(rec["angle"]), float(rec["scale"]), float(rec["dx"]), float(rec["dy"]))
    sx, sy = source_coords(h, w, *geo)
    if kind == MASK and flags & ROT:
        return gather_bilinear(f, sx, sy).astype(dtype), np.ones((h, w), dtype=bool)
    g, safe = gather_nearest(f, sx, sy)
    if kind == MASK:
        return g.astype(dtype), safe
    if kind == VECTOR:
        return rotate_pairs(g, geo[0], geo[1], dtype), safe
    g = g.astype(dtype)
    index = int(rec["index"])
    if flags & BLUR:
        k = int(rec["blur_k"])
        ex, ey = source_coords(h, w, *geo, halo=k // 2)
        g = box_blur_gathered(gather_nearest(f, ex, ey)[0], k, dtype)
    if flags & SHOT:
        g = shot_noise(g, rec["shot_s"], seed, index, epoch, field_id, dtype, counts=shot_counts)
        if shot_counts:
            return g, safe
    if flags & GAUSS:
        g = gauss_noise(g, rec["gauss_sigma"], seed, index, epoch, field_id, dtype)
    if flags & BC:
        g = brightness_contrast(g, rec["alpha"], rec["beta"], dtype)
    return g, safe
