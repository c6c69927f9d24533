"""float64 numpy restatement of the on-device augmentation contract -- TEST INFRASTRUCTURE (next to ``tests/mo2d_oracle.py``).

albumentations and OpenCV cannot be run here, so this file restates the WRITTEN contract (``bio_image_unet_amd/augment.py``'s docstring,
``include/biu.h``), stage by stage, from a parameter record's logical fields (``rot_k``, ``angle``, ``scale``, ``dx``, ``dy``, ``alpha``,
``beta``, ``blur_k``, ``noise_a``, ``noise_b``) -- never from the record's matrix ``m``, which is what the kernel under test consumes.

Sign convention (fixed by ``tests/test_augment_host.py``): the forward map of ``shift_scale_rotate`` is
``x' = s (cos t (x - cx) + sin t (y - cy)) + cx + dx W``, ``y' = s (-sin t (x - cx) + cos t (y - cy)) + cy + dy H``; with it a rotation
by +90 degrees of a square tile equals ``np.rot90(x, 1)`` and -90 degrees ``np.rot90(x, 3)``.

A field is ``[P, H, W]`` uint8 (P channels or z-planes); the element index of a pixel in the noise counter is ``(p H + y) W + x``.
"""
from __future__ import annotations

import numpy as np

GATE, SSR, BC, BLUR, MULT, GAUSS = 1, 2, 4, 8, 16, 32
ORDER_UNET, ORDER_SIAM = 0, 1
STAGE_MULT, STAGE_GAUSS = 1, 2


# ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter: np.ndarray, key) -> np.ndarray:
    """``counter``: ``[..., 4]`` uint32, ``key``: two uint32 -> ``[..., 4]`` uint32 (Random123's Philox4x32 with ten rounds)."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform24(u32: np.ndarray) -> np.ndarray:
    return (np.asarray(u32, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def noise_words(n_elem: int, per_block: int, seed: int, index: int, epoch: int, field_id: int, stage: int) -> np.ndarray:
    """The raw words of elements ``0 .. n_elem - 1``: ``per_block`` neighbouring elements share one Philox block (4 for mult_noise: one
    word each; 2 for gauss_noise: two words each).  Returns ``[n_elem, 4 // per_block]`` uint32."""
    e = np.arange(n_elem, dtype=np.uint64)
    ctr = np.zeros((n_elem, 4), dtype=np.uint32)
    ctr[:, 0] = (e // np.uint64(per_block)).astype(np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = index & 0xFFFFFFFF, epoch & 0xFFFFFFFF, (field_id * 16 + stage) & 0xFFFFFFFF
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    wpe = 4 // per_block
    col = (e % np.uint64(per_block)).astype(np.int64)[:, None] * wpe + np.arange(wpe)[None, :]
    return np.take_along_axis(r, col, axis=1)


# ---- stages ---------------------------------------------------------------------------------------------------------------------------
def quant8(v: np.ndarray) -> np.ndarray:
    return np.rint(np.clip(v, 0.0, 255.0))                      # np.rint rounds half to even


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def source_coords(h: int, w: int, angle: float, scale: float, dx: float, dy: float):
    """float64 source coordinates ``(sx, sy)``, each ``[H, W]``, of every output pixel: the inverse of the forward map."""
    t = np.deg2rad(np.float64(angle))
    c, s = np.cos(t), np.sin(t)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u, v = x - cx - np.float64(dx) * w, y - cy - np.float64(dy) * h
    return (c * u - s * v) / np.float64(scale) + cx, (s * u + c * v) / np.float64(scale) + cy


def shift_scale_rotate(f: np.ndarray, angle, scale, dx, dy, mask: bool):
    """-> (float64 ``[P, H, W]`` already rounded, ``safe`` ``[H, W]`` bool: the source coordinate is farther than 1e-3 from a rounding
    boundary in both axes -- where a nearest-neighbour gather in another precision must agree)."""
    _, h, w = f.shape
    sx, sy = source_coords(h, w, angle, scale, dx, dy)
    g = f.astype(np.float64)
    if mask:
        ix, iy = np.rint(sx).astype(np.int64), np.rint(sy).astype(np.int64)
        dist = lambda a: np.abs(a - np.floor(a) - 0.5)
        return g[:, reflect101(iy, h), reflect101(ix, w)], (dist(sx) > 1e-3) & (dist(sy) > 1e-3)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = reflect101(x0, w), reflect101(x0 + 1, w), reflect101(y0, h), reflect101(y0 + 1, h)
    top = g[:, ya, xa] * (1 - ax) + g[:, ya, xb] * ax
    bot = g[:, yb, xa] * (1 - ax) + g[:, yb, xb] * ax
    return quant8(top * (1 - ay) + bot * ay), np.ones((h, w), dtype=bool)


def brightness_contrast(g: np.ndarray, alpha, beta255) -> np.ndarray:
    return quant8(g * np.float64(alpha) + np.float64(beta255))


def box_blur(g: np.ndarray, k: int) -> np.ndarray:
    r = k // 2
    pad = np.pad(g, ((0, 0), (r, r), (r, r)), mode="reflect")   # numpy's "reflect" does not repeat the edge: reflect-101
    acc = np.zeros_like(g)
    for dy in range(k):
        for dx in range(k):
            acc += pad[:, dy:dy + g.shape[1], dx:dx + g.shape[2]]
    return quant8(acc / float(k * k))


def mult_noise(g: np.ndarray, a, b, seed, index, epoch, field_id) -> np.ndarray:
    u = uniform24(noise_words(g.size, 4, seed, index, epoch, field_id, STAGE_MULT)[:, 0]).reshape(g.shape)
    return quant8(g * (np.float64(a) + np.float64(b) * u))


def gauss_noise(g: np.ndarray, sigma, seed, index, epoch, field_id) -> np.ndarray:
    wds = noise_words(g.size, 2, seed, index, epoch, field_id, STAGE_GAUSS)
    u1, u2 = uniform24(wds[:, 0]).reshape(g.shape), uniform24(wds[:, 1]).reshape(g.shape)
    return quant8(g + np.float64(sigma) * np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2))


def apply(field: np.ndarray, rec, mask: bool, order: int, seed: int, epoch: int, field_id: int):
    """One sample's field ``[P, H, W]`` uint8 through the pipeline the record ``rec`` describes -> (uint8 ``[P, H, W]``, ``safe [H, W]``)."""
    flags = int(rec["flags"])
    f = np.asarray(field)
    assert f.dtype == np.uint8 and f.ndim == 3
    g = np.rot90(f, int(rec["rot_k"]), axes=(1, 2))
    g, safe = shift_scale_rotate(g, rec["angle"], rec["scale"], rec["dx"], rec["dy"], mask)
    if not mask:
        index = int(rec["index"])
        if order == ORDER_UNET:
            if flags & BC:
                g = brightness_contrast(g, rec["alpha"], rec["beta"])
            if flags & BLUR:
                g = box_blur(g, int(rec["blur_k"]))
            if flags & MULT:
                g = mult_noise(g, rec["noise_a"], rec["noise_b"], seed, index, epoch, field_id)
        else:
            if flags & GAUSS:
                g = gauss_noise(g, rec["noise_a"], seed, index, epoch, field_id)
            if flags & BC:
                g = brightness_contrast(g, rec["alpha"], rec["beta"])
    return g.astype(np.uint8), safe
