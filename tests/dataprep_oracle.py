"""numpy restatement of the data preparation stage (``bio_image_unet_amd/dataprep.py``, ``csrc/biu_dataprep.hip``): grey morphology as a
minimum / maximum over explicit footprint offsets with explicit reflect indexing, Zhang-Suen thinning from its rules (vectorised over the
plane), the percentile normalisation in float64, the tile split as ``np.pad`` plus slicing, and the three family pipelines in the
reference's order.  Nothing here calls the package; everything is integer-exact apart from the float64 normalisation, which is the
formula ``workflow._percentile_rescale`` evaluates."""
import numpy as np


# ---- morphology ----------------------------------------------------------------------------------------------------------------------------
def footprint_offsets(kernel, size, op):
    """(dy, dx) of ``disk(size)`` / ``square(size)``; even squares in ``scipy.ndimage``'s convention (erosion [-w/2, w/2 - 1], dilation
    [-(w/2 - 1), w/2] per axis)."""
    if kernel == "disk":
        return [(dy, dx) for dy in range(-size, size + 1) for dx in range(-size, size + 1) if dy * dy + dx * dx <= size * size]
    if kernel != "square":
        raise ValueError(f"Dilate kernel {kernel} unknown!")
    h = size // 2
    lo, hi = (-h, h) if size % 2 else ((-h, h - 1) if op == "erosion" else (-(h - 1), h))
    return [(dy, dx) for dy in range(lo, hi + 1) for dx in range(lo, hi + 1)]


def footprint_array(kernel, size):
    """The 0 / 1 footprint array ``skimage.morphology.disk`` / ``square`` build."""
    if kernel == "disk":
        y, x = np.mgrid[-size:size + 1, -size:size + 1]
        return (y * y + x * x <= size * size).astype(np.uint8)
    return np.ones((size, size), dtype=np.uint8)


def reflect_edge(i, n):
    """``scipy.ndimage`` ``mode='reflect'``: the edge pixel repeated (-1 -> 0, -2 -> 1, n -> n - 1), period 2 n."""
    i = np.asarray(i) % (2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def morph(x, op, kernel, size):
    """Grey erosion (minimum) / dilation (maximum) of the last two axes of ``x``."""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    ys, xs = np.arange(H), np.arange(W)
    acc = None
    for dy, dx in footprint_offsets(kernel, size, op):
        v = x[..., reflect_edge(ys + dy, H)[:, None], reflect_edge(xs + dx, W)[None, :]]
        acc = v if acc is None else (np.minimum(acc, v) if op == "erosion" else np.maximum(acc, v))
    return acc


# ---- thinning ------------------------------------------------------------------------------------------------------------------------------
def clears(p, sub):
    """Whether a set pixel with neighbours ``p = [P2, P3, ..., P9]`` (clockwise from north; scalars or arrays of 0 / 1) is cleared in
    sub-iteration ``sub`` -- the rules, written out."""
    p2, p3, p4, p5, p6, p7, p8, p9 = p
    b = p2 + p3 + p4 + p5 + p6 + p7 + p8 + p9
    cyc = [p2, p3, p4, p5, p6, p7, p8, p9, p2]
    a = sum(((cyc[k] == 0) & (cyc[k + 1] == 1)) * 1 for k in range(8))
    ok = (b >= 2) & (b <= 6) & (a == 1)
    if sub == 0:
        return ok & (p2 * p4 * p6 == 0) & (p4 * p6 * p8 == 0)
    return ok & (p2 * p4 * p8 == 0) & (p2 * p6 * p8 == 0)


def thin_step(img, sub):
    """One sub-iteration on a 0 / 1 plane ``[H, W]``; pixels outside are 0; every pixel judged on ``img``."""
    H, W = img.shape
    q = np.zeros((H + 2, W + 2), dtype=np.int64)
    q[1:-1, 1:-1] = img
    nb = lambda dy, dx: q[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    p = [nb(-1, 0), nb(-1, 1), nb(0, 1), nb(1, 1), nb(1, 0), nb(1, -1), nb(0, -1), nb(-1, -1)]
    gone = (img == 1) & clears(p, sub)
    return np.where(gone, 0, img).astype(np.uint8), int(gone.sum())


def thin(img, return_iterations=False):
    """To the fixed point; ``img``: ``[H, W]`` or ``[planes, H, W]``, nonzero = set.  Iterations counted include the final one that clears nothing."""
    img = (np.asarray(img) != 0).astype(np.uint8)
    if img.ndim == 3:
        res = [thin(p, True) for p in img]
        out = np.stack([r[0] for r in res])
        return (out, [r[1] for r in res]) if return_iterations else out
    it = 0
    while True:
        img, c0 = thin_step(img, 0)
        img, c1 = thin_step(img, 1)
        it += 1
        if c0 + c1 == 0:
            return (img, it) if return_iterations else img


# ---- normalisation and split ---------------------------------------------------------------------------------------------------------------
def normalise_u8(unit, clip):
    """One item (all its channels or planes) clipped at its percentiles, shifted to 0, divided by its maximum, ``* 255``, truncated: float64."""
    a = np.asarray(unit).astype(np.float64)
    a = np.clip(a, a_min=np.nanpercentile(a, clip[0]), a_max=np.percentile(a, clip[1]))
    a = a - np.min(a)
    a = a / np.max(a)
    return (a * 255).astype("uint8")


def split(arr, dim_out, add=0, quirk_3d=False):
    """Tiles of the last ``len(dim_out)`` axes of ``arr`` as the reference cuts them: reflect-pad the far end up to ``dim_out``, N = ceil, N += add
    if N > 1, ``np.linspace(...).astype('int16')`` origins, first axis outermost.  ``quirk_3d``: ``unet3d/data.py:188-190``."""
    k = len(dim_out)
    lead = arr.ndim - k
    gaps = [max(0, d - e) for d, e in zip(dim_out, arr.shape[lead:])]
    arr = np.pad(arr, [(0, 0)] * lead + [(0, g) for g in gaps], "reflect")
    ext = arr.shape[lead:]
    n = [int(np.ceil(e / d)) for e, d in zip(ext, dim_out)]
    if quirk_3d:
        n[1] += add if n[0] > 1 else 0
        n[1] += add if n[1] > 1 else 0
        n[2] += add if n[2] > 1 else 0
    else:
        n = [v + (add if v > 1 else 0) for v in n]
    starts = [np.linspace(0, e - d, v).astype("int16") for e, d, v in zip(ext, dim_out, n)]
    tiles = []
    for idx in np.ndindex(*n):
        sl = tuple(slice(int(starts[a][i]), int(starts[a][i]) + dim_out[a]) for a, i in enumerate(idx))
        tiles.append(arr[(Ellipsis,) + sl])
    return np.stack(tiles)


# ---- the pipelines -------------------------------------------------------------------------------------------------------------------------
def edit_mask(mask, skeletonize, dilate_mask, dilate_kernel, invert):
    """unet / unet3d, per plane: skeletonise (> 1, thin, x 255), erosion for dilate_mask > 0, dilation for < 0, invert."""
    m = np.asarray(mask)
    m = m.astype(np.uint8) * np.uint8(255) if m.dtype == np.bool_ else m.astype(np.uint8)       # a bool mask is taken as 0 / 255
    if skeletonize:
        m = thin(m > 1) * np.uint8(255)
    if dilate_mask > 0:
        m = morph(m, "erosion", dilate_kernel, dilate_mask)
    elif dilate_mask < 0:
        m = morph(m, "dilation", dilate_kernel, -dilate_mask)
    if invert:
        m = 255 - m
    return m.astype(np.uint8)


def edit_mask_siam(mask, invert_masks, threshold_masks, skeletonize, dilate_mask, dilate_kernel):
    """siam: invert, threshold, skeletonise, then dilation for dilate_mask > 0 and erosion for < 0."""
    m = np.asarray(mask).astype(np.uint8).copy()
    if invert_masks:
        m = 255 - m
    if threshold_masks is not None:
        m = np.where(m >= threshold_masks, 255, 0).astype(np.uint8)
    if skeletonize:
        m[m > 1] = 1
        m = thin(m) * np.uint8(255)
    if dilate_mask > 0:
        m = morph(m, "dilation", dilate_kernel, dilate_mask)
    elif dilate_mask < 0:
        m = morph(m, "erosion", dilate_kernel, -dilate_mask)
    return m.astype(np.uint8)


def _squeeze(t, channels):
    return t[:, 0] if channels == 1 else t


def pipeline_unet(images, masks, dim_out, add_tile=0, dilate_mask=0, dilate_kernel="disk", invert=False, skeletonize=False, clip=(0.2, 99.8)):
    img_t, msk_t = [], []
    for img, msk in zip(images, masks):
        img, msk = (img[None] if img.ndim == 2 else img), (msk[None] if msk.ndim == 2 else msk)
        img_t.append(_squeeze(split(normalise_u8(img, clip), dim_out, add_tile), img.shape[0]))
        msk_t.append(_squeeze(split(edit_mask(msk, skeletonize, dilate_mask, dilate_kernel, invert), dim_out, add_tile), msk.shape[0]))
    return {"image": np.concatenate(img_t), "mask": np.concatenate(msk_t)}


def pipeline_unet3d(volumes, masks, dim_out, add_patch=0, dilate_mask=0, dilate_kernel="disk", invert=False, skeletonize=False, clip=(0.2, 99.8)):
    vol_t, msk_t = [], []
    for vol, msk in zip(volumes, masks):
        vol_t.append(split(normalise_u8(vol, clip), dim_out, add_patch, quirk_3d=True))
        msk_t.append(split(edit_mask(msk, skeletonize, dilate_mask, dilate_kernel, invert), dim_out, add_patch, quirk_3d=True))
    return {"volume": np.concatenate(vol_t), "mask": np.concatenate(msk_t)}


def pipeline_siam(pairs, masks, dim_out, dilate_mask=0, dilate_kernel="disk", invert_masks=False, threshold_masks=None, skeletonize=False,
                  clip=(0.2, 99.8)):
    out = {"image": [], "prev_image": [], "mask": []}
    for pair, msk in zip(pairs, masks):
        n = normalise_u8(pair, clip)                          # the pair as one unit, whichever way it is laid out
        prev, cur = (n[:, :n.shape[1] // 2], n[:, n.shape[1] // 2:]) if n.ndim == 2 else (n[0], n[1])
        out["prev_image"].append(split(prev, dim_out))
        out["image"].append(split(cur, dim_out))
        out["mask"].append(split(edit_mask_siam(msk, invert_masks, threshold_masks, skeletonize, dilate_mask, dilate_kernel), dim_out))
    return {k: np.concatenate(v) for k, v in out.items()}
