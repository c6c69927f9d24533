"""From raw images and label masks to a training ``TileStore`` on the device (``csrc/biu_dataprep.hip``, ``csrc/biu_prep.hip``).

What is left of the reference's ``DataProcess`` for the three uint8 families once augmentation runs on the fly (``Trainer(..., augment=True)``):
percentile normalisation of the images to bytes, the mask edit (skeletonise, erosion or dilation with a disk or square footprint, invert)
and the tile split.  ``prepare_unet`` / ``prepare_unet3d`` / ``prepare_siam`` take in-memory arrays, run every pixel operation in HBM and
return an open ``feed.TileStore`` of un-augmented uint8 tiles whose ``attrs`` carry ``dim_out``, ``clip_threshold`` and the augmentation
limits -- ``Trainer(store, ..., augment=True)`` needs nothing else.

Contract (what the tests hold it to; every comparison is an equality)

* Images: ``DeviceFrontEnd(...).normalise('single', clip_threshold)`` and ``tiles(..., out='uint8')`` as they stand, one item -- all its
  channels or planes, or both frames of a Siamese pair -- as one unit.  That is fp64 arithmetic from the uploaded values; the reference
  computes in float32, so the truncation can differ by one grey level on isolated pixels (DESIGN).
* ``morph``: grey erosion / dilation with ``disk(r)`` = ``{dy^2 + dx^2 <= r^2}`` (1 <= r <= 7) or ``square(w)`` (1 <= w <= 15), border and
  even-footprint convention of ``scipy.ndimage.grey_erosion`` / ``grey_dilation(footprint=..., mode='reflect')``.
* ``thin``: Zhang-Suen thinning as ``thin_table`` states it, pixels outside the plane 0, both sub-iterations judged on the state before
  them, iterated to the fixed point.  It is defined by these rules, not pinned to ``skimage.morphology.skeletonize``.
* ``gather``: tiles with ``np.pad(..., 'reflect')`` beyond the far end (``preprocess.reflect_index``), optional ``255 - v``.
* The split (``split_starts``, ``origins_2d``, ``origins_3d``) is the reference's, ``add_patch`` quirk of ``unet3d/data.py:188-190`` included.
* Masks are uint8; a bool mask is taken as 0 / 255.  The reference's ``int8`` round trip of masks is the identity on bytes.

The 2-D multi-output family has a fourth entry point at the end of this file, ``prepare_mo2d``: its ``DataProcess`` keeps every image whole
and crops at random, so the result is a ``feed.ImageStore`` of whole normalised images and float targets (NaN kept), not a store of tiles.
The 3-D multi-output family's ``prepare_mo3d`` does the same for whole volumes (``feed.VolumeStore``).
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import check, lib, ptr as _ptr, stream as _stream
from .feed import ImageStore, TileStore, VolumeStore
from .preprocess import DeviceFrontEnd
from .utils import get_device

ERODE, DILATE = 0, 1
FOOTPRINTS = {"disk": 0, "square": 1}
THIN_BLOCK = 8                  # full iterations enqueued between two reads of the cleared-pixel counter


# ---- host: the thinning table and the split geometry -------------------------------------------------------------------------------------
def thin_table() -> np.ndarray:
    """The 256-entry table ``biu_thin_step_u8`` reads, built from the Zhang-Suen rules.  Entry ``n`` describes the neighbourhood with
    P2 (north) in bit 0 of ``n`` and then clockwise P3 (NE), P4 (E), P5 (SE), P6 (S), P7 (SW), P8 (W), P9 (NW) in bits 1..7.  With
    B = set neighbours and A = 0 -> 1 steps in the cycle P2, P3, ..., P9, P2, a set pixel is cleared if 2 <= B <= 6, A == 1 and

        first sub-iteration  (bit 0 of the entry):  P2 P4 P6 == 0 and P4 P6 P8 == 0
        second sub-iteration (bit 1 of the entry):  P2 P4 P8 == 0 and P2 P6 P8 == 0"""
    tab = np.zeros(256, dtype=np.uint8)
    for n in range(256):
        p = [(n >> k) & 1 for k in range(8)]                 # p[0] = P2 ... p[7] = P9
        b = sum(p)
        a = sum(1 for k in range(8) if p[k] == 0 and p[(k + 1) % 8] == 1)
        if not (2 <= b <= 6 and a == 1):
            continue
        p2, p4, p6, p8 = p[0], p[2], p[4], p[6]
        first = p2 * p4 * p6 == 0 and p4 * p6 * p8 == 0
        second = p2 * p4 * p8 == 0 and p2 * p6 * p8 == 0
        tab[n] = int(first) | (int(second) << 1)
    return tab


def split_starts(extent: int, dim: int, add: int = 0) -> np.ndarray:
    """Tile origins along one axis as the reference's ``__split`` computes them: the axis is reflect-padded to ``dim`` where it is shorter,
    ``N = ceil(extent / dim)``, ``N += add`` if ``N > 1``, origins ``np.linspace(0, extent - dim, N).astype('int16')``."""
    extent = max(int(extent), int(dim))
    n = int(np.ceil(extent / dim))
    n += add if n > 1 else 0
    return np.linspace(0, extent - dim, n).astype("int16")


def origins_2d(shape, dim_out, add_tile: int = 0):
    """(row, column) of every tile of an ``[H, W]`` image in the reference's loop order (rows outer)."""
    ys, xs = split_starts(shape[0], dim_out[0], add_tile), split_starts(shape[1], dim_out[1], add_tile)
    return [(int(y), int(x)) for y in ys for x in xs]


def origins_3d(shape, dim_out, add_patch: int = 0):
    """(z, row, column) of every patch of a ``[D, H, W]`` volume, ``unet3d/data.py:185-200`` as written: ``N_x`` grows by ``add_patch`` when
    ``N_z > 1`` and again when the grown ``N_x > 1``; ``N_y`` grows when ``N_y > 1``; ``N_z`` never grows."""
    ext = [max(int(e), int(d)) for e, d in zip(shape, dim_out)]
    n_z, n_x, n_y = (int(np.ceil(e / d)) for e, d in zip(ext, dim_out))
    n_x += add_patch if n_z > 1 else 0
    n_x += add_patch if n_x > 1 else 0
    n_y += add_patch if n_y > 1 else 0
    zs, xs, ys = (np.linspace(0, e - d, n).astype("int16") for e, d, n in zip(ext, dim_out, (n_z, n_x, n_y)))
    return [(int(z), int(x), int(y)) for z in zs for x in xs for y in ys]


# ---- device: the four kernels --------------------------------------------------------------------------------------------------------------
def _planes(x: torch.Tensor, what: str) -> torch.Tensor:
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise RuntimeError(f"{what} needs a tensor on the GPU; there is no CPU path")
    if x.dtype != torch.uint8 or x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"{what}: need a non-empty uint8 tensor [planes, H, W], got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def lut(x: torch.Tensor, table, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``table[x]`` for a uint8 device tensor (``biu_lut_u8``); ``table``: 256 values in 0..255.  ``out`` may be ``x`` itself."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()):
        raise ValueError("lut: need a contiguous uint8 tensor on the GPU")
    tab = np.asarray(table)
    if tab.shape != (256,) or tab.min() < 0 or tab.max() > 255:
        raise ValueError("lut: the table holds 256 values in 0..255")
    out = torch.empty_like(x) if out is None else out
    if x.numel() == 0:
        return out
    with torch.cuda.device(x.device):
        t = torch.from_numpy(tab.astype(np.uint8)).to(x.device)
        check(lib.biu_lut_u8(_ptr(x), _ptr(t), _ptr(out), x.numel(), _stream()), "lut_u8")
    return out


def morph(x: torch.Tensor, op: str, kernel: str, size: int) -> torch.Tensor:
    """Grey ``'erosion'`` or ``'dilation'`` of every plane of ``x`` ``[planes, H, W]`` (uint8, on the GPU) with ``disk(size)`` or
    ``square(size)`` (``biu_morph_u8``); enqueued on the current stream."""
    if op not in ("erosion", "dilation"):
        raise ValueError(f"morph: operation {op} unknown!")
    if kernel not in FOOTPRINTS:
        raise ValueError(f"Dilate kernel {kernel} unknown!")
    x = _planes(x, "morph")
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(lib.biu_morph_u8(_ptr(x), _ptr(out), x.shape[0], x.shape[1], x.shape[2], ERODE if op == "erosion" else DILATE, FOOTPRINTS[kernel],
                               int(size), _stream()), "morph_u8")
    return out


def thin(x: torch.Tensor, block: int = THIN_BLOCK) -> torch.Tensor:
    """Zhang-Suen thinning of every plane of ``x`` ``[planes, H, W]`` (uint8 on the GPU, nonzero = set) to its fixed point; returns 0 / 1 bytes.

    Launch plan: one launch per sub-iteration, ping-pong between two buffers (the kernel boundary is the only synchronisation between
    workgroups).  ``block`` full iterations are enqueued, then the counter the launches added their cleared pixels to is read once; the
    loop stops when a block cleared nothing.  A converged image is a fixed point of both sub-iterations, so the result does not depend on
    ``block``.  Every iteration before convergence clears at least one pixel, so (foreground + 1) iterations always suffice: a block that
    would start beyond them (beyond ``foreground + block - 1`` in whole blocks) raises ``RuntimeError`` instead."""
    x = _planes(x, "thin")
    block = int(block)
    if block < 1:
        raise ValueError("thin: block >= 1")
    with torch.cuda.device(x.device):
        table = torch.from_numpy(thin_table()).to(x.device)
        a, b = torch.empty_like(x), torch.empty_like(x)
        counter = torch.zeros((1,), dtype=torch.int64, device=x.device)
        foreground = int(torch.count_nonzero(x).item())
        args = (x.shape[0], x.shape[1], x.shape[2])
        src, done = x, 0
        while True:
            if done > foreground + block - 1:
                raise RuntimeError(f"thin: no fixed point after {done} iterations of an image with {foreground} foreground pixels")
            counter.zero_()
            for _ in range(block):
                check(lib.biu_thin_step_u8(_ptr(src), _ptr(a), *args, 0, _ptr(table), _ptr(counter), _stream()), "thin_step_u8")
                check(lib.biu_thin_step_u8(_ptr(a), _ptr(b), *args, 1, _ptr(table), _ptr(counter), _stream()), "thin_step_u8")
                src = b
            done += block
            if int(counter.item()) == 0:
                return b


def gather(x: torch.Tensor, depth: int, origins, tile, invert: bool = False) -> torch.Tensor:
    """Tiles ``[len(origins), td, th, tw]`` of the uint8 stack ``x`` ``[planes, H, W]`` (``biu_tile_gather_u8``): ``origins`` are (plane, row,
    column) with the plane counted over the whole stack; a tile stays inside the block of ``depth`` planes that holds its first plane and
    reflects beyond the far ends as ``np.pad(..., 'reflect')`` does.  ``invert`` writes ``255 - v``."""
    x = _planes(x, "gather")
    td, th, tw = (int(t) for t in tile)
    rec = np.asarray([(0, z, y, c) for z, y, c in origins], dtype=np.int64).reshape(-1, 4)
    if depth < 1 or x.shape[0] % depth or min(td, th, tw) < 1:
        raise ValueError(f"gather: depth {depth} does not divide {x.shape[0]} planes, or an empty tile {tile}")
    if rec.size == 0 or rec.min() < 0 or rec.max() >= 2 ** 30 or (rec[:, 1] >= x.shape[0]).any():
        raise ValueError("tile origins outside the stack")
    out = torch.empty((rec.shape[0], td, th, tw), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        dev = torch.from_numpy(np.ascontiguousarray(rec.astype(np.int32))).to(x.device)
        check(lib.biu_tile_gather_u8(_ptr(x), x.shape[0], int(depth), x.shape[1], x.shape[2], _ptr(dev), rec.shape[0], td, th, tw,
                                     int(bool(invert)), _ptr(out), _stream()), "tile_gather_u8")
    return out


# ---- the mask edit -------------------------------------------------------------------------------------------------------------------------
_V = np.arange(256)
_TIMES_255 = np.where(_V != 0, 255, 0)


def edit_mask(m: torch.Tensor, skeletonize: bool, dilate_mask: int, dilate_kernel: str) -> torch.Tensor:
    """``unet`` / ``unet3d`` (``unet/data.py:148-161``), every plane by itself: binarise ``> 1``, thin, ``x 255`` if ``skeletonize``;
    ``dilate_mask > 0`` ERODES with ``kernel(dilate_mask)``, ``< 0`` dilates with ``kernel(-dilate_mask)`` (the reference's sign).  The
    final ``255 - v`` of ``invert`` commutes with the tile gather and rides in it."""
    if skeletonize:
        m = lut(thin(lut(m, _V > 1)), _TIMES_255)
    if dilate_mask > 0:
        m = morph(m, "erosion", dilate_kernel, dilate_mask)
    elif dilate_mask < 0:
        m = morph(m, "dilation", dilate_kernel, -dilate_mask)
    return m


def edit_mask_siam(m: torch.Tensor, invert_masks: bool, threshold_masks, skeletonize: bool, dilate_mask: int, dilate_kernel: str) -> torch.Tensor:
    """``siam_unet/data.py:162-179``: invert, threshold (``>= t`` -> 255, else 0), skeletonise (``> 1`` -> 1, thin what is not 0, ``x 255``),
    then ``dilate_mask > 0`` DILATES and ``< 0`` erodes -- the opposite sign of the other two families.  The pointwise steps are one table."""
    v = _V.copy()
    if invert_masks:
        v = 255 - v
    if threshold_masks is not None:
        v = np.where(v >= threshold_masks, 255, 0)
    if skeletonize:
        v = np.where(v > 1, 1, v) != 0
    if invert_masks or threshold_masks is not None or skeletonize:
        m = lut(m, v)
    if skeletonize:
        m = lut(thin(m), _TIMES_255)
    if dilate_mask > 0:
        m = morph(m, "dilation", dilate_kernel, dilate_mask)
    elif dilate_mask < 0:
        m = morph(m, "erosion", dilate_kernel, -dilate_mask)
    return m


# ---- the three entry points ----------------------------------------------------------------------------------------------------------------
def _load(item) -> np.ndarray:
    if isinstance(item, (str, os.PathLike)):
        import tifffile                                       # optional, as for Predict2D: arrays need nothing
        return tifffile.imread(os.fspath(item))
    return np.asarray(item)


def _mask_u8(m: np.ndarray) -> np.ndarray:
    if m.dtype == np.bool_:
        return m.astype(np.uint8) * 255
    if m.dtype != np.uint8:
        raise TypeError(f"masks are uint8 or bool arrays, got {m.dtype}")
    return m


def _check_common(images, masks, dilate_kernel):
    if len(masks) != len(images):
        raise ValueError("Number of ground truth does not match number of image stacks")
    if dilate_kernel not in FOOTPRINTS:
        raise ValueError(f"Dilate kernel {dilate_kernel} unknown!")
    if len(images) == 0:
        raise ValueError("no images")


def _device(device) -> torch.device:
    device = get_device() if device == "auto" else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"data preparation runs on the GPU (biu_morph_u8, biu_thin_step_u8, biu_tile_gather_u8); got device '{device}'")
    return device


def _attrs(dim_out, clip_threshold, **limits):
    plain = lambda v: [plain(e) for e in v] if isinstance(v, (tuple, list)) else v
    return {"dim_out": [int(d) for d in dim_out], "clip_threshold": plain(clip_threshold), **{k: plain(v) for k, v in limits.items()}}


def _image_tiles(unit: np.ndarray, device, clip_threshold, origins, tile, view) -> np.ndarray:
    """``unit`` ``[planes, H, W]`` normalised as one image; ``origins``: (plane, row, column) per tile."""
    fe = DeviceFrontEnd(unit, device, depth=unit.shape[0])
    fe.normalise("single", clip_threshold)
    t = fe.tiles([(0, z, y, x) for z, y, x in origins], tile, out="uint8", view=view)
    return t.batch(0, len(t)).cpu().numpy()


def prepare_unet(images: Sequence, masks: Sequence, path: str, dim_out=(256, 256), in_channels: int = 1, out_channels: int = 1, dilate_mask: int = 0,
                 dilate_kernel: str = "disk", add_tile: int = 0, invert: bool = False, skeletonize: bool = False, clip_threshold=(0.2, 99.8),
                 shiftscalerotate=(0, 0, 0), noise_lims=(0.5, 1.2), brightness_contrast=(0.25, 0.25), blur_limit=(3, 7), device="auto") -> TileStore:
    """``bio_image_unet.unet.DataProcess`` up to its split (``unet/data.py:124-215``) from arrays: ``images`` ``[H, W]`` or ``[C, H, W]`` of any
    dtype the device front end uploads, ``masks`` ``[H, W]`` or ``[C, H, W]`` uint8 or bool, sizes free per item.  Returns the open store at
    ``path`` with fields ``image`` / ``mask`` (a channel axis only where ``in_channels`` / ``out_channels`` exceeds 1)."""
    _check_common(images, masks, dilate_kernel)
    items = []
    for img, msk in zip(images, masks):
        img, msk = _load(img), _mask_u8(_load(msk))
        img, msk = (img[None] if img.ndim == 2 else img), (msk[None] if msk.ndim == 2 else msk)
        if img.ndim != 3 or msk.ndim != 3 or img.shape[0] != in_channels or msk.shape[0] != out_channels or img.shape[1:] != msk.shape[1:]:
            raise ValueError(f"image {img.shape} and mask {msk.shape} do not make an item of {in_channels} input and {out_channels} output channels")
        items.append((img, msk, origins_2d(img.shape[1:], dim_out, add_tile)))
    device = _device(device)
    th, tw = (int(d) for d in dim_out)
    shp = lambda c: (th, tw) if c == 1 else (c, th, tw)
    store = TileStore.create(path, sum(len(o) for _, _, o in items), {"image": shp(in_channels), "mask": shp(out_channels)},
                             _attrs(dim_out, clip_threshold, shiftscalerotate=shiftscalerotate, noise_lims=noise_lims,
                                    brightness_contrast=brightness_contrast, blur_limit=blur_limit))
    n = 0
    for img, msk, org in items:
        zyx = [(0, y, x) for y, x in org]
        store.maps["image"][n:n + len(org)] = _image_tiles(img, device, clip_threshold, zyx, (in_channels, th, tw), shp(in_channels))
        m = edit_mask(torch.from_numpy(np.ascontiguousarray(msk)).to(device), skeletonize, dilate_mask, dilate_kernel)
        store.maps["mask"][n:n + len(org)] = gather(m, out_channels, zyx, (out_channels, th, tw), invert).view((len(org),) + shp(out_channels)).cpu().numpy()
        n += len(org)
    store.flush()
    return store


def prepare_unet3d(volumes: Sequence, masks: Sequence, path: str, dim_out=(128, 128, 128), dilate_mask: int = 0, dilate_kernel: str = "disk",
                   add_patch: int = 0, invert: bool = False, skeletonize: bool = False, clip_threshold=(0.2, 99.8), shiftscalerotate=(0, 0, 0),
                   noise_amp=10, brightness_contrast=(0.25, 0.25), device="auto") -> TileStore:
    """``bio_image_unet.unet3d.DataProcess`` up to its split (``unet3d/data.py:116-207``) from ``[D, H, W]`` arrays; the mask edit runs slice by
    slice in 2-D, as there.  Fields ``volume`` / ``mask``, both ``dim_out``."""
    _check_common(volumes, masks, dilate_kernel)
    items = []
    for vol, msk in zip(volumes, masks):
        vol, msk = _load(vol), _mask_u8(_load(msk))
        if vol.ndim != 3 or vol.shape != msk.shape:
            raise ValueError(f"volume {vol.shape} and mask {msk.shape} do not make a [D, H, W] item")
        items.append((vol, msk, origins_3d(vol.shape, dim_out, add_patch)))
    device = _device(device)
    dim = tuple(int(d) for d in dim_out)
    store = TileStore.create(path, sum(len(o) for _, _, o in items), {"volume": dim, "mask": dim},
                             _attrs(dim_out, clip_threshold, shiftscalerotate=shiftscalerotate, noise_amp=noise_amp, brightness_contrast=brightness_contrast))
    n = 0
    for vol, msk, org in items:
        store.maps["volume"][n:n + len(org)] = _image_tiles(vol, device, clip_threshold, org, dim, dim)
        m = edit_mask(torch.from_numpy(np.ascontiguousarray(msk)).to(device), skeletonize, dilate_mask, dilate_kernel)
        store.maps["mask"][n:n + len(org)] = gather(m, vol.shape[0], org, dim, invert).cpu().numpy()
        n += len(org)
    store.flush()
    return store


def prepare_siam(pairs: Sequence, masks: Sequence, path: str, dim_out=(256, 256), dilate_mask: int = 0, dilate_kernel: str = "disk",
                 invert_masks: bool = False, threshold_masks=None, skeletonize: bool = False, clip_threshold=(0.2, 99.8), shiftscalerotate=(0, 0, 0),
                 noise_amp=10, brightness_contrast=(0.25, 0.25), rescale=None, device="auto") -> TileStore:
    """``bio_image_unet.siam_unet.DataProcess`` up to its split (``siam_unet/data.py:126-233``) from arrays: a pair is ``[2, H, W]`` (previous,
    current) or ``[H, 2 W]`` (previous on the left) and is normalised as one unit; ``masks`` are ``[H, W]``.  Fields ``image`` / ``prev_image`` /
    ``mask``.  ``rescale`` other than ``None`` is refused: it is ``skimage.transform.rescale``."""
    if rescale is not None:
        raise NotImplementedError("rescale needs skimage.transform and is not supported: rescale the arrays before they are prepared")
    _check_common(pairs, masks, dilate_kernel)
    items = []
    for pair, msk in zip(pairs, masks):
        pair, msk = _load(pair), _mask_u8(_load(msk))
        if pair.ndim == 2:
            if pair.shape[1] % 2:
                raise ValueError(f"a side-by-side pair needs an even width, got {pair.shape}")
            half = pair.shape[1] // 2
            pair = np.stack([pair[:, :half], pair[:, half:]])
        elif pair.ndim != 3 or pair.shape[0] != 2:
            raise ValueError("Unknown data structure of input images.")
        if msk.ndim != 2 or msk.shape != pair.shape[1:]:
            raise ValueError(f"pair {pair.shape} and mask {msk.shape} do not make an item")
        items.append((pair, msk, origins_2d(msk.shape, dim_out)))
    device = _device(device)
    th, tw = (int(d) for d in dim_out)
    store = TileStore.create(path, sum(len(o) for _, _, o in items), {"image": (th, tw), "prev_image": (th, tw), "mask": (th, tw)},
                             _attrs(dim_out, clip_threshold, shiftscalerotate=shiftscalerotate, noise_amp=noise_amp, brightness_contrast=brightness_contrast))
    n = 0
    for pair, msk, org in items:
        both = _image_tiles(pair, device, clip_threshold, [(z, y, x) for z in (0, 1) for y, x in org], (1, th, tw), (th, tw))
        store.maps["prev_image"][n:n + len(org)], store.maps["image"][n:n + len(org)] = both[:len(org)], both[len(org):]
        m = edit_mask_siam(torch.from_numpy(np.ascontiguousarray(msk[None])).to(device), invert_masks, threshold_masks, skeletonize, dilate_mask, dilate_kernel)
        store.maps["mask"][n:n + len(org)] = gather(m, 1, [(0, y, x) for y, x in org], (1, th, tw)).view(len(org), th, tw).cpu().numpy()
        n += len(org)
    store.flush()
    return store


# ---- the 2-D multi-output family: whole items, NaN targets ------------------------------------------------------------------------------------
def _mo2d_items(images, targets, in_channels):
    """The host half of ``prepare_mo2d``: every item as ``(image [C, H, W], {name: float32 [planes, H, W]})`` plus the planes and the
    squeeze flag of every field.  Needs no device, so every ``ValueError`` of ``prepare_mo2d`` is raised before one is asked for."""
    if len(images) == 0:
        raise ValueError("no images")
    if not targets:
        raise ValueError("no targets")
    for name, seq in targets.items():
        if name == "image":
            raise ValueError('a target cannot be named "image"')
        if len(seq) != len(images):
            raise ValueError(f'target "{name}": {len(seq)} items for {len(images)} images')
    items, planes, squeeze = [], {}, {}
    for i, img in enumerate(images):
        img = _load(img)
        unit = img[None] if img.ndim == 2 else img
        if unit.ndim != 3 or unit.shape[0] != in_channels:
            raise ValueError(f"image {i}: shape {img.shape} is not [H, W] or [{in_channels}, H, W] (in_channels = {in_channels})")
        item = {}
        for name, seq in targets.items():
            t = _load(seq[i])
            if t.dtype.kind not in "buif":
                raise ValueError(f'target "{name}" of item {i}: bool or a real dtype, got {t.dtype}')
            if t.shape[-2:] != unit.shape[1:] or t.ndim not in (2, 3) or (name == "orientation" and t.ndim != 2):
                raise ValueError(f"Item: {i}. Shape mismatch: {name} has shape {t.shape} but expected {img.shape}")
            t = t.astype(np.float32)
            if name == "orientation":                        # an angle map becomes the rotated pair; NaN in both where the angle is NaN
                t, sq = np.stack([np.cos(t), np.sin(t)]), False
            else:
                t, sq = (t[None], True) if t.ndim == 2 else (t, False)
            if planes.setdefault(name, t.shape[0]) != t.shape[0] or squeeze.setdefault(name, sq) != sq:
                raise ValueError(f'target "{name}" of item {i}: {t.shape[0]} plane(s), the items before it have {planes[name]}')
            item[name] = t
        items.append((unit, item))
    return items, planes, squeeze


def prepare_mo2d(images: Sequence, targets, path: str, dim_out=(256, 256), in_channels: int = 1, nan_to_val: float = 0,
                 clip_threshold=(0., 99.99), aug_factor: float = 2, gauss_noise_lims=(0.01, 0.1), shot_noise_lims=(0.001, 0.01),
                 brightness_contrast=(0.1, 0.1), blur_limit=(3, 5), random_rotate: bool = True, scale_limit=(0, 0), image_dtype: str = "f32",
                 device="auto") -> ImageStore:
    """``bio_image_unet.multi_output_unet.DataProcess`` up to its augmentation (``multi_output_unet/data.py:140-185``) from arrays, into a
    ``feed.ImageStore`` of WHOLE items: ``TrainerMo2d(store, ...)`` then renders ``max(int(H W / (dh dw) aug_factor), 2)`` fresh random
    crops per item and epoch on the device.  ``images``: ``[H, W]`` or ``[C, H, W]`` of any dtype the device front end uploads, each
    normalised as one unit by ``DeviceFrontEnd.normalise('single', clip_threshold)`` and read back whole as float32 (``image_dtype="u8"``:
    as bytes, a quarter of the arena).  ``targets``: ``{name: sequence}`` of ``[H, W]`` or ``[C, H, W]`` arrays, bool or real, stored as
    float32 with NaN ("no label here") kept; the target named ``orientation`` is an angle map ``[H, W]`` and is stored as the two planes
    ``(cos, sin)``.  ``add_tile`` and ``val_split`` of the reference do not apply (the Trainer splits patch indices)."""
    if image_dtype not in ("f32", "u8"):
        raise ValueError(f'image_dtype "{image_dtype}": "f32" or "u8"')
    if len(dim_out) != 2 or min(dim_out) < 1:
        raise ValueError(f"dim_out {dim_out}: (height, width) of a patch")
    if not aug_factor > 0:
        raise ValueError("aug_factor must be positive")
    if not np.isfinite(nan_to_val):
        raise ValueError("nan_to_val must be finite")
    items, planes, squeeze = _mo2d_items(images, targets, int(in_channels))
    device = _device(device)
    fields = {"image": int(in_channels), **planes}
    store = ImageStore.create(path, [u.shape[1:] for u, _ in items], fields,
                              {**_attrs(dim_out, clip_threshold, gauss_noise_lims=gauss_noise_lims, shot_noise_lims=shot_noise_lims,
                                        brightness_contrast=brightness_contrast, blur_limit=blur_limit, scale_limit=scale_limit),
                               "random_rotate": bool(random_rotate), "aug_factor": aug_factor, "nan_to_val": float(nan_to_val)},
                              {"image": image_dtype, **{k: "f32" for k in planes}}, {"image": in_channels == 1, **squeeze})
    for i, (unit, item) in enumerate(items):
        c, h, w = unit.shape
        fe = DeviceFrontEnd(unit, device, depth=c)
        fe.normalise("single", clip_threshold)
        t = fe.tiles([(0, 0, 0, 0)], (c, h, w), out="uint8" if image_dtype == "u8" else "float32")
        store.put(i, "image", t.batch(0, 1)[0].cpu().numpy())
        for name, v in item.items():
            store.put(i, name, v)
    store.flush()
    return store


# ---- the 3-D multi-output family: whole volumes, NaN targets ------------------------------------------------------------------------------------
def _mo3d_items(volumes, targets, in_channels, dim_out):
    """The host half of ``prepare_mo3d``: every item as ``(volume [C, D, H, W], {name: float32 [channels, D, H, W]})`` plus the channels and
    the squeeze flag of every field.  Needs no device, so every ``ValueError`` of ``prepare_mo3d`` is raised before one is asked for."""
    if len(volumes) == 0:
        raise ValueError("no volumes")
    if not targets:
        raise ValueError("no targets")
    for name, seq in targets.items():
        if name == "volume":
            raise ValueError('a target cannot be named "volume"')
        if len(seq) != len(volumes):
            raise ValueError(f'target "{name}": {len(seq)} items for {len(volumes)} volumes')
    items, channels, squeeze = [], {}, {}
    for i, vol in enumerate(volumes):
        vol = _load(vol)
        unit = vol[None] if vol.ndim == 3 else vol
        if unit.ndim != 4 or unit.shape[0] != in_channels:
            raise ValueError(f"volume {i}: shape {vol.shape} is not [D, H, W] or [{in_channels}, D, H, W] (in_channels = {in_channels})")
        if any(e < t for e, t in zip(unit.shape[1:], dim_out)):
            raise ValueError(f"item {i}: {tuple(unit.shape[1:])} is smaller than dim_out {tuple(dim_out)}; a crop cannot be larger than its volume")
        item = {}
        for name, seq in targets.items():
            t = _load(seq[i])
            if t.dtype.kind not in "buif":
                raise ValueError(f'target "{name}" of item {i}: bool or a real dtype, got {t.dtype}')
            if t.shape[-3:] != unit.shape[1:] or t.ndim not in (3, 4) or (name == "orientation" and t.ndim != 3):
                raise ValueError(f"Item: {i}. Shape mismatch: {name} has shape {t.shape} but expected {vol.shape}")
            t = t.astype(np.float32)
            if name == "orientation":                        # an angle volume becomes the rotated pair; NaN in both where the angle is NaN
                t, sq = np.stack([np.cos(t), np.sin(t)]), False
            else:
                t, sq = (t[None], True) if t.ndim == 3 else (t, False)
            if channels.setdefault(name, t.shape[0]) != t.shape[0] or squeeze.setdefault(name, sq) != sq:
                raise ValueError(f'target "{name}" of item {i}: {t.shape[0]} channel(s), the items before it have {channels[name]}')
            item[name] = t
        items.append((unit, item))
    return items, channels, squeeze


def prepare_mo3d(volumes: Sequence, targets, path: str, dim_out=(128, 128, 128), in_channels: int = 1, nan_to_val: float = 0,
                 clip_threshold=(0., 99.99), aug_factor: int = 10, scale_limit=(-0.75, 0), rotate_limit=(0, 360), gauss_noise_lims=(0.01, 0.1),
                 shot_noise_lims=(0.005, 0.01), brightness_contrast=(0.1, 0.1), blur_limit=(3, 7), volume_dtype: str = "f32",
                 device="auto") -> VolumeStore:
    """``bio_image_unet.multi_output_unet3d.DataProcess`` up to its augmentation (``multi_output_unet3d/data.py:57-150``) from arrays, into a
    ``feed.VolumeStore`` of WHOLE volumes: ``TrainerMo3d(store, ...)`` then renders ``aug_factor`` fresh random crops per volume and epoch on
    the device (shift-scale-rotate of the whole volume, then ``RandomCrop3D(dim_out)``).  The keywords and defaults are the reference
    ``DataProcess``'s; its ``add_tile``, ``val_split``, ``random_rotate`` and ``create`` do not apply (nothing is tiled or written as TIFF,
    the Trainer splits patch indices, and the rotation is ``rotate_limit``'s).

    ``volumes``: ``[D, H, W]`` or ``[C, D, H, W]`` of any dtype the device front end uploads, each normalised as one unit by
    ``DeviceFrontEnd.normalise('single', clip_threshold)`` and read back whole as the field ``volume`` in float32 (``volume_dtype="u8"``: as
    bytes, a quarter of the arena).  ``targets``: ``{name: sequence}`` of ``[D, H, W]`` or ``[C, D, H, W]`` arrays, bool or real, stored as
    float32 with NaN ("no label here") kept; the target named ``orientation`` is an angle volume ``[D, H, W]`` and is stored as the two
    channels ``(cos, sin)``, NaN in both where the angle is NaN."""
    if volume_dtype not in ("f32", "u8"):
        raise ValueError(f'volume_dtype "{volume_dtype}": "f32" or "u8"')
    if len(dim_out) != 3 or min(dim_out) < 1:
        raise ValueError(f"dim_out {dim_out}: (depth, height, width) of a patch")
    if int(aug_factor) != aug_factor or aug_factor < 1:
        raise ValueError("aug_factor: a whole number of patches per volume, at least 1")
    if not np.isfinite(nan_to_val):
        raise ValueError("nan_to_val must be finite")
    dim_out = tuple(int(d) for d in dim_out)
    items, channels, squeeze = _mo3d_items(volumes, targets, int(in_channels), dim_out)
    device = _device(device)
    fields = {"volume": int(in_channels), **channels}
    store = VolumeStore.create(path, [u.shape[1:] for u, _ in items], fields,
                               {**_attrs(dim_out, clip_threshold, scale_limit=scale_limit, rotate_limit=rotate_limit, gauss_noise_lims=gauss_noise_lims,
                                         shot_noise_lims=shot_noise_lims, brightness_contrast=brightness_contrast, blur_limit=blur_limit),
                                "aug_factor": int(aug_factor), "nan_to_val": float(nan_to_val)},
                               {"volume": volume_dtype, **{k: "f32" for k in channels}}, {"volume": in_channels == 1, **squeeze})
    for i, (unit, item) in enumerate(items):
        c, d, h, w = unit.shape
        planes = np.ascontiguousarray(unit).reshape(c * d, h, w)     # one unit for the percentiles: every channel and plane of the volume
        fe = DeviceFrontEnd(planes, device, depth=c * d)
        fe.normalise("single", clip_threshold)
        t = fe.tiles([(0, 0, 0, 0)], (c * d, h, w), out="uint8" if volume_dtype == "u8" else "float32")
        store.put(i, "volume", t.batch(0, 1)[0].cpu().numpy().reshape(c, d, h, w))
        for name, v in item.items():
            store.put(i, name, v)
    store.flush()
    return store
