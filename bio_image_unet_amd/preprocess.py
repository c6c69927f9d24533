"""The front of the Predict pipelines on the device: percentile normalisation and tiling of the raw stack (``csrc/biu_prep.hip``).

The reference's ``Predict`` classes clip every image at two percentiles, rescale it and cut tiles in numpy before the first forward.  The
device front end keeps that stage in HBM: the raw stack goes up once in its own dtype, the order statistics the percentiles need are
selected exactly (``biu_order_stats``: radix select, integer atomics only, deterministic), ``biu_prep_finalize`` restates numpy's linear
percentile in fp64, and ``biu_prep_tiles`` clips, rescales and gathers tiles in one pass -- no normalised image is ever materialised and
no pixel is touched by host arithmetic.  ``Predict*(..., preprocess='device')`` in ``workflow.py`` is the user; the default stays ``'host'``.

Contract (what the tests hold it to)

* ``order_stats`` returns ``np.sort(segment)[rank]`` exactly, as fp64.
* The percentile is ``percentile_from_neighbours``: ``np.percentile`` / ``np.nanpercentile`` (method ``'linear'``) of float64 data bit for bit.
* Pixel arithmetic is fp64 from the values as uploaded, in the host's operation order, one rounding per operation (FMA contraction is off in
  the kernels).  For integer and float64 input that is the host path bit for bit (``Predict2D`` / ``Predict3D`` / ``PredictSiam`` compute in
  float64 there).  float64 input is uploaded as float32 and therefore refused (``ValueError``) unless every value is exactly representable.
* For float32 input ``Predict2D`` / ``Predict3D`` and the two multi-output predictors run their host arithmetic -- numpy's percentile
  interpolation included -- in float32; the device result is the same formula evaluated in float64 and rounded once.
* NaN in float input raises ``ValueError`` (use ``preprocess='host'``); the count comes from the selection kernels, read once per stack.
* A constant image divides 0 by 0 as on the host; the uint8 cast of that NaN is unspecified on both paths.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from ._lib import check, lib, stream as _stream

ELEM_U8, ELEM_U16, ELEM_I16, ELEM_F32 = 0, 1, 2, 3
_ELEM_NP = {np.dtype("uint8"): ELEM_U8, np.dtype("uint16"): ELEM_U16, np.dtype("int16"): ELEM_I16, np.dtype("float32"): ELEM_F32}
_ELEM_TORCH = {torch.uint8: ELEM_U8, torch.uint16: ELEM_U16, torch.int16: ELEM_I16, torch.float32: ELEM_F32}
FAMILIES = {"minmax": 0, "minmax_eps": 1, "lohi_eps": 2}
MAX_RANKS = 8


def percentile_ranks(q: float, n: int):
    """0-based sorted positions (k, k1) of the two neighbours ``np.percentile(x, q)`` interpolates between for ``len(x) == n``:
    ``k = floor(q/100 * (n - 1))``, ``k1 = k + 1``, and ``k1 = k = n - 1`` once the virtual index reaches the last element."""
    if not 0. <= q <= 100.:
        raise ValueError("Percentiles must be in the range [0, 100]")
    vi = (n - 1) * (q / 100.0)
    k = min(int(math.floor(vi)), n - 1)
    return k, (k if vi >= n - 1 else k + 1)


def percentile_from_neighbours(xk, xk1, q: float, n: int):
    """numpy's linear percentile from the two selected neighbours, in float64 -- the formula ``biu_prep_finalize`` evaluates:

        vi = q/100 * (n - 1);  g = vi - floor(vi);  r = xk + (xk1 - xk) * g,  and  r = xk1 - (xk1 - xk) * (1 - g)  when g >= 0.5

    with ``xk = sorted[k]``, ``xk1 = sorted[k1]`` of ``percentile_ranks(q, n)``.  Equal to ``np.percentile`` and ``np.nanpercentile`` of
    NaN-free float64 data bit for bit (every operation rounded on its own: no FMA)."""
    xk, xk1 = np.float64(xk), np.float64(xk1)
    vi = np.float64(n - 1) * np.float64(q / 100.0)
    g = vi - np.floor(vi)
    d = xk1 - xk
    return xk1 - d * (np.float64(1.0) - g) if g >= 0.5 else xk + d * g


def reflect_index(i: int, n: int) -> int:
    """Source index of position ``i >= 0`` along an axis of extent ``n`` under ``np.pad(..., 'reflect')`` at the far end (no edge repeat,
    period ``2 (n - 1)``, folded as often as it takes; ``n == 1`` -> 0) -- the rule ``biu_prep_tiles`` applies beyond the image."""
    if n == 1:
        return 0
    i %= 2 * (n - 1)
    return i if i < n else 2 * (n - 1) - i


def order_stats(x: torch.Tensor, ranks, segments: int = 1, n: int = None, stride: int = None, return_nan_count: bool = False):
    """Exact order statistics of a device tensor (uint8, uint16, int16 or float32, contiguous): ``x`` is read as ``segments`` runs of ``n``
    elements, run ``s`` starting at element ``s * stride`` (default: ``x`` cut into ``segments`` equal parts), and the result
    ``[segments, len(ranks)]`` (float64, on the device) holds ``np.sort(run)[rank]`` for every rank (0-based, at most 8).  Enqueued on the
    current stream without a synchronisation.  With ``return_nan_count`` also the number of NaN elements met (device int64 scalar)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise RuntimeError("order_stats needs a tensor on the GPU; there is no CPU path")
    if x.dtype not in _ELEM_TORCH:
        raise TypeError(f"order_stats: dtype {x.dtype} is not uint8, uint16, int16 or float32")
    if not x.is_contiguous():
        raise ValueError("order_stats: x must be contiguous")
    ranks = [int(r) for r in ranks]
    total = x.numel()
    if n is None:
        if segments < 1 or total % segments:
            raise ValueError(f"order_stats: {total} elements do not divide into {segments} segments")
        n = total // segments
    stride = n if stride is None else int(stride)
    if segments < 1 or n < 1 or stride < 0 or (segments - 1) * stride + n > total:
        raise ValueError(f"order_stats: {segments} segments of {n} elements on a stride of {stride} do not fit {total} elements")
    if not 1 <= len(ranks) <= MAX_RANKS or any(not 0 <= r < n for r in ranks):
        raise ValueError(f"order_stats: need 1 to {MAX_RANKS} ranks inside [0, {n})")
    out = torch.empty((segments, len(ranks)), dtype=torch.float64, device=x.device)
    nan = torch.empty((1,), dtype=torch.int64, device=x.device)
    ws_bytes = lib.biu_order_stats_workspace(segments, len(ranks))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.biu_order_stats(C.c_void_p(x.data_ptr()), _ELEM_TORCH[x.dtype], segments, n, stride, (C.c_longlong * len(ranks))(*ranks),
                                  len(ranks), C.c_void_p(out.data_ptr()), C.c_void_p(nan.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes,
                                  _stream()), "order_stats")
    return (out, nan[0]) if return_nan_count else out


def _uploadable(arr: np.ndarray) -> np.ndarray:
    """The array in one of the four element types the kernels read, values unchanged -- or ``ValueError``."""
    if arr.dtype in _ELEM_NP:
        return arr
    if arr.dtype == np.bool_:
        return arr.astype(np.uint8)
    if arr.dtype == np.int8:
        return arr.astype(np.int16)
    if arr.dtype.kind not in "iuf":
        raise TypeError(f"dtype {arr.dtype} cannot be normalised")
    a32 = arr.astype(np.float32)
    if not np.array_equal(a32.astype(arr.dtype), arr, equal_nan=arr.dtype.kind == "f"):
        raise ValueError(f"{arr.dtype} input holds values float32 cannot represent exactly, and the device front end uploads it as float32: "
                         "use preprocess=\"host\"")
    return a32


class _Tiles:
    """Patches ``offset .. offset + n`` of a front end's tile list; ``batch(i, j)`` cuts, normalises and returns patches ``i:j`` as one
    device tensor ``[j - i, *view]``.  ``per`` origin records make one patch (2: the Siamese (current, previous) channel pair)."""

    def __init__(self, fe, origins, n, tile, out, invert, pad_zero, view, per=1, offset=0):
        self.fe, self.origins, self.n, self.tile, self.out, self.invert, self.pad_zero = fe, origins, n, tuple(tile), out, invert, pad_zero
        self.view, self.per, self.offset = tuple(view), per, offset
        self.shape = (n,) + self.view

    def __len__(self):
        return self.n

    def frame(self, i, count):
        return _Tiles(self.fe, self.origins, count, self.tile, self.out, self.invert, self.pad_zero, self.view, self.per, self.offset + i * count)

    def batch(self, i, j):
        j = min(j, self.n)
        if not 0 <= i < j:
            raise IndexError(f"patches {i}:{j} of {self.n}")
        fe, (td, th, tw) = self.fe, self.tile
        rec0, nrec = (self.offset + i) * self.per, (j - i) * self.per
        res = torch.empty((j - i,) + self.view, dtype=self.out, device=fe.x.device)
        assert res.numel() == nrec * td * th * tw
        with torch.cuda.device(fe.x.device):
            check(lib.biu_prep_tiles(C.c_void_p(fe.x.data_ptr()), fe.elem, fe.planes, fe.depth, fe.H, fe.W,
                                     C.c_void_p(self.origins.data_ptr() + rec0 * 16), nrec, td, th, tw, C.c_void_p(fe.scalars.data_ptr()),
                                     fe.scalars.shape[0], int(self.pad_zero), int(self.out == torch.float32), int(bool(self.invert)),
                                     C.c_void_p(res.data_ptr()), _stream()), "prep_tiles")
        return res


class DeviceFrontEnd:
    """Owns the uploaded raw stack, the per-unit scalars and the tile origins, and hands out patch batches as device tensors.

    ``stack``: ``[images, H, W]`` (``depth`` planes make one image: 1 for a 2-D stack, D for one volume) or ``[volumes, D, H, W]``.
    ``normalise(mode, clip, family)`` selects the order statistics -- per image (``'single'``), of the first image (``'first'``; minimum and
    maximum still over the whole stack, as ``a - np.min(a)`` on the host) or of the whole stack (``'all'``) -- and derives ``lo``, ``hi`` and
    the subtrahend and divisor of the family's formula; ``normalise_pairs`` does it for the Siamese predictor's (previous, current) pairs,
    all pairs in one batch.  ``tiles`` / ``pair_tiles`` then fix the tile list; nothing synchronises except the one NaN count read per
    stack for float input."""

    @staticmethod
    def native(dtype) -> bool:
        """Whether arrays of ``dtype`` are uploaded as they are (uint8, uint16, int16, float32)."""
        return np.dtype(dtype) in _ELEM_NP

    def __init__(self, stack, device, depth: int = 1):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"the device front end runs on the GPU (biu_order_stats / biu_prep_tiles); got device '{device}'. Use preprocess=\"host\".")
        arr = _uploadable(np.asarray(stack))
        if arr.ndim == 4:
            depth = arr.shape[1]
            arr = arr.reshape((-1,) + arr.shape[2:])
        if arr.ndim != 3 or arr.size == 0 or arr.shape[0] % depth:
            raise ValueError(f"Unsupported input shape: {np.asarray(stack).shape}")
        self.planes, self.H, self.W = arr.shape
        self.depth, self.n_img = depth, arr.shape[0] // depth
        self.elem = _ELEM_NP[arr.dtype]
        self.x = torch.from_numpy(np.ascontiguousarray(arr)).to(device)              # the only upload of pixels
        self.scalars, self.per_image = None, False

    # ---- statistics ----------------------------------------------------------------------------------------------
    @staticmethod
    def _ranks6(n, clip, halve=False):
        r = [0, n - 1, *percentile_ranks(float(clip[0]), n), *percentile_ranks(float(clip[1]), n)]
        return [v // 2 for v in r] if halve else r

    def _select(self, ranks, segments, n, stride=None):
        return order_stats(self.x.view(-1), ranks, segments, n, stride, return_nan_count=True)

    def _refuse_nan(self, count):
        if self.elem == ELEM_F32 and int(count.item()) > 0:            # once per stack
            raise ValueError("the input holds NaN; the device front end does not normalise around NaN: use preprocess=\"host\"")

    def _finalize(self, stats, n, clip, family):
        stats = stats.contiguous()
        assert stats.dtype == torch.float64 and stats.dim() == 2 and stats.shape[1] == 6
        self.scalars = torch.empty((stats.shape[0], 4), dtype=torch.float64, device=stats.device)
        with torch.cuda.device(stats.device):
            check(lib.biu_prep_finalize(C.c_void_p(stats.data_ptr()), stats.shape[0], n, float(clip[0]), float(clip[1]), FAMILIES[family],
                                        C.c_void_p(self.scalars.data_ptr()), _stream()), "prep_finalize")

    def normalise(self, mode: str, clip, family: str = "minmax"):
        img, total = self.depth * self.H * self.W, self.planes * self.H * self.W
        if mode == "single":
            stats, nan = self._select(self._ranks6(img, clip), self.n_img, img)
            n = img
        elif mode == "first":
            first, _ = self._select(self._ranks6(img, clip), 1, img)
            ends, nan = self._select([0, img - 1], self.n_img, img)
            stats = torch.cat([ends[:, 0].amin().view(1), ends[:, 1].amax().view(1), first[0, 2:]]).view(1, 6)
            n = img
        elif mode == "all":
            stats, nan = self._select(self._ranks6(total, clip), 1, total)
            n = total
        else:
            raise ValueError(f"normalization_mode {mode} not valid!")
        self._refuse_nan(nan)
        self.per_image = mode == "single"
        self._finalize(stats, n, clip, family)

    def normalise_pairs(self, mode: str, clip):
        """Frame i with its predecessor (frame 0 with frame 1, or with itself in a one-frame movie) as the Siamese predictor pairs them:
        ``'single'`` normalises every image by itself; ``'first'`` takes the percentiles of the previous frame and minimum / maximum of the
        pair; ``'all'`` everything from the pair.  One selection over all frames (or all two-frame windows) before the frame loop."""
        if self.depth != 1:
            raise ValueError("pairs are pairs of 2-D frames")
        T, img = self.planes, self.H * self.W
        self.prev = [(0 if T == 1 else 1) if i == 0 else i - 1 for i in range(T)]
        if mode == "single":
            stats, nan = self._select(self._ranks6(img, clip), T, img)
            n = img
        elif mode == "first":
            own, nan = self._select(self._ranks6(img, clip), T, img)
            p = torch.tensor(self.prev, device=own.device)
            stats = torch.cat([torch.minimum(own[p, 0], own[:, 0])[:, None], torch.maximum(own[p, 1], own[:, 1])[:, None], own[p, 2:]], dim=1)
            n = img
        elif mode == "all":
            n = 2 * img
            if T == 1:                                                                # the frame twice: sorted pair [j] = sorted frame [j // 2]
                stats, nan = self._select(self._ranks6(n, clip, halve=True), 1, img)
            else:                                                                     # frames i - 1 and i are one window of 2 * img elements
                win, nan = self._select(self._ranks6(n, clip), T - 1, n, stride=img)
                stats = win[torch.tensor([max(i - 1, 0) for i in range(T)], device=win.device)]
        else:
            raise ValueError(f"normalization_mode {mode} not valid!")
        self._refuse_nan(nan)
        self.per_image = mode == "single"
        self._finalize(stats, n, clip, "minmax")

    # ---- tiles ---------------------------------------------------------------------------------------------------
    def _upload_origins(self, records):
        rec = np.asarray(records, dtype=np.int64).reshape(-1, 4)
        if rec.size == 0 or rec.min() < 0 or rec.max() >= 2 ** 30 or (rec[:, 0] >= self.scalars.shape[0]).any() or (rec[:, 1] >= self.planes).any():
            raise ValueError("tile origins outside the stack")
        return torch.from_numpy(np.ascontiguousarray(rec.astype(np.int32))).to(self.x.device)

    def tiles(self, origins, tile, out: str = "uint8", invert: bool = False, view=None) -> _Tiles:
        """``origins``: (image, z, row, column) per patch, in the order the patches are wanted; ``tile``: (depth, height, width).  Beyond the
        image the tile reflects as ``np.pad(..., 'reflect')`` at the far end does.  ``out``: ``'uint8'`` (``* 255``, optional ``255 - .``,
        truncated) or ``'float32'``."""
        if self.scalars is None:
            raise RuntimeError("normalise() first")
        tile = tuple(int(t) for t in tile)
        ext = (self.depth, self.H, self.W)
        rec = []
        for i, z, y, x in origins:
            if not 0 <= i < self.n_img or any(o < 0 or o + t > max(e, t) for o, t, e in zip((z, y, x), tile, ext)):
                raise ValueError(f"tile origin {(i, z, y, x)} with tile {tile} lies outside the padded image {ext}")
            rec.append((i if self.per_image else 0, i * self.depth + z, y, x))      # (z < depth follows from the check above)
        return _Tiles(self, self._upload_origins(rec), len(rec), tile, torch.uint8 if out == "uint8" else torch.float32, invert, False,
                      view if view is not None else tile)

    def pair_tiles(self, origins, resize_dim, invert: bool = False) -> _Tiles:
        """Patches ``[2, th, tw]`` uint8 -- channel 0 the current frame, channel 1 the previous -- for every frame and every origin
        (., ., row, column), frame-major; zero beyond the image (the reference pads after normalisation).  ``.frame(i, count)`` of the
        result is frame i's patch list."""
        if self.scalars is None:
            raise RuntimeError("normalise_pairs() first")
        th, tw = (int(t) for t in resize_dim)
        rec = []
        for i in range(self.planes):
            p = self.prev[i]
            for _, _, y, x in origins:
                rec.append((i, i, y, x))
                rec.append(((p if self.per_image else i), p, y, x))
        return _Tiles(self, self._upload_origins(rec), len(rec) // 2, (1, th, tw), torch.uint8, invert, True, (2, th, tw), per=2)
