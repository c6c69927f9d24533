"""Data feed for the hot path: a memory-mapped uint8 tile store and an asynchronous host-to-device feeder.

The reference keeps every training tile as its own uint8 TIFF and ``DataProcess.__getitem__`` re-reads, decodes and divides it by
255 for every access (``unet/data.py:253-266``), with ``num_workers=0`` (``unet/train.py:92-93``): fine for a CPU that needs a
third of a second per step, a starvation hazard for eight GPUs that take ~10 ms.  Here the tiles of a data set live in ONE
flat uint8 file per field, mapped into memory:

* ``TileStore`` -- ``[N, *shape]`` uint8 arrays (``image``, ``mask``, ``prev_image``, ``volume`` ... -- the reference's item keys).  It
  is a ``torch.utils.data.Dataset`` with the reference's item contract (``float32`` in [0, 1]), so every Trainer takes it as is;
  ``TileStore.from_dataset`` converts any data set that yields such items (values are multiples of 1/255 there, so the round
  trip is exact).
* ``DeviceFeeder`` -- what the Trainers iterate when handed a ``TileStore``: a background thread gathers the next batches out of
  the page cache into pinned buffers, a side HIP stream copies them to the device as BYTES (a quarter of the float32 traffic over
  PCIe) while the current step computes, and the batch reaches the network as uint8 -- the division by 255 rides in the input-layout
  kernel (``biu_from_nchw_u8``), targets are widened by ``biu_u8_to_f32``.

Normalisation, the mask edit and tiling run once and their output is what this store holds: ``dataprep.prepare_unet`` / ``prepare_unet3d`` /
``prepare_siam`` do them on the device for the three uint8 families (TIFF decoding stays with the caller).  Augmentation does not run once: ``DeviceFeeder(..., augmenter=augment.Augmenter(...))`` augments every training batch on the device, fresh
every epoch, from a store of un-augmented tiles (``augment.py``).

The 2-D multi-output family's items are float32 (``multi_output_unet/data.py:318-349``): distance and probability maps, and an
``orientation`` target that reaches the network as ``(cos, sin)`` in [-1, 1].  A store field therefore has a dtype, ``"u8"`` (the default) or
``"f32"`` (file ``<path>.<field>.f32``, written and read back bit for bit, never scaled); the feeder carries float fields as float32 and
``augment.AugmenterF32`` (2-D) or ``augment.AugmenterVol`` (volumes) augments them.  A mixed store (``image`` as u8, targets as f32) keeps the image's PCIe traffic at a quarter.
``AugmenterF32(target_interp="cubic")`` keeps its spline scratch per field: every augmentation launch of a feeder runs on one stream, so one augmenter serves one feeder.

The reference's ``DataProcess`` of that family keeps every image WHOLE and crops at random out of the rotated image, with NaN in a target
meaning "no label here" (``multi_output_unet/data.py:140-311``).  ``ImageStore`` holds such items -- whole, of differing size, NaN kept -- and
``CropFeeder`` renders every training patch from them on the device (``biu_augment_f32_crop``); ``dataprep.prepare_mo2d`` writes one from raw
arrays.  ``VolumeStore`` is the same for the 3-D multi-output family (``multi_output_unet3d/data.py:152-230``): whole volumes, the same feeder,
``biu_augment_vol_f32_crop``, ``dataprep.prepare_mo3d``.  All three are at the end of this file.  With ``AugmenterF32(target_interp="cubic")``
an ``ImageStore`` resamples its scalar targets with the reference's cubic spline: ``ImageStore.spline_tables`` computes what depends on the
items alone once per device, ``CropFeeder(..., spline=tables)`` reads it every batch (``biu_augment_f32_crop_cubic``).
"""
from __future__ import annotations

import json
import os
import queue
import threading
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

_MAGIC = "biu-tilestore-1"
_NP_DTYPE = {"u8": np.uint8, "f32": np.float32}
_TORCH_DTYPE = {"u8": torch.uint8, "f32": torch.float32}


def _field_dtypes(fields, dtypes) -> Dict[str, str]:
    """``dtypes``: None (all uint8), one name for every field, or ``{field: "u8" | "f32"}`` (fields it does not name are uint8)."""
    if dtypes is None or isinstance(dtypes, str):
        dtypes = {k: dtypes or "u8" for k in fields}
    unknown = [k for k in dtypes if k not in fields]
    if unknown:
        raise ValueError(f"dtypes names fields the store does not have: {unknown}")
    res = {k: dtypes.get(k, "u8") for k in fields}
    for k, v in res.items():
        if v not in _NP_DTYPE:
            raise ValueError(f'field "{k}": dtype "{v}" not defined (one of {sorted(_NP_DTYPE)})')
    return res


class TileStore(torch.utils.data.Dataset):
    """Flat files ``<path>.<field>.u8`` (uint8) or ``<path>.<field>.f32`` (float32) + ``<path>.json``; fields are ``[N, *shape]``.  The
    header's ``dtypes`` map is optional: a header without it (every all-uint8 store) names uint8 fields only."""

    def __init__(self, path: str, mode: str = "r"):
        with open(path + ".json") as f:
            hdr = json.load(f)
        if hdr.get("magic") != _MAGIC:
            raise ValueError(f"{path}.json is not a tile store header")
        self.path, self.n, self.fields = path, int(hdr["n"]), {k: tuple(v) for k, v in hdr["fields"].items()}
        self.attrs = hdr.get("attrs", {})
        self.dim_out = tuple(self.attrs["dim_out"]) if "dim_out" in self.attrs else next(iter(self.fields.values()))
        for k, v in self.attrs.items():                      # aug_factor, clip_threshold, ...: the Trainers record them in checkpoints
            if k != "dim_out" and not hasattr(self, k):
                setattr(self, k, v)
        self.dtypes = _field_dtypes(self.fields, hdr.get("dtypes"))
        self.maps = {k: np.memmap(f"{path}.{k}.{self.dtypes[k]}", dtype=_NP_DTYPE[self.dtypes[k]], mode=mode, shape=(self.n,) + shp)
                     for k, shp in self.fields.items()}

    # ---- construction ----------------------------------------------------------------------------------------------
    @classmethod
    def create(cls, path: str, n: int, fields: Dict[str, Sequence[int]], attrs: Optional[dict] = None, dtypes=None) -> "TileStore":
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        dtypes = _field_dtypes(fields, dtypes)
        for k, shp in fields.items():
            np.memmap(f"{path}.{k}.{dtypes[k]}", dtype=_NP_DTYPE[dtypes[k]], mode="w+", shape=(n,) + tuple(shp)).flush()
        hdr = {"magic": _MAGIC, "n": n, "fields": {k: list(v) for k, v in fields.items()}, "attrs": attrs or {}}
        if any(v != "u8" for v in dtypes.values()):          # an all-uint8 store keeps the header every earlier reader knows
            hdr["dtypes"] = dtypes
        with open(path + ".json", "w") as f:
            json.dump(hdr, f)
        return cls(path, mode="r+")

    @classmethod
    def from_dataset(cls, path: str, dataset: Iterable, keys: Optional[Sequence[str]] = None, dtypes=None) -> "TileStore":
        """Convert a data set with the reference's item contract (dict of float32 tensors) into a store.  uint8 fields (the default) hold
        values in [0, 1] as multiples of 1/255; ``dtypes`` (``"f32"`` for every field, or ``{field: "u8" | "f32"}``) names the fields that
        are written as the data set yields them: no clipping, no rounding.  Non-finite values are refused: the store holds what
        ``DataProcess.__getitem__`` yields, i.e. NaN already replaced by ``nan_to_val``."""
        first = dataset[0]
        keys = list(keys) if keys is not None else [k for k, v in first.items() if torch.is_tensor(v) or isinstance(v, np.ndarray)]
        fields = {k: tuple(np.asarray(first[k]).shape) for k in keys}
        attrs = {}
        for a in ("dim_out", "aug_factor", "clip_threshold", "noise_lims", "noise_amp", "brightness_contrast", "shiftscalerotate", "blur_limit",
                  "gauss_noise_lims", "shot_noise_lims", "random_rotate", "scale_limit", "rotate_limit"):
            if hasattr(dataset, a):
                v = getattr(dataset, a)
                attrs[a] = list(v) if isinstance(v, (tuple, list)) else v
        st = cls.create(path, len(dataset), fields, attrs, dtypes)
        for i in range(len(dataset)):
            item = dataset[i]
            for k in keys:
                if st.dtypes[k] == "f32":
                    v = np.asarray(item[k], dtype=np.float32)
                    if not np.isfinite(v).all():
                        raise ValueError(f'field "{k}" of item {i} holds non-finite values: replace NaN (nan_to_val) before the store is written')
                    st.maps[k][i] = v
                else:
                    st.maps[k][i] = np.clip(np.rint(np.asarray(item[k], dtype=np.float64) * 255.0), 0, 255).astype(np.uint8)
        st.flush()
        return st

    def flush(self):
        for m in self.maps.values():
            m.flush()

    # ---- Dataset contract of the reference: float32 (uint8 fields: in [0, 1]; float fields: as written) --------------
    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {k: torch.from_numpy(np.array(m[i], dtype=np.float32) if self.dtypes[k] == "f32" else np.asarray(m[i], dtype=np.float32) / 255.0)
                for k, m in self.maps.items()}

    def batch_u8(self, indices, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Batch ``{field: [B, *shape]}`` in the fields' own dtypes (uint8, or float32 for float fields), gathered from the map (into
        ``out``'s tensors when given, e.g. pinned buffers).  ``batch_host`` is the same method under a dtype-neutral name."""
        idx = np.asarray(indices, dtype=np.int64)
        res = {}
        for k, m in self.maps.items():
            if out is not None:
                dst = out[k][:len(idx)]
                np.take(m, idx, axis=0, out=dst.numpy())
                res[k] = dst
            else:
                res[k] = torch.from_numpy(np.take(m, idx, axis=0))
        return res

    batch_host = batch_u8


class DeviceFeeder:
    """Iterable over device batches of a ``TileStore`` in the fields' own dtypes (one epoch per ``iter()``), ``depth`` batches in flight.

    With an ``augmenter`` (``augment.Augmenter``) the feeder thread also draws the per-sample parameter records, uploads them with the batch
    and enqueues the augmentation launches on the copy stream in front of the ``ready`` event, into a second set of device buffers: the work
    overlaps the running step exactly as the upload does.  ``epoch`` (the second argument of ``Augmenter.draw``) advances per ``iter()``.
    ``augment_stream="main"`` enqueues the launches on the consumer's stream at hand-over instead (same bytes; for A/B measurements of how
    the augmentation kernels share the device with the step, ``tools/bench_augment.py``)."""

    def __init__(self, store: TileStore, indices: Sequence[int], batch_size: int, device, drop_last: bool = True, depth: int = 3,
                 augmenter=None, augment_stream: str = "copy"):
        self.store, self.indices, self.batch_size = store, list(indices), batch_size
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"DeviceFeeder copies to a GPU; got device '{device}'")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.drop_last, self.depth = drop_last, max(2, depth)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        dtypes = {k: _TORCH_DTYPE[v] for k, v in getattr(store, "dtypes", {k: "u8" for k in store.fields}).items()}
        mk = lambda k, pin, dt=None: (torch.empty((batch_size,) + store.fields[k], dtype=dt or dtypes[k]).pin_memory() if pin
                                      else torch.empty((batch_size,) + store.fields[k], dtype=dt or dtypes[k], device=self.device))
        self.slots = [{"host": {k: mk(k, True) for k in store.fields}, "dev": {k: mk(k, False) for k in store.fields},
                       "ready": None, "free": None, "released": threading.Event()} for _ in range(self.depth)]
        if augment_stream not in ("copy", "main"):
            raise ValueError('augment_stream: "copy" or "main"')
        self.augmenter, self.epoch, self.augment_on_main = augmenter, 0, augment_stream == "main"
        if augmenter is not None:
            out_dtype = augmenter.dst_dtype                                  # augment.AugmenterF32 writes float32 whatever the field holds
            if out_dtype == torch.uint8 and any(dt != torch.uint8 for dt in dtypes.values()):
                raise ValueError("a store with float fields needs augment.AugmenterF32 or AugmenterVol (augment.Augmenter works on uint8 fields)")
            rec = augmenter.params_dtype.itemsize
            for slot in self.slots:
                slot["aug"] = {k: mk(k, False, out_dtype) for k in store.fields}
                slot["params_host"] = torch.empty(batch_size * rec, dtype=torch.uint8).pin_memory()
                slot["params_dev"] = torch.empty(batch_size * rec, dtype=torch.uint8, device=self.device)

    def __len__(self):
        n = len(self.indices)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        batches = [self.indices[i:i + self.batch_size] for i in range(0, len(self.indices), self.batch_size)]
        if self.drop_last:
            batches = [b for b in batches if len(b) == self.batch_size]
        filled: "queue.Queue" = queue.Queue(maxsize=self.depth - 1)
        epoch, out_key = self.epoch, "dev" if self.augmenter is None else "aug"
        self.epoch += 1
        stop = threading.Event()
        for slot in self.slots:
            slot["released"].set()
            slot["free"] = None

        def producer():
            try:
                produce()
            except BaseException as e:                       # surface a failure of the feeder thread in the training thread
                filled.put(e)

        def produce():
            # gather (page cache -> pinned memory) and enqueue the asynchronous upload; never blocks the training thread
            torch.cuda.set_device(self.device)
            for bi, idx in enumerate(batches):
                slot = self.slots[bi % self.depth]
                slot["released"].wait()                     # the consumer has handed the slot back ...
                slot["released"].clear()
                if stop.is_set():
                    break
                if slot["free"] is not None:
                    slot["free"].synchronize()              # ... and the step that read its device buffers has finished on the GPU
                self.store.batch_u8(idx, out=slot["host"])
                if self.augmenter is not None:
                    params = self.augmenter.draw(epoch, idx, shape=next(iter(self.store.fields.values())))
                    nbytes = params.nbytes
                    slot["params_host"][:nbytes].numpy()[:] = params.view(np.uint8)
                with torch.cuda.stream(self.copy_stream):
                    for k in slot["host"]:
                        slot["dev"][k][:len(idx)].copy_(slot["host"][k][:len(idx)], non_blocking=True)
                    if self.augmenter is not None:
                        slot["params_dev"][:nbytes].copy_(slot["params_host"][:nbytes], non_blocking=True)
                        slot["params"] = params
                    if self.augmenter is not None and not self.augment_on_main:
                        self.augmenter({k: v[:len(idx)] for k, v in slot["dev"].items()}, params, epoch,
                                       out={k: v[:len(idx)] for k, v in slot["aug"].items()}, params_dev=slot["params_dev"])
                    ev = torch.cuda.Event()
                    ev.record(self.copy_stream)
                slot["ready"] = ev
                filled.put((bi, len(idx)))
            filled.put(None)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        try:
            while True:
                item = filled.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise RuntimeError("DeviceFeeder: the feeder thread failed") from item
                bi, nb = item
                slot = self.slots[bi % self.depth]
                torch.cuda.current_stream(self.device).wait_event(slot["ready"])     # device-side wait: the host does not block
                if self.augmenter is not None and self.augment_on_main:
                    self.augmenter({k: v[:nb] for k, v in slot["dev"].items()}, slot["params"], epoch,
                                   out={k: v[:nb] for k, v in slot["aug"].items()}, params_dev=slot["params_dev"])
                yield {k: v[:nb] for k, v in slot[out_key].items()}
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(self.device))                  # everything enqueued so far read the slot
                slot["free"] = done
                slot["released"].set()
        finally:
            stop.set()
            for slot in self.slots:
                slot["released"].set()
            while th.is_alive():
                try:
                    filled.get(timeout=0.05)
                except queue.Empty:
                    pass
            th.join()


# =====================================================================================================================================
# whole items: the 2-D multi-output family's DataProcess (``multi_output_unet/data.py:140-311``)
# =====================================================================================================================================
_IMAGE_MAGIC = "biu-imagestore-1"
_ITEM_LIMIT = 2 ** 31 - 4                     # planes * H * W of one item: the crop kernel's index math inside an item is 32-bit


def patches_of(h: int, w: int, dim_out, aug_factor) -> int:
    """The reference's number of crops per image: ``max(int(H W / (dh dw) * aug_factor), 2)`` (``multi_output_unet/data.py:258-259``)."""
    return max(int((h * w) / (dim_out[0] * dim_out[1]) * aug_factor), 2)


class ImageStore(torch.utils.data.Dataset):
    """Whole items of differing size: per field one flat file ``<path>.<field>.f32`` / ``.u8`` (``TileStore``'s naming) that holds the items
    one after the other, each ``[planes, H_i, W_i]``, and the header ``<path>.json`` (magic ``biu-imagestore-1``) with the planes and dtype
    of every field, ``(H_i, W_i)`` of every item and ``attrs`` (``dim_out``, ``aug_factor``, ``nan_to_val``, ``clip_threshold`` and the
    augmentation limits ``AugmenterF32.store_attrs`` lists).

    Float fields may hold NaN ("no label here"), written and read back bit for bit; the field ``image`` may not.  Its length is the number
    of PATCHES per epoch, the reference's count per item (``patches_of``) summed; ``locate(j)`` maps a patch index to its item.  Patches are
    rendered on the device only (``CropFeeder`` / ``biu_augment_f32_crop``): ``__getitem__`` raises.  ``fields`` is the shape of a rendered
    patch per field, as ``TileStore.fields`` is the shape of a tile."""
    recipe = "mo2d"                              # the augmenter that draws its crops: augment.AugmenterF32

    def __init__(self, path: str, mode: str = "r"):
        with open(path + ".json") as f:
            hdr = json.load(f)
        if hdr.get("magic") != _IMAGE_MAGIC:
            raise ValueError(f"{path}.json is not an image store header")
        self.path, self.attrs = path, hdr.get("attrs", {})
        self.sizes = np.asarray(hdr["items"], dtype=np.int64).reshape(-1, 2)
        self.n_items = len(self.sizes)
        self.planes = {k: int(v["planes"]) for k, v in hdr["fields"].items()}
        self.dtypes = {k: v["dtype"] for k, v in hdr["fields"].items()}
        self.squeeze = {k: bool(v.get("squeeze", False)) for k, v in hdr["fields"].items()}
        self.dim_out = tuple(int(d) for d in self.attrs["dim_out"])
        self.aug_factor = self.attrs.get("aug_factor", 2)
        self.nan_to_val = float(self.attrs.get("nan_to_val", 0.0))
        for k, v in self.attrs.items():
            if not hasattr(self, k):
                setattr(self, k, v)
        self.fields = {k: self.dim_out if self.squeeze[k] else (p,) + self.dim_out for k, p in self.planes.items()}
        pixels = self.sizes[:, 0] * self.sizes[:, 1]
        start = np.concatenate([[0], np.cumsum(pixels)])
        self.offsets = {k: start[:-1] * p for k, p in self.planes.items()}          # element offset of every item in its field's file
        self.elements = {k: int(start[-1]) * p for k, p in self.planes.items()}
        self.counts = np.asarray([patches_of(int(h), int(w), self.dim_out, self.aug_factor) for h, w in self.sizes], dtype=np.int64)
        self._ends = np.cumsum(self.counts)
        self.maps = {k: np.memmap(f"{path}.{k}.{self.dtypes[k]}", dtype=_NP_DTYPE[self.dtypes[k]], mode=mode, shape=(self.elements[k],))
                     for k in self.planes}

    # ---- construction ----------------------------------------------------------------------------------------------
    @classmethod
    def create(cls, path: str, sizes, fields: Dict[str, int], attrs: dict, dtypes=None, squeeze: Optional[Dict[str, bool]] = None) -> "ImageStore":
        """An empty store for items of the extents ``sizes`` ``[(H_i, W_i)]``; ``fields``: planes per field; ``attrs`` needs ``dim_out``.
        ``squeeze``: fields whose patches are handed out without the plane axis (one plane, given as ``[H, W]``)."""
        sizes = [(int(h), int(w)) for h, w in sizes]
        if not sizes or not fields or any(h < 1 or w < 1 for h, w in sizes) or any(int(p) < 1 for p in fields.values()):
            raise ValueError("an image store needs items and fields of positive extent")
        if "dim_out" not in (attrs or {}) or len(attrs["dim_out"]) != 2 or min(attrs["dim_out"]) < 1:
            raise ValueError("attrs needs dim_out = (height, width) of a patch")
        for name, p in fields.items():
            for i, (h, w) in enumerate(sizes):
                if int(p) * h * w >= _ITEM_LIMIT:
                    raise ValueError(f'field "{name}" of item {i}: {p} x {h} x {w} elements; one item holds fewer than 2^31 - 4 per field')
        dtypes = _field_dtypes(fields, dtypes if dtypes is not None else "f32")
        squeeze = {k: bool((squeeze or {}).get(k, False)) and int(fields[k]) == 1 for k in fields}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        total = sum(h * w for h, w in sizes)
        for k, p in fields.items():
            np.memmap(f"{path}.{k}.{dtypes[k]}", dtype=_NP_DTYPE[dtypes[k]], mode="w+", shape=(total * int(p),)).flush()
        plain = lambda v: [plain(e) for e in v] if isinstance(v, (tuple, list)) else v
        hdr = {"magic": _IMAGE_MAGIC, "items": [list(s) for s in sizes], "attrs": {k: plain(v) for k, v in attrs.items()},
               "fields": {k: {"planes": int(p), "dtype": dtypes[k], "squeeze": squeeze[k]} for k, p in fields.items()}}
        with open(path + ".json", "w") as f:
            json.dump(hdr, f)
        return cls(path, mode="r+")

    def item(self, i: int, name: str) -> np.ndarray:
        """Item ``i`` of field ``name`` as a view ``[planes, H_i, W_i]`` of the map."""
        h, w = (int(v) for v in self.sizes[i])
        o, p = int(self.offsets[name][i]), self.planes[name]
        return self.maps[name][o:o + p * h * w].reshape(p, h, w)

    def put(self, i: int, name: str, value) -> None:
        """Write item ``i`` of field ``name``: float fields as given (NaN kept, bit for bit), except that the field ``image`` is refused where
        it is not finite; uint8 fields take bytes, or floats in [0, 1] as multiples of 1/255."""
        dst = self.item(i, name)
        v = np.asarray(value)
        v = v[None] if v.ndim == 2 else v
        if v.shape != dst.shape:
            raise ValueError(f'field "{name}" of item {i}: expected {dst.shape}, got {v.shape}')
        if name == "image" and v.dtype.kind == "f" and not np.isfinite(v).all():
            raise ValueError(f'field "image" of item {i} holds non-finite values: NaN means "no label" and is for targets only')
        if self.dtypes[name] == "f32":
            dst[...] = v.astype(np.float32, copy=False)
        elif v.dtype == np.uint8:
            dst[...] = v
        else:
            dst[...] = np.clip(np.rint(v.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)

    def flush(self):
        for m in self.maps.values():
            m.flush()

    # ---- Dataset contract: patches per epoch -------------------------------------------------------------------------
    def __len__(self):
        return int(self._ends[-1])

    def locate(self, j):
        """Item of patch ``j`` (an index or an array of indices): patches ``0 .. counts[0] - 1`` come from item 0, and so on."""
        idx = np.asarray(j, dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(f"patch index outside 0 .. {len(self) - 1}")
        res = np.searchsorted(self._ends, idx, side="right")
        return int(res) if res.ndim == 0 else res

    def __getitem__(self, j):
        raise RuntimeError("ImageStore: patches are rendered on the device only (feed.CropFeeder, biu_augment_f32_crop); there is no CPU path")

    def to_device(self, device):
        """Upload every field once as ONE device tensor (the arena).  Returns ``(arenas {field: 1-D tensor}, offsets {field: int64 [items]},
        H [items], W [items])`` (a ``VolumeStore``: ``D, H, W``); the offsets count elements of the field's own arena.  A store that does not fit raises ``RuntimeError``.
        The upload happens once per device and is kept (a ``put`` after it is not seen there)."""
        extents = (self.sizes[:, a].copy() for a in range(self.sizes.shape[1]))       # H, W (a VolumeStore: D, H, W)
        return (self._arenas_on(device), {k: v.astype(np.int64) for k, v in self.offsets.items()}, *extents)

    def _arenas_on(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}.to_device uploads to a GPU; got device '{device}'")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        cache = self.__dict__.setdefault("_arenas", {})      # the training and the validation feeder of a Trainer share one upload
        if device not in cache:
            cache[device] = self._upload(device)
        return cache[device]

    def _upload(self, device):
        arenas = {}
        try:
            for k, m in self.maps.items():
                arenas[k] = torch.from_numpy(np.ascontiguousarray(m)).to(device)
        except torch.cuda.OutOfMemoryError as e:
            need = sum(self.elements[k] * (1 if self.dtypes[k] == "u8" else 4) for k in self.maps)
            arenas.clear()
            raise RuntimeError(f"{type(self).__name__} {self.path}: the store ({need} bytes) does not fit in the HBM of {device}; a streamed store is not "
                               f"supported") from e
        return arenas

    def spline_tables(self, device, names) -> Dict[str, "SplineTables"]:
        """What ``AugmenterF32(target_interp="cubic")`` needs of the fields ``names`` (its "mask" fields: ``AugmenterF32.spline_fields(store)``)
        to resample them with the reference's cubic spline: per field a ``SplineTables`` on ``device`` -- the coefficients of the periodic
        cubic B-spline through every item (NaN read as 0) in an fp32 arena with the field arena's layout, the same through ``isnan(item)``
        if some item of the field holds a NaN (else no second arena), and per item its value range and whether it holds a NaN
        (``biu_spline_prefilter_items``, ``include/biu.h``).  They depend on the items alone, so they are computed once per (store, device)
        after ``to_device`` and kept as the arenas are: the feeders of a Trainer share them (hand the result to ``CropFeeder(..., spline=)``).
        They cost HBM: 4 bytes per element of the field, twice that with NaN; tables that do not fit raise ``RuntimeError``."""
        if self.sizes.shape[1] != 2:
            raise NotImplementedError(f"{type(self).__name__}: cubic-spline tables exist for 2-D items only (the reference resamples 3-D masks nearest)")
        arenas = self._arenas_on(device)
        device = next(iter(arenas.values())).device
        cache = self.__dict__.setdefault("_splines", {}).setdefault(device, {})
        for name in names:
            if name not in arenas:
                raise KeyError(f'{type(self).__name__} {self.path} has no field "{name}"')
            if name not in cache:
                cache[name] = SplineTables.build(arenas[name], self.planes[name], self.offsets[name], self.sizes, f'{self.path} field "{name}"')
        return {name: cache[name] for name in names}


SPLINE_ITEM_DTYPE = np.dtype([("lo", "<f4"), ("hi", "<f4"), ("has_nan", "<u4"), ("reserved", "<u4")])       # include/biu.h: biu_spline_item


class SplineTables:
    """The cubic-spline tables of one field of an ``ImageStore`` on one device (``ImageStore.spline_tables``): ``coef`` (float32, the
    arena's layout), ``indicator`` (the same, or ``None`` if no item holds a NaN), ``table`` (device bytes: one ``biu_spline_item`` per
    item) and its host copy ``items`` (``SPLINE_ITEM_DTYPE``: ``lo``, ``hi``, ``has_nan``)."""

    def __init__(self, coef, indicator, table, items):
        self.coef, self.indicator, self.table, self.items, self.n_items = coef, indicator, table, items, len(items)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.coef, self.indicator, self.table) if t is not None)

    @classmethod
    def build(cls, arena: torch.Tensor, planes: int, offsets, sizes, what: str = "arena") -> "SplineTables":
        """Run ``biu_spline_prefilter_items`` on the 1-D device tensor ``arena`` (float32 or uint8) whose items ``[planes, h_i, w_i]`` start at
        the element ``offsets``; ``sizes [items, 2]``.  The indicator arena is allocated only after the table says that some item has a NaN."""
        import ctypes as C
        from ._lib import check, lib
        from .augment import SOURCE_DTYPE
        if not arena.is_cuda or arena.dim() != 1 or not arena.is_contiguous() or arena.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"{what}: the arena is a contiguous 1-D float32 or uint8 device tensor")
        n, sizes = len(offsets), np.asarray(sizes)
        src = np.empty(n, dtype=SOURCE_DTYPE)
        src["offset"], src["h"], src["w"] = np.asarray(offsets), sizes[:, 0], sizes[:, 1]
        stream = C.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)
        need = arena.numel() * 4

        def alloc():
            try:
                return torch.empty(arena.numel(), dtype=torch.float32, device=arena.device)
            except torch.cuda.OutOfMemoryError as e:
                raise RuntimeError(f"{what}: a cubic-spline table ({need} bytes; two of them if the field holds NaN) does not fit in the HBM of "
                                   f"{arena.device}") from e

        def run(coef, indicator):
            check(lib.biu_spline_prefilter_items(C.c_void_p(arena.data_ptr()), int(arena.dtype == torch.uint8), arena.numel(),
                                                 C.c_void_p(coef.data_ptr()) if coef is not None else None,
                                                 C.c_void_p(indicator.data_ptr()) if indicator is not None else None, C.c_void_p(table.data_ptr()),
                                                 n, int(planes), src.ctypes.data_as(C.c_void_p), stream), "spline_prefilter_items")

        with torch.cuda.device(arena.device):
            coef, table = alloc(), torch.empty(n * SPLINE_ITEM_DTYPE.itemsize, dtype=torch.uint8, device=arena.device)
            run(coef, None)
            items = table.cpu().numpy().view(SPLINE_ITEM_DTYPE).copy()             # synchronises: the table is complete
            indicator = None
            if items["has_nan"].any():
                indicator = alloc()
                run(None, indicator)
                torch.cuda.current_stream(arena.device).synchronize()              # the feeders read the tables on streams of their own
        return cls(coef, indicator, table, items)


_VOLUME_MAGIC = "biu-volumestore-1"


class VolumeStore(ImageStore):
    """``ImageStore`` for whole VOLUMES of differing size ``(D_i, H_i, W_i)``: the same file layout (one flat file per field, the items one
    after the other, each ``[channels, D_i, H_i, W_i]``; header magic ``biu-volumestore-1``) and the same API.  ``attrs`` holds a 3-tuple
    ``dim_out``, an integer ``aug_factor``, ``nan_to_val``, ``clip_threshold`` and the limits ``AugmenterVol.store_attrs`` lists.

    Float fields may hold NaN ("no label here"), written and read back bit for bit; the field ``volume`` may not.  Its length is
    ``n_items * aug_factor`` -- the reference draws ``aug_factor`` patches per volume (``multi_output_unet3d/data.py:192``) -- and
    ``locate(j) = j // aug_factor``.  Patches are rendered on the device only (``CropFeeder`` / ``biu_augment_vol_f32_crop``): ``__getitem__``
    raises.  ``planes`` is the number of channels per field, ``fields`` the shape of a rendered patch."""
    recipe = "mo3d"                              # augment.AugmenterVol

    def __init__(self, path: str, mode: str = "r"):
        with open(path + ".json") as f:
            hdr = json.load(f)
        if hdr.get("magic") != _VOLUME_MAGIC:
            raise ValueError(f"{path}.json is not a volume store header")
        self.path, self.attrs = path, hdr.get("attrs", {})
        self.sizes = np.asarray(hdr["items"], dtype=np.int64).reshape(-1, 3)
        self.n_items = len(self.sizes)
        self.planes = {k: int(v["channels"]) for k, v in hdr["fields"].items()}
        self.dtypes = {k: v["dtype"] for k, v in hdr["fields"].items()}
        self.squeeze = {k: bool(v.get("squeeze", False)) for k, v in hdr["fields"].items()}
        self.dim_out = tuple(int(d) for d in self.attrs["dim_out"])
        self.aug_factor = int(self.attrs.get("aug_factor", 10))
        self.nan_to_val = float(self.attrs.get("nan_to_val", 0.0))
        for k, v in self.attrs.items():
            if not hasattr(self, k):
                setattr(self, k, v)
        self.fields = {k: self.dim_out if self.squeeze[k] else (c,) + self.dim_out for k, c in self.planes.items()}
        start = np.concatenate([[0], np.cumsum(self.sizes.prod(axis=1))])
        self.offsets = {k: start[:-1] * c for k, c in self.planes.items()}          # element offset of every item in its field's file
        self.elements = {k: int(start[-1]) * c for k, c in self.planes.items()}
        self.maps = {k: np.memmap(f"{path}.{k}.{self.dtypes[k]}", dtype=_NP_DTYPE[self.dtypes[k]], mode=mode, shape=(self.elements[k],))
                     for k in self.planes}

    @classmethod
    def create(cls, path: str, sizes, fields: Dict[str, int], attrs: dict, dtypes=None, squeeze: Optional[Dict[str, bool]] = None) -> "VolumeStore":
        """An empty store for items of the extents ``sizes`` ``[(D_i, H_i, W_i)]``; ``fields``: channels per field; ``attrs`` needs ``dim_out``
        (3 extents).  ``squeeze``: fields whose patches are handed out without the channel axis (one channel, given as ``[D, H, W]``).  An
        item smaller than ``dim_out`` in any axis is refused (``RandomCrop3D`` would raise there)."""
        sizes = [tuple(int(v) for v in sz) for sz in sizes]
        if not sizes or not fields or any(len(sz) != 3 or min(sz) < 1 for sz in sizes) or any(int(c) < 1 for c in fields.values()):
            raise ValueError("a volume store needs items (D, H, W) and fields of positive extent")
        if "dim_out" not in (attrs or {}) or len(attrs["dim_out"]) != 3 or min(attrs["dim_out"]) < 1:
            raise ValueError("attrs needs dim_out = (depth, height, width) of a patch")
        if int(attrs.get("aug_factor", 10)) != attrs.get("aug_factor", 10) or int(attrs.get("aug_factor", 10)) < 1:
            raise ValueError("aug_factor: a whole number of patches per volume, at least 1")
        dim_out = tuple(int(d) for d in attrs["dim_out"])
        for i, sz in enumerate(sizes):
            if any(e < t for e, t in zip(sz, dim_out)):
                raise ValueError(f"item {i}: {sz} is smaller than dim_out {dim_out}; a crop cannot be larger than its volume")
            for name, c in fields.items():
                if int(c) * sz[0] * sz[1] * sz[2] >= _ITEM_LIMIT:
                    raise ValueError(f'field "{name}" of item {i}: {c} x {sz[0]} x {sz[1]} x {sz[2]} elements; one item holds fewer than 2^31 - 4 per field')
        dtypes = _field_dtypes(fields, dtypes if dtypes is not None else "f32")
        squeeze = {k: bool((squeeze or {}).get(k, False)) and int(fields[k]) == 1 for k in fields}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        total = sum(d * h * w for d, h, w in sizes)
        for k, c in fields.items():
            np.memmap(f"{path}.{k}.{dtypes[k]}", dtype=_NP_DTYPE[dtypes[k]], mode="w+", shape=(total * int(c),)).flush()
        plain = lambda v: [plain(e) for e in v] if isinstance(v, (tuple, list)) else v
        hdr = {"magic": _VOLUME_MAGIC, "items": [list(sz) for sz in sizes], "attrs": {k: plain(v) for k, v in attrs.items()},
               "fields": {k: {"channels": int(c), "dtype": dtypes[k], "squeeze": squeeze[k]} for k, c in fields.items()}}
        with open(path + ".json", "w") as f:
            json.dump(hdr, f)
        return cls(path, mode="r+")

    def item(self, i: int, name: str) -> np.ndarray:
        """Item ``i`` of field ``name`` as a view ``[channels, D_i, H_i, W_i]`` of the map."""
        d, h, w = (int(v) for v in self.sizes[i])
        o, c = int(self.offsets[name][i]), self.planes[name]
        return self.maps[name][o:o + c * d * h * w].reshape(c, d, h, w)

    def put(self, i: int, name: str, value) -> None:
        """Write item ``i`` of field ``name``: float fields as given (NaN kept, bit for bit), except that the field ``volume`` is refused where
        it is not finite; uint8 fields take bytes, or floats in [0, 1] as multiples of 1/255."""
        dst = self.item(i, name)
        v = np.asarray(value)
        v = v[None] if v.ndim == 3 else v
        if v.shape != dst.shape:
            raise ValueError(f'field "{name}" of item {i}: expected {dst.shape}, got {v.shape}')
        if name == "volume" and v.dtype.kind == "f" and not np.isfinite(v).all():
            raise ValueError(f'field "volume" of item {i} holds non-finite values: NaN means "no label" and is for targets only')
        if self.dtypes[name] == "f32":
            dst[...] = v.astype(np.float32, copy=False)
        elif v.dtype == np.uint8:
            dst[...] = v
        else:
            dst[...] = np.clip(np.rint(v.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)

    def __len__(self):
        return self.n_items * self.aug_factor

    def locate(self, j):
        """Item of patch ``j`` (an index or an array of indices): ``j // aug_factor``."""
        idx = np.asarray(j, dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(f"patch index outside 0 .. {len(self) - 1}")
        res = idx // self.aug_factor
        return int(res) if res.ndim == 0 else res

    def __getitem__(self, j):
        raise RuntimeError("VolumeStore: patches are rendered on the device only (feed.CropFeeder, biu_augment_vol_f32_crop); there is no CPU path")


class CropFeeder:
    """Iterable over device batches of random crops out of an ``ImageStore`` or a ``VolumeStore`` (one epoch per ``iter()``), ``depth`` batches
    in flight: what the Trainer iterates when handed such a store.  The store is uploaded once (``to_device``); per batch a background thread
    draws the records and sources (``AugmenterF32.draw_crops`` / ``AugmenterVol.draw_crops``), uploads the two small buffers on a copy stream
    and launches one ``biu_augment_f32_crop`` / ``biu_augment_vol_f32_crop`` per field (the augmenter's ``launch_crop``) into rotating output
    buffers in front of a ``ready`` event -- ``DeviceFeeder``'s slot and event hand-over,
    a failure of the feeder thread surfaces in the consumer.  No tile bytes cross PCIe after the upload.

    ``spline``: ``store.spline_tables(device, augmenter.spline_fields(store))``, required by ``AugmenterF32(target_interp="cubic")`` (without
    it that augmenter raises ``NotImplementedError`` here): "mask" fields of batches with an arbitrary-angle record are then rendered by
    ``biu_augment_f32_crop_cubic``; the feeder uploads the item index of every patch behind the sources.

    ``epoch_key``: ``None`` -- the epoch (``draw_crops``' second argument) advances per ``iter()``; a number -- every ``iter()`` uses it, so the
    batches are the same every time (the Trainer's validation feeder: ``augment.VALIDATION_EPOCH``)."""

    def __init__(self, store: ImageStore, patch_indices: Sequence[int], batch_size: int, device, augmenter, epoch_key: Optional[int] = None,
                 depth: int = 3, drop_last: bool = True, spline: Optional[Dict[str, "SplineTables"]] = None):
        self.store, self.indices, self.batch_size = store, [int(i) for i in patch_indices], int(batch_size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"CropFeeder renders on a GPU; got device '{device}'")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if augmenter is None or not hasattr(augmenter, "draw_crops"):
            raise ValueError("CropFeeder needs an augment.AugmenterF32 (ImageStore) or augment.AugmenterVol (VolumeStore): such a store cannot "
                             "be read un-augmented")
        if augmenter.recipe != store.recipe:
            raise ValueError(f'{type(augmenter).__name__} (recipe "{augmenter.recipe}") does not draw crops out of a {type(store).__name__}')
        self.spline = None
        if getattr(augmenter, "target_interp", "linear") == "cubic":
            # the tables are HBM of the store's, up to twice the field's arena, shared by its feeders: the caller asks for them as for to_device
            if spline is None:
                raise NotImplementedError('target_interp="cubic" on an ImageStore needs the store\'s spline tables: pass '
                                          'spline=store.spline_tables(device, augmenter.spline_fields(store)), as workflow._loaders does')
            missing = [k for k in augmenter.spline_fields(store) if k not in spline]
            if missing:
                raise ValueError(f'target_interp="cubic": no spline tables for the field(s) {missing}')
            self.spline = dict(spline)
        self.augmenter, self.epoch_key, self.epoch = augmenter, epoch_key, 0
        self.drop_last, self.depth = drop_last, max(2, depth)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.arenas, self.offsets = store.to_device(self.device)[:2]
        self.names = list(store.fields)
        # what is store-specific: the patch extent (2 or 3 axes) and the size of a source record; draw_crops and launch_crop are the augmenter's
        rec, src = augmenter.params_dtype.itemsize, augmenter.source_dtype.itemsize
        self._rec_bytes, self._src_bytes = batch_size * rec, batch_size * src
        small = self._rec_bytes + len(self.names) * self._src_bytes                  # records, then one block of sources per field
        self._idx_off = small                                                          # cubic targets: then the item of every patch (int32)
        if self.spline is not None:
            small += batch_size * 4
        self.slots = [{"out": {k: torch.empty((batch_size, store.planes[k], *store.dim_out), dtype=torch.float32, device=self.device) for k in self.names},
                       "host": torch.empty(small, dtype=torch.uint8).pin_memory(),
                       "dev": torch.empty(small, dtype=torch.uint8, device=self.device),
                       "ready": None, "free": None, "released": threading.Event()} for _ in range(self.depth)]

    def __len__(self):
        n = len(self.indices)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _view(self, slot, nb):
        return {k: (v[:nb, 0] if self.store.squeeze[k] else v[:nb]) for k, v in slot["out"].items()}

    def __iter__(self):
        blur_flag = self.augmenter.blur_flag
        batches = [self.indices[i:i + self.batch_size] for i in range(0, len(self.indices), self.batch_size)]
        if self.drop_last:
            batches = [b for b in batches if len(b) == self.batch_size]
        filled: "queue.Queue" = queue.Queue(maxsize=self.depth - 1)
        epoch = self.epoch if self.epoch_key is None else int(self.epoch_key)
        self.epoch += 1
        stop = threading.Event()
        for slot in self.slots:
            slot["released"].set()
            slot["free"] = None
        nan_to_val = self.store.nan_to_val
        rot_flag = getattr(self.augmenter, "rot_flag", 0)

        def producer():
            try:
                produce()
            except BaseException as e:                       # surface a failure of the feeder thread in the training thread
                filled.put(e)

        def produce():
            torch.cuda.set_device(self.device)
            for bi, idx in enumerate(batches):
                slot = self.slots[bi % self.depth]
                slot["released"].wait()
                slot["released"].clear()
                if stop.is_set():
                    break
                if slot["free"] is not None:
                    slot["free"].synchronize()              # the step that read the slot's output buffers has finished on the GPU
                params, sources = self.augmenter.draw_crops(epoch, idx, self.store, self.offsets)
                nb, host = len(idx), slot["host"].numpy()
                host[:params.nbytes] = params.view(np.uint8)
                for f, k in enumerate(self.names):
                    o = self._rec_bytes + f * self._src_bytes
                    host[o:o + sources[k].nbytes] = sources[k].view(np.uint8)
                blurs = params["blur_k"][(params["flags"] & blur_flag) != 0]
                max_blur = int(blurs.max()) if len(blurs) else 0
                cubic = {}
                if self.spline is not None and bool((params["flags"] & rot_flag).any()):      # read from the records, as max_blur is
                    host[self._idx_off:self._idx_off + 4 * nb] = self.store.locate(idx).astype(np.int32).view(np.uint8)
                    cubic = {"item_index_dev": slot["dev"][self._idx_off:self._idx_off + 4 * nb]}
                with torch.cuda.stream(self.copy_stream):
                    slot["dev"].copy_(slot["host"], non_blocking=True)
                    for f, k in enumerate(self.names):
                        o = self._rec_bytes + f * self._src_bytes
                        self.augmenter.launch_crop(k, self.arenas[k], slot["out"][k][:nb], slot["dev"][:self._rec_bytes],
                                                   slot["dev"][o:o + self._src_bytes], nan_to_val, max_blur, epoch,
                                                   **({"spline": self.spline[k], **cubic} if cubic and k in self.spline else {}))
                    ev = torch.cuda.Event()
                    ev.record(self.copy_stream)
                slot["ready"] = ev
                filled.put((bi, nb))
            filled.put(None)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        try:
            while True:
                item = filled.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise RuntimeError("CropFeeder: the feeder thread failed") from item
                bi, nb = item
                slot = self.slots[bi % self.depth]
                torch.cuda.current_stream(self.device).wait_event(slot["ready"])     # device-side wait: the host does not block
                yield self._view(slot, nb)
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(self.device))
                slot["free"] = done
                slot["released"].set()
        finally:
            stop.set()
            for slot in self.slots:
                slot["released"].set()
            while th.is_alive():
                try:
                    filled.get(timeout=0.05)
                except queue.Empty:
                    pass
            th.join()


def u8_to_float(t: torch.Tensor, divisor: float = 255.0) -> torch.Tensor:
    """uint8 device tensor -> float32 / divisor through ``biu_u8_to_f32`` (targets of the fused losses): the correctly rounded quotient,
    the value ``TileStore.__getitem__`` and the augmentation kernels give for the same byte."""
    import ctypes as C
    from ._lib import check, lib
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    check(lib.biu_u8_to_f32(C.c_void_p(t.data_ptr()), float(divisor), C.c_void_p(out.data_ptr()), t.numel(),
                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "u8_to_f32")
    return out
