"""On-the-fly training augmentation on the device for uint8 tile batches (``biu_augment_u8``).

The reference augments offline: ``DataProcess.__augment`` runs an albumentations pipeline ``aug_factor`` times per tile and writes every
result to disk (``unet/data.py:217-245``, ``siam_unet/data.py:236-243``, ``unet3d/data.py:209-239``).  Here the same five transforms run
where the batch already is, fresh every epoch, in one kernel launch per field:

=========  ==============================================================================================================
recipe     stages (in the reference's order)
=========  ==============================================================================================================
"unet"     rot90 -> shift_scale_rotate -> brightness_contrast -> blur -> mult_noise
"siam"     rot90 -> shift_scale_rotate -> gauss_noise -> brightness_contrast
"unet3d"   as "siam"; the z-planes of a volume are channels, every plane gets the same in-plane transform
=========  ==============================================================================================================

The whole pipeline is applied with probability ``p``; ``shift_scale_rotate`` and ``brightness_contrast`` with 0.5, ``blur`` with 0.2, the
noise stage with 0.3.  Fields named ``mask`` are masks (nearest-neighbour gather, nothing else touches them), every other field is an image
(bilinear gather, then the intensity stages); ``kinds={"name": "mask" | "image"}`` overrides.  After every stage the value is clipped to
[0, 255] and rounded to nearest-even, as a uint8 pipeline does.

Geometry.  ``shift_scale_rotate`` maps a source pixel forward by ``x' = s (cos t (x - cx) + sin t (y - cy)) + cx + dx W``,
``y' = s (-sin t (x - cx) + cos t (y - cy)) + cy + dy H`` about ``(cx, cy) = ((W - 1) / 2, (H - 1) / 2)``; with this sign a rotation by
+90 degrees of a square tile equals ``np.rot90(x, 1)`` and -90 degrees ``np.rot90(x, 3)``.  ``rot90`` is a pixel permutation, so it is composed
with the inverse of that map into ONE 2x3 matrix per sample, computed on the host and handed to the kernel in float64 (the kernel does no
trigonometry; its coordinates and interpolation weights are float64 too, so the gather agrees with a float64 restatement): one resampling per field.

Randomness.  The per-sample record is a pure function of ``(seed, epoch, dataset index)`` (numpy's Philox generator with the key (seed, epoch) and the counter set to the index), so it does
not depend on batch composition, thread timing or call order; per-pixel noise is Philox4x32-10 in the kernel, keyed by the seed with the
counter (element group, dataset index, epoch, field-and-stage id).  Same seed -> same epoch, bit for bit.

This is distribution-level equivalence to the reference pipeline, not bit parity ("On-device augmentation").

The 2-D multi-output family's float fields have a pipeline of their own, ``AugmenterF32`` / ``biu_augment_f32`` in the second half of this file;
the 3-D multi-output family's volumes a third, ``AugmenterVol`` / ``biu_augment_vol_f32`` at the end.  The three classes share the record
stream and the launch loop (``_AugmenterCore``) and keep their own limits and kernels (the two float classes share the record).
``AugmenterF32`` also draws crops out of WHOLE items (``draw_crops`` / ``crop_matrix`` / ``biu_augment_f32_crop``, for ``feed.ImageStore``):
the same record and stream, the map going from a tile pixel into the item, NaN targets replaced by ``nan_to_val`` on the way.
``AugmenterVol`` does the same for WHOLE volumes (``draw_crops`` / ``vol_crop_matrix`` / ``biu_augment_vol_f32_crop``, for ``feed.VolumeStore``).
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import threading
import zlib
from typing import Dict, Optional, Sequence

import numpy as np
import torch

GATE, SSR, BC, BLUR, MULT, GAUSS = 1, 2, 4, 8, 16, 32          # include/biu.h: BIU_AUG_*
ORDER_UNET, ORDER_SIAM = 0, 1
MAX_BLUR = 15

# include/biu.h: biu_aug_params, 96 bytes
PARAMS_DTYPE = np.dtype([("flags", "<u4"), ("rot_k", "<u4"), ("blur_k", "<u4"), ("index", "<u4"), ("m", "<f8", (6,)),
                         ("alpha", "<f4"), ("beta", "<f4"), ("noise_a", "<f4"), ("noise_b", "<f4"),
                         ("angle", "<f4"), ("scale", "<f4"), ("dx", "<f4"), ("dy", "<f4")])
assert PARAMS_DTYPE.itemsize == 96

RECIPES = {"unet": ORDER_UNET, "siam": ORDER_SIAM, "unet3d": ORDER_SIAM}
STAGE_P = {"shift_scale_rotate": 0.5, "brightness_contrast": 0.5, "blur": 0.2, "noise": 0.3}


def field_id(name: str) -> int:
    """28-bit id of a field name in the noise counter: the same whatever other fields a batch holds."""
    return zlib.crc32(name.encode()) >> 4


def _matrix(k: int, angle: float, scale: float, dx: float, dy: float, h: int, w: int):
    """``inverse_matrix`` in plain Python floats (the feeder thread draws records while the training thread enqueues: every microsecond
    here is taken from the interpreter lock both share)."""
    if k % 2 and h != w:
        raise ValueError("rot90 by an odd number of quarter turns needs a square tile")
    if angle != 0:
        t = math.radians(angle)
        c, s = math.cos(t) / scale, math.sin(t) / scale
    else:
        c, s = 1.0 / scale, 0.0
    # inverse of the forward matrix scale [[cos, sin], [-sin, cos]]: a = [[c, -s], [s, c]]; offset b = centre - a (centre + shift)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    ux, uy = cx + dx * w, cy + dy * h
    bx, by = cx - (c * ux - s * uy), cy - (s * ux + c * uy)
    # np.rot90(src, k)[y, x] = src[sy, sx] with (sx, sy) = P_k (x, y) + o_k; below: P_k a and P_k b + o_k
    if k == 0:
        return c, -s, bx, s, c, by
    if k == 1:
        return -s, -c, w - 1 - by, c, -s, bx
    if k == 2:
        return -c, s, w - 1 - bx, -s, -c, h - 1 - by
    return s, c, by, -c, s, h - 1 - bx


def inverse_matrix(rot_k: int, angle: float, scale: float, dx: float, dy: float, h: int, w: int) -> np.ndarray:
    """float64 ``[m0 .. m5]``: output pixel (x, y) samples the source at ``(m0 x + m1 y + m2, m3 x + m4 y + m5)`` for
    ``shift_scale_rotate(np.rot90(src, rot_k))``.  Whole-pixel cases come out as exact integers."""
    return np.array(_matrix(int(rot_k) % 4, float(angle), float(scale), float(dx), float(dy), int(h), int(w))) + 0.0     # no negative zeros


_F4 = struct.Struct("<4f")
_REC = struct.Struct("<4I6d8f")
assert _REC.size == PARAMS_DTYPE.itemsize


def _pack(buf, offset, index, h, w, gate, rot_k, ssr, bc, blur_k, noise_flag, noise_a, noise_b):
    """Write one record at ``buf[offset:]``; stages behind a closed gate, and stages not given, leave the identity.  The matrix is computed
    from the fp32 values the record keeps, so the record alone says what the kernel was asked to do."""
    if not gate:
        rot_k, ssr, bc, blur_k, noise_flag = 0, None, None, 0, 0
    flags = (GATE if gate else 0) | (SSR if ssr is not None else 0) | (BC if bc is not None else 0) | (BLUR if blur_k else 0) | noise_flag
    angle, scale, dx, dy = _F4.unpack(_F4.pack(*ssr)) if ssr is not None else (0.0, 1.0, 0.0, 0.0)
    alpha, beta = (bc[0], 255.0 * bc[1]) if bc is not None else (1.0, 0.0)
    if not noise_flag:
        noise_a = noise_b = 0.0
    _REC.pack_into(buf, offset, flags, rot_k, blur_k, index, *_matrix(rot_k % 4, angle, scale, dx, dy, h, w), alpha, beta, noise_a, noise_b,
                   angle, scale, dx, dy)


def record(index: int, h: int, w: int, *, gate: bool = True, rot_k: int = 0, ssr=None, bc=None, blur_k: int = 0, mult=None,
           gauss_sigma: Optional[float] = None) -> np.ndarray:
    """One parameter record from its logical description: ``ssr = (angle in degrees, scale, dx, dy)``, ``bc = (alpha, beta)`` with beta as a
    fraction of 255, ``mult = (lo, hi)``.  With ``gate=False`` the sample passes unchanged.  ``Augmenter.draw`` builds its records the same way."""
    if blur_k and (blur_k % 2 == 0 or not 1 <= blur_k <= MAX_BLUR):
        raise ValueError(f"blur kernel {blur_k}: odd and at most {MAX_BLUR}")
    if mult is not None and gauss_sigma is not None:
        raise ValueError("a record carries one noise stage")
    noise = (MULT, mult[0], mult[1] - mult[0]) if mult is not None else (GAUSS, gauss_sigma, 0.0) if gauss_sigma is not None else (0, 0.0, 0.0)
    buf = bytearray(_REC.size)
    _pack(buf, 0, int(index), int(h), int(w), bool(gate), int(rot_k), ssr, bc, int(blur_k), *noise)
    return np.frombuffer(buf, dtype=PARAMS_DTYPE)[0]


class _AugmenterCore:
    """What ``Augmenter``, ``AugmenterF32`` and ``AugmenterVol`` share: the per-sample Philox stream and the record buffer on the host, the
    checks and the per-field loop around the launch on the device.  A subclass names its record (``params_dtype``, ``_rec``, ``n_uniform``,
    ``blur_flag``), its kinds, the store attributes its constructor takes, its tensor dtypes and layouts (``field_dims``, ``field_layout``), and
    provides ``_packer`` and ``_launch``."""
    field_dims, field_layout = (3, 4), "[B, H, W] or [B, C, H, W]"      # a field without / with the channel axis

    def _init_core(self, seed, kinds, shape):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.kinds = dict(kinds or {})
        for v in self.kinds.values():
            if v not in self.allowed_kinds:
                raise ValueError(f'kind "{v}": one of {sorted(self.allowed_kinds)}')
        self.shape = tuple(shape) if shape is not None else None
        self._bitgen = np.random.Philox(key=[0, 0])              # draw() sets key and counter per sample
        self._gen, self._state, self._lock = np.random.Generator(self._bitgen), self._bitgen.state, threading.Lock()

    @classmethod
    def _store_kw(cls, store, overrides):
        """Constructor keywords from the attributes a ``TileStore`` records (those of the ``DataProcess`` it was converted from)."""
        attrs = getattr(store, "attrs", {})
        kw = {a: attrs[a] for a in cls.store_attrs if attrs.get(a) is not None}
        kw["shape"] = tuple(store.fields["image"] if "image" in store.fields else next(iter(store.fields.values())))
        kw.update(overrides)
        return kw

    # ---- host: the per-sample records -------------------------------------------------------------------------------------------
    def draw(self, epoch: int, indices, shape: Optional[Sequence[int]] = None) -> np.ndarray:
        """Record array for the samples ``indices`` of epoch ``epoch``; ``shape``: the tile shape (its last two axes count)."""
        shape = tuple(shape) if shape is not None else self.shape
        if shape is None or len(shape) < 2:
            raise ValueError(f"{type(self).__name__}.draw needs the tile shape (constructor's or this call's `shape`)")
        pack = self._packer(int(shape[-2]), int(shape[-1]))
        return self._records(epoch, indices, lambda i: pack)

    def _records(self, epoch: int, indices, pack_of, n_uniform: Optional[int] = None) -> np.ndarray:
        """The record stream under ``draw``: sample ``i`` is packed by ``pack_of(i)`` from its own uniforms (``n_uniform`` of them, default the
        class's; the generator hands out doubles one after the other, so a longer draw begins with the shorter one's numbers)."""
        idx = np.atleast_1d(np.asarray(indices, dtype=np.int64)).tolist()
        size, n = self._rec.size, self.n_uniform if n_uniform is None else int(n_uniform)
        buf = bytearray(len(idx) * size)
        key = (self.seed, int(epoch) & 0xFFFFFFFFFFFFFFFF)
        with self._lock:
            for j, i in enumerate(idx):
                # the generator's stream is a function of its key (seed, epoch) and counter (0, dataset index, 0, 0) alone; a fixed number of
                # uniforms in a fixed order whatever the gates say: nothing shifts the stream
                st = self._state
                st["state"]["key"][:] = key
                st["state"]["counter"][:] = (0, i & 0xFFFFFFFFFFFFFFFF, 0, 0)
                st["buffer_pos"], st["has_uint32"] = 4, 0
                self._bitgen.state = st
                pack_of(i)(buf, j * size, i & 0xFFFFFFFF, self._gen.random(n).tolist())
        return np.frombuffer(buf, dtype=self.params_dtype)

    # ---- device ------------------------------------------------------------------------------------------------------------------
    def __call__(self, batch: Dict[str, torch.Tensor], params: np.ndarray, epoch: int, out: Optional[Dict[str, torch.Tensor]] = None,
                 params_dev: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Augment ``{field: device tensor [B, H, W] | [B, C or D, H, W]}`` (``AugmenterVol``: ``[B, D, H, W] | [B, C, D, H, W]``) with the records ``params`` (``draw``'s result, one per sample) on the
        current stream; ``out``: tensors to write into (never the inputs: a gather cannot run in place); ``params_dev``: the same records
        already on the device as bytes (the feeder uploads them with the batch).  ``Augmenter`` takes and writes uint8; ``AugmenterF32``
        takes float32 or uint8 and always writes float32."""
        from ._lib import check, lib
        params = np.ascontiguousarray(params, dtype=self.params_dtype)
        first = next(iter(batch.values()))
        if len(params) != first.shape[0]:
            raise ValueError(f"{len(params)} parameter records for a batch of {first.shape[0]}")
        blurs = params["blur_k"][(params["flags"] & self.blur_flag) != 0]
        max_blur = int(blurs.max()) if len(blurs) else 0
        if params_dev is None:
            params_dev = torch.from_numpy(params.view(np.uint8).copy()).to(first.device)
        stream = C.c_void_p(torch.cuda.current_stream(first.device).cuda_stream)
        src, dst_dtype = self.src_dtypes, self.dst_dtype
        res = {}
        for name, t in batch.items():
            if t.dtype not in src or not t.is_cuda or t.dim() not in self.field_dims or not t.is_contiguous():
                raise ValueError(f'field "{name}": a contiguous {_names(src)} device tensor {self.field_layout} is expected')
            dst = out[name] if out is not None else torch.empty(t.shape, dtype=dst_dtype, device=t.device)
            if dst.shape != t.shape or dst.dtype != dst_dtype or dst.device != t.device or not dst.is_contiguous() or dst.data_ptr() == t.data_ptr():
                raise ValueError(f'field "{name}": the output must be a second contiguous {_names((dst_dtype,))} tensor of the same shape and device')
            check(self._launch(lib, name, t, dst, t.shape[1] if t.dim() == self.field_dims[1] else 1, params_dev, max_blur, int(epoch) & 0xFFFFFFFF, stream),
                  self.launch_name)
            res[name] = dst
        return res


def _names(dtypes) -> str:
    return " or ".join(str(d).split(".")[-1] for d in dtypes)


class Augmenter(_AugmenterCore):
    """Draws per-sample parameter records on the host and runs ``biu_augment_u8`` on device batches; see the module docstring."""

    params_dtype, _rec, n_uniform, blur_flag = PARAMS_DTYPE, _REC, 13, BLUR        # DeviceFeeder sizes its record buffers by params_dtype
    allowed_kinds = ("mask", "image")
    store_attrs = ("shiftscalerotate", "brightness_contrast", "noise_lims", "noise_amp", "blur_limit")
    src_dtypes, dst_dtype, launch_name = (torch.uint8,), torch.uint8, "augment_u8"

    def __init__(self, recipe: str, *, shiftscalerotate=(0, 0, 0), brightness_contrast=(0.25, 0.25), noise_lims=(0.5, 1.2), noise_amp=10,
                 blur_limit=(3, 7), p: float = 0.8, seed: int = 0, kinds: Optional[Dict[str, str]] = None, shape: Optional[Sequence[int]] = None):
        if recipe not in RECIPES:
            raise ValueError(f'recipe "{recipe}" not defined (one of {sorted(RECIPES)})')
        self.recipe, self.order = recipe, RECIPES[recipe]
        self.shiftscalerotate = tuple(float(v) for v in shiftscalerotate)
        self.brightness_contrast = tuple(float(v) for v in brightness_contrast)
        self.noise_lims = tuple(float(v) for v in noise_lims)
        self.noise_amp = float(noise_amp)
        self.blur_limit = (int(blur_limit), int(blur_limit)) if np.isscalar(blur_limit) else tuple(int(v) for v in blur_limit)
        if len(self.shiftscalerotate) != 3 or len(self.brightness_contrast) != 2 or len(self.noise_lims) != 2 or len(self.blur_limit) != 2:
            raise ValueError("shiftscalerotate takes 3 limits, brightness_contrast, noise_lims and blur_limit 2")
        if self.blur_limit[1] > MAX_BLUR:
            raise ValueError(f"blur_limit {self.blur_limit}: box kernels above {MAX_BLUR} are not supported")
        self.blur_sizes = [k for k in range(max(1, self.blur_limit[0]), self.blur_limit[1] + 1) if k % 2]
        if not self.blur_sizes:
            raise ValueError(f"blur_limit {self.blur_limit} holds no odd kernel size")
        if self.noise_amp < 0 or not 0.0 <= p <= 1.0:
            raise ValueError("noise_amp is a variance and p a probability")
        self.p = float(p)
        self._init_core(seed, kinds, shape)

    @classmethod
    def from_store(cls, store, recipe: str, **overrides) -> "Augmenter":
        """Limits from the attributes a ``TileStore`` records, else the defaults."""
        return cls(recipe, **cls._store_kw(store, overrides))

    def describe(self) -> dict:
        return {"recipe": self.recipe, "p": self.p, "seed": self.seed, "shiftscalerotate": self.shiftscalerotate,
                "brightness_contrast": self.brightness_contrast, "noise_lims": self.noise_lims, "noise_amp": self.noise_amp,
                "blur_limit": self.blur_limit, "stage_p": dict(STAGE_P), "kinds": dict(self.kinds)}

    def kind(self, name: str) -> str:
        return self.kinds.get(name, "mask" if name == "mask" else "image")

    def _packer(self, h, w):
        """``draw``'s record from thirteen uniforms."""
        sym = lambda v, a: (2.0 * v - 1.0) * a
        p, lim, bcl, sizes, unet = self.p, self.shiftscalerotate, self.brightness_contrast, self.blur_sizes, self.order == ORDER_UNET
        noise = (MULT, self.noise_lims[0], self.noise_lims[1] - self.noise_lims[0]) if unet else (GAUSS, math.sqrt(self.noise_amp), 0.0)

        def pack(buf, offset, index, u):
            _pack(buf, offset, index, h, w, u[0] < p, int(u[1] * 4) if h == w else 2 * int(u[1] * 2),
                  (sym(u[3], lim[2]), 1.0 + sym(u[4], lim[1]), sym(u[5], lim[0]), sym(u[6], lim[0])) if u[2] < STAGE_P["shift_scale_rotate"] else None,
                  (1.0 + sym(u[8], bcl[1]), sym(u[9], bcl[0])) if u[7] < STAGE_P["brightness_contrast"] else None,
                  sizes[min(int(u[11] * len(sizes)), len(sizes) - 1)] if unet and u[10] < STAGE_P["blur"] else 0,
                  *(noise if u[12] < STAGE_P["noise"] else (0, 0.0, 0.0)))
        return pack

    def _launch(self, lib, name, t, dst, planes, params_dev, max_blur, epoch, stream):
        mask = self.kind(name) == "mask"
        return lib.biu_augment_u8(C.c_void_p(t.data_ptr()), C.c_void_p(dst.data_ptr()), t.shape[0], planes, t.shape[-2], t.shape[-1], int(mask),
                                  C.c_void_p(params_dev.data_ptr()), self.order, 0 if mask else max_blur, self.seed, epoch, field_id(name), stream)


# =====================================================================================================================================
# float fields: the 2-D multi-output family (``biu_augment_f32``)
# =====================================================================================================================================
# The reference's pipeline for this family (``multi_output_unet/data.py:187-311``) is none of the three recipes above: either an arbitrary
# angle (``scipy.ndimage.rotate(mode='grid-wrap')``, image ``order=0``) or a quarter turn, then ``RandomScale`` (nearest) -> ``Blur`` ->
# ``PadIfNeeded(BORDER_WRAP)`` -> ``RandomCrop`` -> ``ShotNoise`` -> ``GaussNoise`` -> ``RandomBrightnessContrast``, on float32 data, with an
# ``orientation`` target whose VALUES change under rotation.  Here rotation, scale and crop offset are one 2x3 map with wrap-around indices:
#
# =========  ================================================================================================================
# kind       what the kernel does
# =========  ================================================================================================================
# "image"    nearest gather, then blur -> shot noise -> Gauss noise -> brightness/contrast (fp32, clipped to [0, 1])
# "mask"     any scalar target (mask, probability, distance map): bilinear under an arbitrary angle, nearest otherwise;
#            ``target_interp="cubic"``: the reference's periodic cubic B-spline and its clip instead of the bilinear gather
# "vector"   plane pairs ``(cos phi, sin phi)``: nearest gather, the pair is rotated by the record's rotation (phi - t)
# =========  ================================================================================================================
#
# The field ``image`` is an image, a field named ``orientation`` a vector, every other field a mask; ``kinds={...}`` overrides.
ROT_F, SCALE_F, BLUR_F, SHOT_F, GAUSS_F, BC_F = 1, 2, 4, 8, 16, 32          # include/biu.h: BIU_AUGF_*
KIND_IMAGE, KIND_MASK, KIND_VECTOR = 0, 1, 2
KINDS_F32 = {"image": KIND_IMAGE, "mask": KIND_MASK, "vector": KIND_VECTOR}
STAGE_P_MO2D = {"arbitrary_angle": 0.5, "scale": 0.75, "blur": 0.25, "shot_noise": 0.25, "gauss_noise": 0.25, "brightness_contrast": 0.5}

# include/biu.h: biu_augf_params, 104 bytes; dx, dy in pixels
PARAMS_F32_DTYPE = np.dtype([("flags", "<u4"), ("rot_k", "<u4"), ("blur_k", "<u4"), ("index", "<u4"), ("m", "<f8", (6,)),
                             ("cos_t", "<f4"), ("sin_t", "<f4"), ("alpha", "<f4"), ("beta", "<f4"), ("shot_s", "<f4"), ("gauss_sigma", "<f4"),
                             ("angle", "<f4"), ("scale", "<f4"), ("dx", "<f4"), ("dy", "<f4")])
assert PARAMS_F32_DTYPE.itemsize == 104
_F1 = struct.Struct("<f")
_REC_F32 = struct.Struct("<4I6d10f")
assert _REC_F32.size == PARAMS_F32_DTYPE.itemsize
_QUARTER = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))                # (cos, sin) of k quarter turns, exact
TARGET_INTERP = ("linear", "cubic")                                          # AugmenterF32(target_interp=...)


def _f32(v: float) -> float:
    return _F1.unpack(_F1.pack(v))[0]


def _pack_f32(buf, offset, index, h, w, rot_k, angle, scale, shift, blur_k, shot_s, gauss_sigma, bc):
    """Write one float-path record at ``buf[offset:]``; stages not given leave the identity.  Matrix and ``(cos_t, sin_t)`` are computed from
    the fp32 values the record keeps.  The rotation the orientation pair sees is ``rot_k`` quarter turns plus ``angle``."""
    flags = ((ROT_F if angle is not None else 0) | (SCALE_F if scale is not None or shift != (0, 0) else 0) | (BLUR_F if blur_k else 0)
             | (SHOT_F if shot_s is not None else 0) | (GAUSS_F if gauss_sigma is not None else 0) | (BC_F if bc is not None else 0))
    a = _f32(angle) if angle is not None else 0.0
    s = _f32(scale) if scale is not None else 1.0
    dx, dy = float(int(shift[0])), float(int(shift[1]))
    qc, qs = _QUARTER[rot_k % 4]
    if a != 0:
        t = math.radians(a)
        ca, sa = math.cos(t), math.sin(t)
        ct, st = qc * ca - qs * sa, qs * ca + qc * sa               # quarter turns only swap and negate
    else:
        ct, st = qc, qs
    alpha, beta = bc if bc is not None else (1.0, 0.0)
    _REC_F32.pack_into(buf, offset, flags, rot_k, blur_k, index, *_matrix(rot_k % 4, a, s, dx / w, dy / h, h, w), ct + 0.0, st + 0.0, alpha, beta,
                       shot_s if shot_s is not None else 0.0, gauss_sigma if gauss_sigma is not None else 0.0, a, s, dx, dy)


def record_f32(index: int, h: int, w: int, *, rot_k: int = 0, angle: Optional[float] = None, scale: Optional[float] = None, shift=(0, 0),
               blur_k: int = 0, shot_s: Optional[float] = None, gauss_sigma: Optional[float] = None, bc=None) -> np.ndarray:
    """One ``biu_augf_params`` record from its logical description: ``rot_k`` quarter turns, ``angle`` in degrees (given at all, mask fields
    are gathered bilinearly), ``scale`` about the tile centre, ``shift = (dx, dy)`` in whole pixels, ``bc = (alpha, beta)`` with
    ``v * alpha + beta`` on the [0, 1] scale.  ``AugmenterF32.draw`` builds its records the same way."""
    if blur_k and (blur_k % 2 == 0 or not 1 <= blur_k <= MAX_BLUR):
        raise ValueError(f"blur kernel {blur_k}: odd and at most {MAX_BLUR}")
    if shot_s is not None and not shot_s > 0:
        raise ValueError("shot noise needs a positive scale")
    if scale is not None and not scale > 0:
        raise ValueError("scale must be positive")
    buf = bytearray(_REC_F32.size)
    _pack_f32(buf, 0, int(index), int(h), int(w), int(rot_k), angle, scale, (int(shift[0]), int(shift[1])), int(blur_k), shot_s, gauss_sigma, bc)
    return np.frombuffer(buf, dtype=PARAMS_F32_DTYPE)[0]


# ---- whole items (``feed.ImageStore``, ``biu_augment_f32_crop``): the map goes from an output TILE pixel to a coordinate in the ITEM --------------
SOURCE_DTYPE = np.dtype([("offset", "<u8"), ("h", "<i4"), ("w", "<i4")])     # include/biu.h: biu_augf_source, 16 bytes
assert SOURCE_DTYPE.itemsize == 16
VALIDATION_EPOCH = 0xFFFFFFFF                                                # the fixed epoch key of validation patches


def _after(a, b):
    """The 2x3 map ``a`` applied to the result of the 2x3 map ``b``, in plain Python floats."""
    return (a[0] * b[0] + a[1] * b[3], a[0] * b[1] + a[1] * b[4], a[0] * b[2] + a[1] * b[5] + a[2],
            a[3] * b[0] + a[4] * b[3], a[3] * b[1] + a[4] * b[4], a[3] * b[2] + a[4] * b[5] + a[5])


def _crop_matrix(k, angle, scale, ox, oy, h, w):
    k %= 4
    ht, wt = (w, h) if k % 2 else (h, w)                     # the turned item
    # 1. crop origin, 2. scale about pixel centres: tile pixel -> pixel of the scaled image -> coordinate in the turned, rotated item
    inv = 1.0 / scale
    shift = 0.5 * inv - 0.5
    m = (inv, 0.0, ox * inv + shift, 0.0, inv, oy * inv + shift)
    # 3. rotation about the item centre (``_matrix``'s sign: +90 degrees equals np.rot90(x, 1))
    if angle != 0:
        t = math.radians(angle)
        c, s = math.cos(t), math.sin(t)
        cx, cy = (wt - 1) / 2.0, (ht - 1) / 2.0
        m = _after((c, -s, cx - (c * cx - s * cy), s, c, cy - (s * cx + c * cy)), m)
    # 4. quarter turn: np.rot90(src, k)[y, x] = src[sy, sx], an index permutation
    if k == 1:
        m = _after((0.0, -1.0, w - 1.0, 1.0, 0.0, 0.0), m)
    elif k == 2:
        m = _after((-1.0, 0.0, w - 1.0, 0.0, -1.0, h - 1.0), m)
    elif k == 3:
        m = _after((0.0, 1.0, 0.0, -1.0, 0.0, h - 1.0), m)
    return tuple(v + 0.0 for v in m)                         # no negative zeros


def crop_matrix(rot_k: int, angle: float, scale: float, origin, item_hw, tile_hw=None) -> np.ndarray:
    """float64 ``[m0 .. m5]``: pixel (x, y) of an output tile samples the ITEM ``[h, w]`` at ``(m0 x + m1 y + m2, m3 x + m4 y + m5)``.  Four
    steps in one map: the crop ``origin = (ox, oy)`` in the scaled image; ``scale`` about pixel centres (pixel X of the scaled image is
    ``(X + 0.5) / scale - 0.5``); rotation by ``angle`` degrees about the centre of the turned item; ``rot_k`` quarter turns
    (``np.rot90(item, rot_k)``, which is ``w x h`` for odd ``rot_k``).  The tile extent does not enter the map (a tile larger than the scaled
    item simply wraps); ``tile_hw`` is accepted so that a call names everything a crop consists of.  Whole-pixel cases are exact integers."""
    if not scale > 0:
        raise ValueError("scale must be positive")
    return np.array(_crop_matrix(int(rot_k), float(angle), float(scale), float(origin[0]), float(origin[1]), int(item_hw[0]), int(item_hw[1])))


def _pack_crop(buf, offset, index, h, w, rot_k, angle, scale, origin, blur_k, shot_s, gauss_sigma, bc):
    """``_pack_f32`` for a crop out of a whole item ``[h, w]``: the same record, ``m`` from ``_crop_matrix``, ``dx, dy`` the crop origin."""
    flags = ((ROT_F if angle is not None else 0) | (SCALE_F if scale is not None else 0) | (BLUR_F if blur_k else 0)
             | (SHOT_F if shot_s is not None else 0) | (GAUSS_F if gauss_sigma is not None else 0) | (BC_F if bc is not None else 0))
    a = _f32(angle) if angle is not None else 0.0
    s = _f32(scale) if scale is not None else 1.0
    ox, oy = float(int(origin[0])), float(int(origin[1]))
    qc, qs = _QUARTER[rot_k % 4]
    if a != 0:
        t = math.radians(a)
        ca, sa = math.cos(t), math.sin(t)
        ct, st = qc * ca - qs * sa, qs * ca + qc * sa
    else:
        ct, st = qc, qs
    alpha, beta = bc if bc is not None else (1.0, 0.0)
    _REC_F32.pack_into(buf, offset, flags, rot_k, blur_k, index, *_crop_matrix(rot_k, a, s, ox, oy, h, w), ct + 0.0, st + 0.0, alpha, beta,
                       shot_s if shot_s is not None else 0.0, gauss_sigma if gauss_sigma is not None else 0.0, a, s, ox, oy)


def record_crop(index: int, item_hw, *, rot_k: int = 0, angle: Optional[float] = None, scale: Optional[float] = None, origin=(0, 0),
                blur_k: int = 0, shot_s: Optional[float] = None, gauss_sigma: Optional[float] = None, bc=None) -> np.ndarray:
    """One ``biu_augf_params`` record for ``biu_augment_f32_crop`` from its logical description (``record_f32``'s, with ``origin = (ox, oy)`` the
    crop's first pixel in the turned, rotated and scaled item).  ``AugmenterF32.draw_crops`` builds its records the same way."""
    if blur_k and (blur_k % 2 == 0 or not 1 <= blur_k <= MAX_BLUR):
        raise ValueError(f"blur kernel {blur_k}: odd and at most {MAX_BLUR}")
    if shot_s is not None and not shot_s > 0:
        raise ValueError("shot noise needs a positive scale")
    if scale is not None and not scale > 0:
        raise ValueError("scale must be positive")
    buf = bytearray(_REC_F32.size)
    _pack_crop(buf, 0, int(index), int(item_hw[0]), int(item_hw[1]), int(rot_k), angle, scale, origin, int(blur_k), shot_s, gauss_sigma, bc)
    return np.frombuffer(buf, dtype=PARAMS_F32_DTYPE)[0]


def _pair(v, what):
    v = (v, v) if np.isscalar(v) else tuple(v)
    if len(v) != 2:
        raise ValueError(f"{what} takes two limits")
    return v


class AugmenterF32(_AugmenterCore):
    """Draws ``biu_augf_params`` records on the host and runs ``biu_augment_f32`` on device batches of float32 or uint8 fields (the output is
    always float32, so ``DeviceFeeder``'s augmented buffers are float32 whatever the store holds): the 2-D multi-output family's recipe ``"mo2d"``.

    ``target_interp``: how "mask" fields are resampled under an arbitrary-angle rotation.  ``"linear"`` (the default) gathers bilinearly;
    ``"cubic"`` is the reference's ``scipy.ndimage.rotate(order=3, mode='grid-wrap')`` with its clip into the target's own range
    (``biu_spline_prefilter_f32`` + ``biu_augment_f32_cubic``, three launches for such a field instead of one).  The mode draws no uniform:
    the records of both are the same, and batches without an arbitrary-angle sample take the one ``biu_augment_f32`` launch either way.
    On a ``feed.ImageStore`` the coefficients, the clip range and the NaN indicator are those of the whole item, computed once per store
    (``ImageStore.spline_tables``, handed to ``feed.CropFeeder(..., spline=)``) and read by one ``biu_augment_f32_crop_cubic`` launch per
    such field and batch; NaN is carried as the reference's ``rotate_array`` carries it at ``order=3``."""

    recipe = "mo2d"
    params_dtype, _rec, n_uniform, blur_flag = PARAMS_F32_DTYPE, _REC_F32, 16, BLUR_F
    allowed_kinds = tuple(KINDS_F32)
    store_attrs = ("gauss_noise_lims", "shot_noise_lims", "brightness_contrast", "blur_limit", "random_rotate", "scale_limit")
    src_dtypes, dst_dtype, launch_name = (torch.float32, torch.uint8), torch.float32, "augment_f32"
    source_dtype = SOURCE_DTYPE                  # feed.CropFeeder sizes its source buffers by it
    rot_flag = ROT_F                             # ... and reads from the records whether a batch needs the cubic launch

    def __init__(self, *, gauss_noise_lims=(0.01, 0.1), shot_noise_lims=(0.001, 0.01), brightness_contrast=(0.1, 0.1), blur_limit=(3, 5),
                 random_rotate: bool = True, scale_limit=(0, 0), seed: int = 0, kinds: Optional[Dict[str, str]] = None,
                 shape: Optional[Sequence[int]] = None, target_interp: str = "linear"):
        self.gauss_noise_lims = tuple(float(v) for v in _pair(gauss_noise_lims, "gauss_noise_lims"))
        self.shot_noise_lims = tuple(float(v) for v in _pair(shot_noise_lims, "shot_noise_lims"))
        self.brightness_contrast = tuple(float(v) for v in _pair(brightness_contrast, "brightness_contrast"))
        self.blur_limit = tuple(int(v) for v in _pair(blur_limit, "blur_limit"))
        sl = _pair(scale_limit, "scale_limit")
        self.scale_limit = tuple(float(v) for v in ((-sl[0], sl[0]) if np.isscalar(scale_limit) else sl))
        self.random_rotate = bool(random_rotate)
        if target_interp not in TARGET_INTERP:
            raise ValueError(f'target_interp "{target_interp}": one of {list(TARGET_INTERP)}')
        self.target_interp = target_interp
        self._spline_scratch = {}                # (field name, shape, device) -> (coef, range), see _launch
        if self.blur_limit[1] > MAX_BLUR:
            raise ValueError(f"blur_limit {self.blur_limit}: box kernels above {MAX_BLUR} are not supported")
        self.blur_sizes = [k for k in range(max(3, self.blur_limit[0]), self.blur_limit[1] + 1) if k % 2]
        if not self.blur_sizes:
            raise ValueError(f"blur_limit {self.blur_limit} holds no odd kernel size of 3 or more")
        if not 0 < self.shot_noise_lims[0] <= self.shot_noise_lims[1]:
            raise ValueError("shot_noise_lims: positive scales, lower first")
        if not 0 <= self.gauss_noise_lims[0] <= self.gauss_noise_lims[1]:
            raise ValueError("gauss_noise_lims: standard deviations, lower first")
        if not -1 < self.scale_limit[0] <= self.scale_limit[1]:
            raise ValueError("scale_limit: 1 + limit must stay positive, lower first")
        self._init_core(seed, kinds, shape)

    @classmethod
    def from_store(cls, store, recipe: str = "mo2d", **overrides) -> "AugmenterF32":
        """Limits from the attributes a ``TileStore`` records, else the reference's defaults."""
        if recipe != "mo2d":
            raise ValueError(f'recipe "{recipe}" not defined for float fields (only "mo2d")')
        return cls(**cls._store_kw(store, overrides))

    def describe(self) -> dict:
        return {"recipe": self.recipe, "seed": self.seed, "gauss_noise_lims": self.gauss_noise_lims, "shot_noise_lims": self.shot_noise_lims,
                "brightness_contrast": self.brightness_contrast, "blur_limit": self.blur_limit, "random_rotate": self.random_rotate,
                "scale_limit": self.scale_limit, "stage_p": dict(STAGE_P_MO2D), "kinds": dict(self.kinds), "target_interp": self.target_interp}

    def kind(self, name: str) -> str:
        return self.kinds.get(name, "image" if name == "image" else "vector" if name == "orientation" else "mask")

    def __call__(self, batch, params, epoch, out=None, params_dev=None):
        # the host knows from the records, as it knows max_blur, whether any sample of the batch takes the cubic path
        self._any_rot = self.target_interp == "cubic" and bool((np.asarray(params["flags"]) & ROT_F).any())
        return super().__call__(batch, params, epoch, out, params_dev)

    def _packer(self, h, w):
        """``draw``'s record from sixteen uniforms."""
        lerp = lambda u, lim: lim[0] + u * (lim[1] - lim[0])
        P, sizes, bcl, rotate = STAGE_P_MO2D, self.blur_sizes, self.brightness_contrast, self.random_rotate
        scale_limit, shot_lims, gauss_lims = self.scale_limit, self.shot_noise_lims, self.gauss_noise_lims

        def pack(buf, offset, index, u):
            rot_k, angle, scale, shift = 0, None, None, (0, 0)
            if rotate:
                if u[0] < P["arbitrary_angle"]:
                    angle = 360.0 * u[1]
                else:                                        # {0, 1, 2, 3} on square tiles; upstream's randint(0, 3) never draws 3
                    rot_k = int(u[2] * 4) if h == w else 2 * int(u[2] * 2)
            if u[3] < P["scale"]:
                scale = _f32(1.0 + lerp(u[4], scale_limit))
                # RandomCrop out of the up-scaled tile: a whole-pixel offset around the centred crop; a down-scaled tile is wrap-padded
                fw, fh = max(int(round(w * scale)) - w, 0), max(int(round(h * scale)) - h, 0)
                shift = (fw // 2 - min(int(u[5] * (fw + 1)), fw), fh // 2 - min(int(u[6] * (fh + 1)), fh))
            _pack_f32(buf, offset, index, h, w, rot_k, angle, scale, shift,
                      sizes[min(int(u[8] * len(sizes)), len(sizes) - 1)] if u[7] < P["blur"] else 0,
                      lerp(u[10], shot_lims) if u[9] < P["shot_noise"] else None,
                      lerp(u[12], gauss_lims) if u[11] < P["gauss_noise"] else None,
                      (1.0 + (2.0 * u[14] - 1.0) * bcl[1], (2.0 * u[15] - 1.0) * bcl[0]) if u[13] < P["brightness_contrast"] else None)
        return pack

    # ---- whole items: crops out of a ``feed.ImageStore`` ---------------------------------------------------------------------------------
    def _crop_packer(self, h, w, th, tw):
        """``draw_crops``' record from the same sixteen uniforms behind the same gates as ``_packer``.  What differs: the quarter turns are
        drawn from {0, 1, 2, 3} whatever the item's shape (the turned item is ``w x h`` and the crop comes out of it), and ``u[5]``, ``u[6]``
        ALWAYS place the crop -- ``RandomCrop`` has ``p = 1`` -- in the turned item's extent times the scale, rounded."""
        lerp = lambda u, lim: lim[0] + u * (lim[1] - lim[0])
        P, sizes, bcl, rotate = STAGE_P_MO2D, self.blur_sizes, self.brightness_contrast, self.random_rotate
        scale_limit, shot_lims, gauss_lims = self.scale_limit, self.shot_noise_lims, self.gauss_noise_lims

        def pack(buf, offset, index, u):
            rot_k, angle, scale = 0, None, None
            if rotate:
                if u[0] < P["arbitrary_angle"]:
                    angle = 360.0 * u[1]
                else:
                    rot_k = int(u[2] * 4)
            if u[3] < P["scale"]:
                scale = _f32(1.0 + lerp(u[4], scale_limit))
            s = scale if scale is not None else 1.0
            ht, wt = (w, h) if rot_k % 2 else (h, w)
            hs, ws = max(int(round(ht * s)), 1), max(int(round(wt * s)), 1)
            ox = min(int(u[5] * (ws - tw + 1)), ws - tw) if ws >= tw else 0          # a scaled item smaller than the tile: the wrap pads
            oy = min(int(u[6] * (hs - th + 1)), hs - th) if hs >= th else 0
            _pack_crop(buf, offset, index, h, w, rot_k, angle, scale, (ox, oy),
                       sizes[min(int(u[8] * len(sizes)), len(sizes) - 1)] if u[7] < P["blur"] else 0,
                       lerp(u[10], shot_lims) if u[9] < P["shot_noise"] else None,
                       lerp(u[12], gauss_lims) if u[11] < P["gauss_noise"] else None,
                       (1.0 + (2.0 * u[14] - 1.0) * bcl[1], (2.0 * u[15] - 1.0) * bcl[0]) if u[13] < P["brightness_contrast"] else None)
        return pack

    def draw_crops(self, epoch: int, patch_indices, store, offsets: Optional[Dict[str, np.ndarray]] = None):
        """Records and sources for the patches ``patch_indices`` of a ``feed.ImageStore`` in epoch ``epoch``: a pure function of
        ``(seed, epoch, patch index)`` -- Philox key ``(seed, epoch)``, counter = the patch index, ``draw``'s stream.  Returns
        ``(records [n], {field: sources [n]})``; a source is ``(element offset of the patch's item in the field's arena, h, w)``.
        ``offsets``: the per-item offsets ``store.to_device`` returned (default: the store's own, which are the same numbers)."""
        idx = np.atleast_1d(np.asarray(patch_indices, dtype=np.int64))
        items = store.locate(idx)
        th, tw = (int(d) for d in store.dim_out)
        sizes, packers, item_of = store.sizes, {}, dict(zip(idx.tolist(), items.tolist()))

        def pack_of(j):
            h, w = sizes[item_of[j]]
            if (h, w) not in packers:
                packers[(h, w)] = self._crop_packer(int(h), int(w), th, tw)
            return packers[(h, w)]

        records = self._records(epoch, idx, pack_of)
        offsets = offsets if offsets is not None else store.offsets
        sources = {}
        for name in store.fields:
            src = np.empty(len(idx), dtype=SOURCE_DTYPE)
            src["offset"], src["h"], src["w"] = np.asarray(offsets[name])[items], sizes[items, 0], sizes[items, 1]
            sources[name] = src
        return records, sources

    def spline_fields(self, store) -> list:
        """The fields of ``store`` that ``target_interp="cubic"`` resamples with the spline: those of kind "mask"."""
        return [k for k in store.fields if self.kind(k) == "mask"]

    def launch_crop(self, name, arena, dst, params_dev, sources_dev, nan_to_val, max_blur, epoch, spline=None, item_index_dev=None):
        """One ``biu_augment_f32_crop`` launch on the current stream: field ``name`` of ``dst.shape[0]`` patches ``dst [n, planes, th, tw]`` out
        of the 1-D device tensor ``arena``; ``params_dev`` / ``sources_dev``: the records and this field's sources on the device, as bytes.

        ``spline`` (the field's ``feed.SplineTables``) with ``item_index_dev`` (the item of every patch, int32 on the device, as bytes or
        numbers): the caller has read from the records that some patch of the batch has the ROT flag, as it reads ``max_blur``; a "mask" field
        of a cubic augmenter then takes the one ``biu_augment_f32_crop_cubic`` launch instead.  Every other field, batch and augmenter
        keeps the launch above."""
        from ._lib import check, lib
        kind = KINDS_F32[self.kind(name)]
        cubic = spline is not None and kind == KIND_MASK and self.target_interp == "cubic"
        if arena.dtype not in self.src_dtypes or not arena.is_cuda or arena.dim() != 1 or not arena.is_contiguous():
            raise ValueError(f'field "{name}": the arena is a contiguous 1-D {_names(self.src_dtypes)} device tensor')
        if dst.dtype != torch.float32 or dst.dim() != 4 or not dst.is_contiguous() or dst.device != arena.device:
            raise ValueError(f'field "{name}": the output is a contiguous float32 tensor [n, planes, th, tw] on the arena\'s device')
        n, planes, th, tw = dst.shape
        if kind == KIND_VECTOR and planes % 2:
            raise ValueError(f'field "{name}": a vector field holds (cos, sin) plane pairs, got {planes} plane(s)')
        if params_dev.numel() * params_dev.element_size() < n * PARAMS_F32_DTYPE.itemsize or \
                sources_dev.numel() * sources_dev.element_size() < n * SOURCE_DTYPE.itemsize:
            raise ValueError(f"{n} patches need {n} parameter records and {n} sources")
        if cubic:
            if item_index_dev is None or item_index_dev.numel() * item_index_dev.element_size() < 4 * n or \
                    spline.coef.numel() != arena.numel() or spline.coef.device != arena.device:
                raise ValueError(f'field "{name}": the spline tables are those of this arena, with one item index per patch')
            ind = spline.indicator
            check(lib.biu_augment_f32_crop_cubic(C.c_void_p(arena.data_ptr()), int(arena.dtype == torch.uint8), arena.numel(), C.c_void_p(spline.coef.data_ptr()),
                                                 C.c_void_p(ind.data_ptr()) if ind is not None else None, C.c_void_p(spline.table.data_ptr()), spline.n_items,
                                                 C.c_void_p(item_index_dev.data_ptr()), C.c_void_p(dst.data_ptr()), n, planes, th, tw,
                                                 C.c_void_p(params_dev.data_ptr()), C.c_void_p(sources_dev.data_ptr()), float(nan_to_val),
                                                 C.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)), "augment_f32_crop_cubic")
            return dst
        check(lib.biu_augment_f32_crop(C.c_void_p(arena.data_ptr()), int(arena.dtype == torch.uint8), arena.numel(), C.c_void_p(dst.data_ptr()),
                                       n, planes, th, tw, kind, C.c_void_p(params_dev.data_ptr()), C.c_void_p(sources_dev.data_ptr()),
                                       float(nan_to_val), max_blur if kind == KIND_IMAGE else 0, self.seed, int(epoch) & 0xFFFFFFFF,
                                       field_id(name), C.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)), "augment_f32_crop")
        return dst

    def _launch(self, lib, name, t, dst, planes, params_dev, max_blur, epoch, stream):
        kind = KINDS_F32[self.kind(name)]
        if kind == KIND_VECTOR and planes % 2:
            raise ValueError(f'field "{name}": a vector field holds (cos, sin) plane pairs, got {planes} plane(s)')
        if kind == KIND_MASK and self._any_rot:
            # coefficients (the field in fp32) and value range, allocated once per (field, shape, device) and reused: every augmentation
            # launch of a feeder runs on one stream, so the next batch's prefilter cannot overtake this batch's gather.  One augmenter
            # serves one feeder (or one caller) at a time.
            key = (name, tuple(t.shape), t.device)
            if key not in self._spline_scratch:
                self._spline_scratch[key] = (torch.empty(t.shape, dtype=torch.float32, device=t.device),
                                             torch.empty((t.shape[0], 2), dtype=torch.float32, device=t.device))
            coef, rng = self._spline_scratch[key]
            args = (t.shape[0], planes, t.shape[-2], t.shape[-1], C.c_void_p(params_dev.data_ptr()), stream)
            status = lib.biu_spline_prefilter_f32(C.c_void_p(t.data_ptr()), int(t.dtype == torch.uint8), C.c_void_p(coef.data_ptr()),
                                                  C.c_void_p(rng.data_ptr()), *args)
            return status or lib.biu_augment_f32_cubic(C.c_void_p(t.data_ptr()), int(t.dtype == torch.uint8), C.c_void_p(coef.data_ptr()),
                                                       C.c_void_p(rng.data_ptr()), C.c_void_p(dst.data_ptr()), *args)
        return lib.biu_augment_f32(C.c_void_p(t.data_ptr()), int(t.dtype == torch.uint8), C.c_void_p(dst.data_ptr()), t.shape[0], planes,
                                   t.shape[-2], t.shape[-1], kind, C.c_void_p(params_dev.data_ptr()), max_blur if kind == KIND_IMAGE else 0,
                                   self.seed, epoch, field_id(name), stream)


# =====================================================================================================================================
# float volumes: the 3-D multi-output family (``biu_augment_vol_f32``)
# =====================================================================================================================================
# The reference's pipeline for this family (``multi_output_unet3d/data.py:152-178``): ``ShiftScaleRotate(shift_limit=0, p=0.8)`` ->
# ``RandomCrop3D(dim_out)`` on the volume and every target (each declared ``mask3d``), then, with probability 0.8, slice by slice on the
# volume alone ``RandomBrightnessContrast(p=0.5)`` -> ``Blur(p=0.3)`` -> ``ShotNoise(p=0.5)`` -> ``GaussNoise(p=0.5)``.  Every z-plane of every
# channel gets the same in-plane map; nothing wraps:
#
# =========  ================================================================================================================
# kind       what the kernel does
# =========  ================================================================================================================
# "image"    bilinear gather, then brightness/contrast -> blur (of that result) -> shot noise -> Gauss noise (fp32, clipped to [0, 1])
# "mask"     any scalar target: nearest gather, nothing else
# "vector"   channel pairs ``(cos phi, sin phi)``, a volume apart: nearest gather, the pair is rotated by the record's rotation (phi - t)
# =========  ================================================================================================================
#
# The fields ``volume`` and ``image`` are images, a field named ``orientation`` a vector, every other field a mask; ``kinds={...}`` overrides.
BORDER_REFLECT, BORDER_CONSTANT = 0, 1                                        # include/biu.h: BIU_AUGV_*
BORDERS_VOL = {"reflect": BORDER_REFLECT, "constant": BORDER_CONSTANT}
STAGE_P_MO3D = {"shift_scale_rotate": 0.8, "intensity": 0.8, "brightness_contrast": 0.5, "blur": 0.3, "shot_noise": 0.5, "gauss_noise": 0.5}


# ---- whole volumes (``feed.VolumeStore``, ``biu_augment_vol_f32_crop``): the map goes from an output TILE pixel into the ITEM's (h, w) plane ------
SOURCE_VOL_DTYPE = np.dtype([("offset", "<u8"), ("d", "<i4"), ("h", "<i4"), ("w", "<i4"), ("z0", "<i4")])     # include/biu.h: biu_augv_source
assert SOURCE_VOL_DTYPE.itemsize == 24


def _vol_crop_matrix(angle, scale, ox, oy, h, w):
    # the whole-plane map of ``draw``'s record, then the crop: tile pixel (x, y) is plane pixel (x + ox, y + oy)
    m = _matrix(0, angle, scale, 0.0, 0.0, h, w)
    return tuple(v + 0.0 for v in _after(m, (1.0, 0.0, ox, 0.0, 1.0, oy)))      # origin (0, 0): ``_matrix``'s numbers bit for bit


def vol_crop_matrix(angle: float, scale: float, origin_xy, item_hw) -> np.ndarray:
    """float64 ``[m0 .. m5]``: pixel (x, y) of an output tile samples a plane of the ITEM ``[h, w]`` at ``(m0 x + m1 y + m2, m3 x + m4 y + m5)``:
    shift-scale-rotate of the whole plane about its centre (``inverse_matrix(0, angle, scale, 0, 0, h, w)``), then the crop at
    ``origin_xy = (ox, oy)``.  Whole-pixel cases are exact integers; with origin ``(0, 0)`` the map is ``inverse_matrix``'s bit for bit."""
    if not scale > 0:
        raise ValueError("scale must be positive")
    return np.array(_vol_crop_matrix(float(angle), float(scale), float(origin_xy[0]), float(origin_xy[1]), int(item_hw[0]), int(item_hw[1])))


def _pack_vol_crop(buf, offset, index, h, w, angle, scale, origin, blur_k, shot_s, gauss_sigma, bc):
    """``_pack_f32`` (no quarter turns, no shift) for a crop out of a whole plane ``[h, w]``: the same record and flags, ``m`` from
    ``_vol_crop_matrix``, ``dx, dy`` the crop origin."""
    flags = ((ROT_F if angle is not None else 0) | (SCALE_F if scale is not None else 0) | (BLUR_F if blur_k else 0)
             | (SHOT_F if shot_s is not None else 0) | (GAUSS_F if gauss_sigma is not None else 0) | (BC_F if bc is not None else 0))
    a = _f32(angle) if angle is not None else 0.0
    s = _f32(scale) if scale is not None else 1.0
    ox, oy = float(int(origin[0])), float(int(origin[1]))
    if a != 0:
        t = math.radians(a)
        ct, st = math.cos(t), math.sin(t)
    else:
        ct, st = 1.0, 0.0
    alpha, beta = bc if bc is not None else (1.0, 0.0)
    _REC_F32.pack_into(buf, offset, flags, 0, blur_k, index, *_vol_crop_matrix(a, s, ox, oy, h, w), ct + 0.0, st + 0.0, alpha, beta,
                       shot_s if shot_s is not None else 0.0, gauss_sigma if gauss_sigma is not None else 0.0, a, s, ox, oy)


def record_vol_crop(index: int, item_hw, *, angle: Optional[float] = None, scale: Optional[float] = None, origin=(0, 0), blur_k: int = 0,
                    shot_s: Optional[float] = None, gauss_sigma: Optional[float] = None, bc=None) -> np.ndarray:
    """One ``biu_augf_params`` record for ``biu_augment_vol_f32_crop`` from its logical description (``record_f32``'s without quarter turns,
    with ``origin = (ox, oy)`` the crop's first pixel in the transformed plane of an item ``item_hw``).  ``AugmenterVol.draw_crops`` builds
    its records the same way."""
    if blur_k and (blur_k % 2 == 0 or not 1 <= blur_k <= MAX_BLUR):
        raise ValueError(f"blur kernel {blur_k}: odd and at most {MAX_BLUR}")
    if shot_s is not None and not shot_s > 0:
        raise ValueError("shot noise needs a positive scale")
    if scale is not None and not scale > 0:
        raise ValueError("scale must be positive")
    buf = bytearray(_REC_F32.size)
    _pack_vol_crop(buf, 0, int(index), int(item_hw[0]), int(item_hw[1]), angle, scale, origin, int(blur_k), shot_s, gauss_sigma, bc)
    return np.frombuffer(buf, dtype=PARAMS_F32_DTYPE)[0]


class AugmenterVol(_AugmenterCore):
    """Draws ``biu_augf_params`` records on the host and runs ``biu_augment_vol_f32`` on device batches of float32 or uint8 volumes
    ``[B, D, H, W]`` or ``[B, C, D, H, W]`` (the output is always float32): the 3-D multi-output family's recipe ``"mo3d"``.

    Limits default to the reference constructor's.  ``border``: what lies outside a plane, ``"reflect"`` (reflect-101, albumentations 1.4's
    default for ``ShiftScaleRotate`` and what this package's uint8 recipes do) or ``"constant"`` (0, albumentations 2's default).  The blur's own
    border is always reflect-101, as ``cv2.blur``'s.  On a ``feed.TileStore`` ``RandomCrop3D(dim_out)`` is the identity: its tiles already have
    ``dim_out``, so ``draw`` has nothing to crop and no offset to draw.  On a ``feed.VolumeStore`` of whole volumes ``draw_crops`` places the crop:
    the same thirteen uniforms behind the same gates, then ``u[13], u[14], u[15]`` for ``z0, oy, ox`` (``biu_augment_vol_f32_crop``).

    ``draw`` takes thirteen uniforms per sample, in this order whatever the gates say:

    ==  ==================================================================================================
    u   use
    ==  ==================================================================================================
    0   shift-scale-rotate gate (< 0.8)
    1   scale: ``1 + scale_limit[0] + u (scale_limit[1] - scale_limit[0])``
    2   angle in degrees: ``rotate_limit[0] + u (rotate_limit[1] - rotate_limit[0])``, about the plane centre, ``_matrix``'s sign
    3   gate of the intensity block as a whole (< 0.8); the four gates below count only behind it
    4   brightness/contrast gate (< 0.5)
    5   contrast: ``alpha = 1 + (2 u - 1) brightness_contrast[1]``
    6   brightness: ``beta = (2 u - 1) brightness_contrast[0]``
    7   blur gate (< 0.3)
    8   blur size: one of the odd sizes in ``blur_limit``
    9   shot-noise gate (< 0.5)
    10  shot-noise scale in ``shot_noise_lims``
    11  Gauss-noise gate (< 0.5)
    12  Gauss-noise standard deviation in ``gauss_noise_lims``
    ==  ==================================================================================================
    """

    recipe = "mo3d"
    params_dtype, _rec, n_uniform, blur_flag = PARAMS_F32_DTYPE, _REC_F32, 13, BLUR_F
    allowed_kinds = tuple(KINDS_F32)
    store_attrs = ("scale_limit", "rotate_limit", "gauss_noise_lims", "shot_noise_lims", "brightness_contrast", "blur_limit")
    src_dtypes, dst_dtype, launch_name = (torch.float32, torch.uint8), torch.float32, "augment_vol_f32"
    field_dims, field_layout = (4, 5), "[B, D, H, W] or [B, C, D, H, W]"

    def __init__(self, *, scale_limit=(-0.75, 0), rotate_limit=(0, 360), gauss_noise_lims=(0.01, 0.1), shot_noise_lims=(0.005, 0.01),
                 brightness_contrast=(0.1, 0.1), blur_limit=(3, 7), border: str = "reflect", seed: int = 0,
                 kinds: Optional[Dict[str, str]] = None, shape: Optional[Sequence[int]] = None):
        sl, rl = _pair(scale_limit, "scale_limit"), _pair(rotate_limit, "rotate_limit")
        self.scale_limit = tuple(float(v) for v in ((-sl[0], sl[0]) if np.isscalar(scale_limit) else sl))
        self.rotate_limit = tuple(float(v) for v in ((-rl[0], rl[0]) if np.isscalar(rotate_limit) else rl))
        self.gauss_noise_lims = tuple(float(v) for v in _pair(gauss_noise_lims, "gauss_noise_lims"))
        self.shot_noise_lims = tuple(float(v) for v in _pair(shot_noise_lims, "shot_noise_lims"))
        self.brightness_contrast = tuple(float(v) for v in _pair(brightness_contrast, "brightness_contrast"))
        self.blur_limit = tuple(int(v) for v in _pair(blur_limit, "blur_limit"))
        if border not in BORDERS_VOL:
            raise ValueError(f'border "{border}": one of {sorted(BORDERS_VOL)}')
        self.border = border
        if self.blur_limit[1] > MAX_BLUR:
            raise ValueError(f"blur_limit {self.blur_limit}: box kernels above {MAX_BLUR} are not supported")
        self.blur_sizes = [k for k in range(max(3, self.blur_limit[0]), self.blur_limit[1] + 1) if k % 2]
        if not self.blur_sizes:
            raise ValueError(f"blur_limit {self.blur_limit} holds no odd kernel size of 3 or more")
        if not 0 < self.shot_noise_lims[0] <= self.shot_noise_lims[1]:
            raise ValueError("shot_noise_lims: positive scales, lower first")
        if not 0 <= self.gauss_noise_lims[0] <= self.gauss_noise_lims[1]:
            raise ValueError("gauss_noise_lims: standard deviations, lower first")
        if not -1 < self.scale_limit[0] <= self.scale_limit[1]:
            raise ValueError("scale_limit: 1 + limit must stay positive, lower first")
        if not self.rotate_limit[0] <= self.rotate_limit[1] or not all(math.isfinite(v) for v in self.rotate_limit):
            raise ValueError("rotate_limit: finite angles in degrees, lower first")
        self._init_core(seed, kinds, shape)

    @classmethod
    def _store_kw(cls, store, overrides):
        kw = super()._store_kw(store, {})
        if "image" not in store.fields and "volume" in store.fields:
            kw["shape"] = tuple(store.fields["volume"])
        kw.update(overrides)
        return kw

    @classmethod
    def from_store(cls, store, recipe: str = "mo3d", **overrides) -> "AugmenterVol":
        """Limits from the attributes a ``TileStore`` records, else the reference's defaults."""
        if recipe != "mo3d":
            raise ValueError(f'recipe "{recipe}" not defined for float volumes (only "mo3d")')
        return cls(**cls._store_kw(store, overrides))

    def describe(self) -> dict:
        return {"recipe": self.recipe, "seed": self.seed, "scale_limit": self.scale_limit, "rotate_limit": self.rotate_limit,
                "gauss_noise_lims": self.gauss_noise_lims, "shot_noise_lims": self.shot_noise_lims,
                "brightness_contrast": self.brightness_contrast, "blur_limit": self.blur_limit, "border": self.border,
                "stage_p": dict(STAGE_P_MO3D), "kinds": dict(self.kinds)}

    def kind(self, name: str) -> str:
        return self.kinds.get(name, "image" if name in ("volume", "image") else "vector" if name == "orientation" else "mask")

    def _packer(self, h, w):
        """``draw``'s record from thirteen uniforms (class docstring)."""
        lerp = lambda u, lim: lim[0] + u * (lim[1] - lim[0])
        P, sizes, bcl = STAGE_P_MO3D, self.blur_sizes, self.brightness_contrast
        scale_limit, rotate_limit, shot_lims, gauss_lims = self.scale_limit, self.rotate_limit, self.shot_noise_lims, self.gauss_noise_lims

        def pack(buf, offset, index, u):
            ssr, on = u[0] < P["shift_scale_rotate"], u[3] < P["intensity"]
            _pack_f32(buf, offset, index, h, w, 0, lerp(u[2], rotate_limit) if ssr else None, 1.0 + lerp(u[1], scale_limit) if ssr else None, (0, 0),
                      sizes[min(int(u[8] * len(sizes)), len(sizes) - 1)] if on and u[7] < P["blur"] else 0,
                      lerp(u[10], shot_lims) if on and u[9] < P["shot_noise"] else None,
                      lerp(u[12], gauss_lims) if on and u[11] < P["gauss_noise"] else None,
                      (1.0 + (2.0 * u[5] - 1.0) * bcl[1], (2.0 * u[6] - 1.0) * bcl[0]) if on and u[4] < P["brightness_contrast"] else None)
        return pack

    # ---- whole volumes: crops out of a ``feed.VolumeStore`` --------------------------------------------------------------------------------
    source_dtype, n_uniform_crop = SOURCE_VOL_DTYPE, 16

    def _crop_packer(self, d, h, w, td, th, tw, z0_out):
        """``draw_crops``' record from sixteen uniforms: ``u[0..12]`` are ``_packer``'s behind the same gates, so the logical fields equal
        ``draw``'s; ``u[13], u[14], u[15]`` ALWAYS place ``z0, oy, ox`` -- ``RandomCrop3D`` has ``p = 1`` -- as ``min(int(u (E - t + 1)), E - t)``
        in the item's own extent (``ShiftScaleRotate`` keeps it).  ``z0`` goes to ``z0_out[index]``: the record has no field for it."""
        lerp = lambda u, lim: lim[0] + u * (lim[1] - lim[0])
        P, sizes, bcl = STAGE_P_MO3D, self.blur_sizes, self.brightness_contrast
        scale_limit, rotate_limit, shot_lims, gauss_lims = self.scale_limit, self.rotate_limit, self.shot_noise_lims, self.gauss_noise_lims
        place = lambda u, e, t: min(int(u * (e - t + 1)), e - t)

        def pack(buf, offset, index, u):
            ssr, on = u[0] < P["shift_scale_rotate"], u[3] < P["intensity"]
            z0_out[offset // _REC_F32.size] = place(u[13], d, td)
            _pack_vol_crop(buf, offset, index, h, w, lerp(u[2], rotate_limit) if ssr else None, 1.0 + lerp(u[1], scale_limit) if ssr else None,
                           (place(u[15], w, tw), place(u[14], h, th)),
                           sizes[min(int(u[8] * len(sizes)), len(sizes) - 1)] if on and u[7] < P["blur"] else 0,
                           lerp(u[10], shot_lims) if on and u[9] < P["shot_noise"] else None,
                           lerp(u[12], gauss_lims) if on and u[11] < P["gauss_noise"] else None,
                           (1.0 + (2.0 * u[5] - 1.0) * bcl[1], (2.0 * u[6] - 1.0) * bcl[0]) if on and u[4] < P["brightness_contrast"] else None)
        return pack

    def draw_crops(self, epoch: int, patch_indices, store, offsets: Optional[Dict[str, np.ndarray]] = None):
        """Records and sources for the patches ``patch_indices`` of a ``feed.VolumeStore`` in epoch ``epoch``: a pure function of
        ``(seed, epoch, patch index)`` -- Philox key ``(seed, epoch)``, counter = the patch index, ``draw``'s stream, sixteen uniforms of
        which the first thirteen are ``draw``'s.  Returns ``(records [n], {field: sources [n]})``; a source is ``(element offset of the patch's
        item in the field's arena, d, h, w, z0)``.  ``offsets``: the per-item offsets ``store.to_device`` returned (default: the store's own)."""
        idx = np.atleast_1d(np.asarray(patch_indices, dtype=np.int64))
        items = np.atleast_1d(store.locate(idx))
        td, th, tw = (int(v) for v in store.dim_out)
        sizes, packers, item_of = store.sizes, {}, dict(zip(idx.tolist(), items.tolist()))
        z0 = np.zeros(len(idx), dtype=np.int32)

        def pack_of(j):
            dhw = tuple(int(v) for v in sizes[item_of[j]])
            if dhw not in packers:
                packers[dhw] = self._crop_packer(*dhw, td, th, tw, z0)
            return packers[dhw]

        records = self._records(epoch, idx, pack_of, self.n_uniform_crop)
        offsets = offsets if offsets is not None else store.offsets
        sources = {}
        for name in store.fields:
            src = np.empty(len(idx), dtype=SOURCE_VOL_DTYPE)
            src["offset"], src["d"], src["h"], src["w"], src["z0"] = np.asarray(offsets[name])[items], sizes[items, 0], sizes[items, 1], sizes[items, 2], z0
            sources[name] = src
        return records, sources

    def launch_crop(self, name, arena, dst, params_dev, sources_dev, nan_to_val, max_blur, epoch):
        """One ``biu_augment_vol_f32_crop`` launch on the current stream: field ``name`` of ``dst.shape[0]`` patches ``dst [n, C, td, th, tw]`` out
        of the 1-D device tensor ``arena``; ``params_dev`` / ``sources_dev``: the records and this field's sources on the device, as bytes."""
        from ._lib import check, lib
        kind = KINDS_F32[self.kind(name)]
        if arena.dtype not in self.src_dtypes or not arena.is_cuda or arena.dim() != 1 or not arena.is_contiguous():
            raise ValueError(f'field "{name}": the arena is a contiguous 1-D {_names(self.src_dtypes)} device tensor')
        if dst.dtype != torch.float32 or dst.dim() != 5 or not dst.is_contiguous() or dst.device != arena.device:
            raise ValueError(f'field "{name}": the output is a contiguous float32 tensor [n, C, td, th, tw] on the arena\'s device')
        n, channels, td, th, tw = dst.shape
        if kind == KIND_VECTOR and channels % 2:
            raise ValueError(f'field "{name}": a vector field holds (cos, sin) channel pairs, got {channels} channel(s)')
        if params_dev.numel() * params_dev.element_size() < n * PARAMS_F32_DTYPE.itemsize or \
                sources_dev.numel() * sources_dev.element_size() < n * SOURCE_VOL_DTYPE.itemsize:
            raise ValueError(f"{n} patches need {n} parameter records and {n} sources")
        check(lib.biu_augment_vol_f32_crop(C.c_void_p(arena.data_ptr()), int(arena.dtype == torch.uint8), arena.numel(), C.c_void_p(dst.data_ptr()),
                                           n, channels, td, th, tw, kind, BORDERS_VOL[self.border], C.c_void_p(params_dev.data_ptr()),
                                           C.c_void_p(sources_dev.data_ptr()), float(nan_to_val), max_blur if kind == KIND_IMAGE else 0, self.seed,
                                           int(epoch) & 0xFFFFFFFF, field_id(name), C.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)),
              "augment_vol_f32_crop")
        return dst

    def _launch(self, lib, name, t, dst, channels, params_dev, max_blur, epoch, stream):
        kind = KINDS_F32[self.kind(name)]
        if kind == KIND_VECTOR and channels % 2:
            raise ValueError(f'field "{name}": a vector field holds (cos, sin) channel pairs [B, 2 j, D, H, W], got {channels} channel(s)')
        return lib.biu_augment_vol_f32(C.c_void_p(t.data_ptr()), int(t.dtype == torch.uint8), C.c_void_p(dst.data_ptr()), t.shape[0], channels,
                                       t.shape[-3], t.shape[-2], t.shape[-1], kind, BORDERS_VOL[self.border], C.c_void_p(params_dev.data_ptr()),
                                       max_blur if kind == KIND_IMAGE else 0, self.seed, epoch, field_id(name), stream)
