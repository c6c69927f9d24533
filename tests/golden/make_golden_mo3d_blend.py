"""Generate ``mo3d_blend.npz`` in this directory with the REFERENCE's own patch splitter and stitcher of the 3-D multi-output Predict.

Run in the build container only (the reference is absent on the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mo3d_blend.py

``multi_output_unet3d/predict.py`` is loaded by file path.  It imports ``tifffile`` (not installed) and, relatively, ``..progress``,
``..utils`` and the model module, so placeholder modules for those and for the parent packages are registered in ``sys.modules`` first; none
of them is used by the three methods driven here.  A bare ``Predict`` is made with ``object.__new__`` and given the attributes its
constructor would set; then its own ``__preprocess``, ``__split`` and ``__stitch`` run, with the CPU float32 outputs of
``tests/mo3d_blend_stub.PositionStub`` in place of ``__predict``.  ``__preprocess`` calls ``ndarray.ptp()``, which numpy 2 removed: the volume
is handed over as an ndarray subclass that has the method back (``np.ptp`` of the same data), the reference's code is unchanged.

The zero-weight voxels are found with the same stitcher: patches of ones stitch to 1 wherever the weight sum is positive and to 0
elsewhere.  Only tensors and settings leave this script.

  meta_json                        {"geometries": {name: {volume, patch, overlap, seed, Z_start, Y_start, X_start, zero_weight_voxels,
                                    volume_crc32}}, "heads", "coef", "ramp_seed", "blend_margin"}
  <geometry>.result.<head>         stitched float32 volume per head ((D, H, W), or (channels, D, H, W))
  <geometry>.Z_start / .Y_start / .X_start
  <geometry>.zero_weight           bit-packed mask (np.packbits of the (D, H, W) mask) of the voxels whose weight sum is 0
  <geometry>.zero_weight_voxels    their count
  <geometry>.volume_crc32          crc32 of the float32 input volume's bytes (the test regenerates the volume from the seed)
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mo3d_blend_stub as S  # noqa: E402

REF = "/root/reference/bio_image_unet"


def load_reference_predict():
    def placeholder(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class ProgressNotifier:
        @staticmethod
        def progress_notifier_tqdm():
            return None

    placeholder("tifffile")
    placeholder("bio_image_unet").__path__ = []
    placeholder("bio_image_unet.multi_output_unet3d").__path__ = []
    placeholder("bio_image_unet.multi_output_unet3d.multi_output_unet3d", MultiOutputUnet3D=None)
    placeholder("bio_image_unet.progress", ProgressNotifier=ProgressNotifier)
    placeholder("bio_image_unet.utils", get_device=lambda: torch.device("cpu"))
    name = "bio_image_unet.multi_output_unet3d.predict"
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "multi_output_unet3d/predict.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _WithPtp(np.ndarray):
    """numpy 2 dropped ``ndarray.ptp``; ``Predict.__preprocess`` calls it on the clipped volume (``np.clip`` keeps the subclass)."""

    def ptp(self, *a, **k):
        return np.ptp(np.asarray(self), *a, **k)


def run(R, geo):
    p = object.__new__(R.Predict)
    p.max_patch_size, p.overlap_factor, p.batch_size = tuple(geo["patch"]), geo["overlap"], S.BATCH_SIZE
    p.normalization_mode, p.clip_threshold = "single", (0., 99.98)
    p.target_keys = list(S.HEADS.keys())
    p.model_params = {"output_heads": S.HEADS}
    vol = S.make_volume(geo["volume"], geo["seed"])
    imgs = vol.astype("float32")[None]                       # what __reshape_data makes of a (D, H, W) volume
    p.imgs_shape = imgs.shape
    imgs = np.asarray(p._Predict__preprocess(imgs.view(_WithPtp)))
    assert imgs.dtype == np.float32 and imgs.min() == 0 and imgs.max() <= 1
    patches = p._Predict__split(imgs)
    net = S.PositionStub(output_heads=S.HEADS)
    with torch.no_grad():
        outs = [net(torch.tensor(patches[b:b + S.BATCH_SIZE], dtype=torch.float32)) for b in range(0, len(patches), S.BATCH_SIZE)]
    result_patches = {k: np.concatenate([o[k].numpy() for o in outs]) for k in p.target_keys}
    result = p._Predict__stitch(result_patches)
    ones = p._Predict__stitch({k: np.ones_like(v) for k, v in result_patches.items()})
    zero = ones["a"] == 0
    assert set(np.unique(ones["a"])) <= {0.0, 1.0} and np.array_equal(ones["b"][0] == 0, zero)
    for k in p.target_keys:
        assert result[k].dtype == np.float32 and np.all(result[k].reshape(-1, *zero.shape)[:, zero] == 0)
    return p, vol, result, zero


def main():
    R = load_reference_predict()
    arrays, meta = {}, {"geometries": {}, "heads": S.HEADS, "coef": S.COEF, "ramp_seed": S.RAMP_SEED, "blend_margin": 16}
    for name, geo in S.GEOMETRIES.items():
        p, vol, result, zero = run(R, geo)
        for k, v in result.items():
            arrays[f"{name}.result.{k}"] = v
        for ax in ("Z_start", "Y_start", "X_start"):
            arrays[f"{name}.{ax}"] = np.asarray(getattr(p, ax), dtype=np.int64)
        arrays[f"{name}.zero_weight"] = np.packbits(zero)
        arrays[f"{name}.zero_weight_voxels"] = np.int64(zero.sum())
        arrays[f"{name}.volume_crc32"] = np.int64(S.volume_checksum(vol))
        meta["geometries"][name] = dict(geo, Z_start=list(map(int, p.Z_start)), Y_start=list(map(int, p.Y_start)), X_start=list(map(int, p.X_start)),
                                        zero_weight_voxels=int(zero.sum()), volume_crc32=int(S.volume_checksum(vol)))
        print(name, "Z", p.Z_start, "Y", p.Y_start, "X", p.X_start, "zero-weight voxels", int(zero.sum()),
              {k: (v.shape, float(np.abs(v).max())) for k, v in result.items()})
    arrays["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "mo3d_blend.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
