"""``PredictMo3d``'s ramp blend against the reference's own stitcher (``tests/golden/mo3d_blend.npz``, written by
``tests/golden/make_golden_mo3d_blend.py`` from ``multi_output_unet3d/predict.py``'s ``__preprocess`` / ``__split`` / ``__stitch``).

The stub network's output depends on the position inside the patch (``tests/mo3d_blend_stub.py``), so overlapping patches disagree about a
voxel and the result is decided by ``PredictMo3d._weights`` (the restated index arithmetic of the reference's ramps), by the weight plane
reaching ``wsum`` in ``biu_stitch_add``, by the patch origins and by ``biu_stitch_finish``'s float mode.

Bound, derived and not measured: a voxel is covered by at most 2 x 2 x 2 = 8 patches (stride >= half a patch on every axis).  Reference and
device both form one rounded fp32 product per patch (the device may fuse it into the addition, which only removes a rounding), add them
in the same order (7 additions for the numerator, 7 for the weights, whose multiples of 1/16 add exactly) and divide once.  All terms are
non-negative, so every partial sum is at most the final one and each of the 8 + 7 + 1 = 16 roundings moves the quotient by at most
2^-24 of its own value on either side: |device - reference| <= 16 x 2^-24 x max|fixture| per head."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mo3d_blend_stub as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mo3d_blend.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z["meta_json"]).decode())


def test_blend_fixture_is_the_stubs(golden):
    z, meta = golden
    assert meta["heads"] == S.HEADS and {k: tuple(v) for k, v in meta["coef"].items()} == S.COEF and meta["ramp_seed"] == S.RAMP_SEED
    assert set(meta["geometries"]) == set(S.GEOMETRIES)
    for name, geo in S.GEOMETRIES.items():
        m = meta["geometries"][name]
        assert tuple(m["volume"]) == geo["volume"] and tuple(m["patch"]) == geo["patch"] and m["overlap"] == geo["overlap"] and m["seed"] == geo["seed"]
        assert int(z[f"{name}.volume_crc32"]) == S.volume_checksum(S.make_volume(geo["volume"], geo["seed"]))
    m = meta["geometries"]["plateau_appended_start"]
    assert (m["Z_start"], m["Y_start"], m["X_start"]) == ([0, 6, 12], [0, 24, 40], [0, 8])


def _unweighted_mean(p, vol, head):
    """Mean of the stub's CPU patch outputs over the patches that cover a voxel, every weight 1: what a stitcher without ramps gives."""
    from bio_image_unet_amd.workflow import PredictMo3d
    x = PredictMo3d._preprocess(np.array(vol, dtype="float32")[None], "single", (0., 99.98))[0]
    pd, ph, pw = p.patch_size
    a, b = S.COEF[head]
    ramp = S.make_ramp(p.patch_size).astype(np.float64)
    acc, cnt = np.zeros(x.shape), np.zeros(x.shape)
    for z in p.Z_start:
        for y in p.Y_start:
            for xs in p.X_start:
                acc[z:z + pd, y:y + ph, xs:xs + pw] += a * x[z:z + pd, y:y + ph, xs:xs + pw] + b * ramp
                cnt[z:z + pd, y:y + ph, xs:xs + pw] += 1
    assert cnt.min() >= 1 and cnt.max() >= 4
    return acc / cnt


@pytest.mark.parametrize("name", list(S.GEOMETRIES))
def test_predict_mo3d_blend_matches_reference_stitcher(golden, name):
    from bio_image_unet_amd.workflow import PredictMo3d
    z, _ = golden
    geo = S.GEOMETRIES[name]
    vol = S.make_volume(geo["volume"], geo["seed"])
    assert S.volume_checksum(vol) == int(z[f"{name}.volume_crc32"])
    p = PredictMo3d(vol.copy(), S.checkpoint(), network=S.PositionStub, max_patch_size=geo["patch"], overlap_factor=geo["overlap"],
                    batch_size=S.BATCH_SIZE, show_progress=False, device="cuda")
    for ax in ("Z_start", "Y_start", "X_start"):
        assert list(map(int, getattr(p, ax))) == z[f"{name}.{ax}"].tolist(), ax
    D, H, W = geo["volume"]
    zero = np.unpackbits(z[f"{name}.zero_weight"])[:D * H * W].astype(bool).reshape(D, H, W)
    assert int(zero.sum()) == int(z[f"{name}.zero_weight_voxels"])
    for k, head in S.HEADS.items():
        want, got = z[f"{name}.result.{k}"], p.result[k]
        assert got.shape == want.shape == ((D, H, W) if head["channels"] == 1 else (head["channels"], D, H, W)) and got.dtype == np.float32
        bound = 16 * 2.0 ** -24 * float(np.abs(want).max())
        dev = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print(f"mo3d blend {name} head {k}: worst deviation {dev:.3e} (bound {bound:.3e}), zero-weight voxels {int(zero.sum())}")
        assert dev <= bound, (name, k, dev, bound)
        # (neither geometry leaves a voxel without weight, the fixture says so: this line holds for a fixture that has some; the zero-weight
        # branch of biu_stitch_finish is asserted in tests/test_gpu_io_ops.py::test_io_stitch_float_weighted_blend)
        assert np.all(got.reshape(-1, D, H, W)[:, zero] == 0)
        # the blend matters: the plain mean of the covering patches is far outside the bound, so the test can tell the weights
        plain = _unweighted_mean(p, vol, k)
        assert float(np.abs(plain - want.reshape(-1, D, H, W)[0]).max()) > 1000 * bound
    assert float(np.abs(z[f"{name}.result.b"][0] - z[f"{name}.result.b"][1]).max()) == 0          # the stub repeats one map over b's channels
    assert np.array_equal(p.result["b"][0], p.result["b"][1])
