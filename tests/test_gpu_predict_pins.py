"""The Predict classes, start to finish on the device, against results of the reference's own constructors
(``tests/golden/predict_pins_*.npz``, written on the CPU by ``tests/golden/make_golden_predict_pins.py``).

The stub networks (``tests/predict_pin_stub.py``) add a seeded ramp of the patch extent, so overlapping tiles disagree about a pixel and the
result is decided by the origins, the tile order, the three overwrite layers of the 3-D stitcher, the frame pairing of the Siam family and
the safe-margin weights and fill of the 2-D multi-output family -- none of it restated here.

uint8 families (2-D, 3-D, Siam): equality, no tolerance.  Every stage is exact: ``byte / 255`` correctly rounded, stub operations that round
once (power-of-two products, one ``add`` each), truncation to uint8, and an integer mean whose float64 (2-D, Siam) or float16 (3-D: a sum of
at most three bytes, exact below 2048, over 1, 2 or 3) quotient cannot cross an integer.  ``preprocess='device'`` is held to the same
equality for the uint16 inputs, as the class docstrings promise.

2-D multi-output: |device - fixture| <= 9 x 2^-24 x max|fixture| per head, derived and not measured.  Patches are float16 values on both
sides (the same bits: the stub rounds once in fp32 and float32 -> float16 is round-to-nearest-even in numpy and on the device); a pixel
has at most 4 tiles with weight (the fixtures record at most 3), each contributing one product with a weight of 0 or 1 and one fp32
addition, then one division: 4 + 4 + 1 = 9 roundings of at most 2^-24 relative each, and since every term is non-negative each partial
sum is at most the final one, so each rounding moves the quotient by at most 2^-24 of its own value.  Pixels without weight hold the
float16 mean of ALL the head's patches and must equal the fixture exactly (the recipe checks that the float64 mean, which the port forms,
and numpy's float16 mean round to the same float16).  With ``preprocess='device'`` the input is rounded once from fp64 where numpy works in
float32; a few float32 ulps there can move a patch value's float16 rounding to the neighbouring value and no further, so the bound gains
one float16 ulp below 1, 2^-11 (as ``test_gpu_workflow.py::test_predict_mo2d_batches_cross_images_stub`` derives), on the weighted pixels
and on the fill."""
import json
import os
import time

import numpy as np
import pytest

from tests import predict_pin_stub as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREPROCESS = {"uint16": ["host", "device"], "float32": ["host"]}


def _cases(family):
    return [(n, pp) for n, g in S.GEOMETRIES[family].items() for pp in PREPROCESS[g["dtype"]]]


@pytest.fixture(scope="module")
def golden():
    t0, loaded = time.time(), {}
    for family in S.GEOMETRIES:
        z = np.load(os.path.join(GOLDEN, f"predict_pins_{family}.npz"))
        loaded[family] = (z, json.loads(bytes(z["meta_json"]).decode()))
        assert loaded[family][1]["geometries"] == json.loads(json.dumps(S.meta()))["geometries"]
    yield loaded
    print(f"\ntest_gpu_predict_pins.py: {time.time() - t0:.1f} s wall (fixtures written with numpy {loaded['unet'][1]['numpy']}, here {np.__version__})")


def _input(z, name, geo):
    x = S.make_input(geo)
    assert S.crc32(x) == int(z[f"{name}.input_crc32"])
    return x


def _equal(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (tag, got.shape, got.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{tag}: {len(bad)} of {want.size} pixels differ, first at {bad[0].tolist()}: "
                           f"{int(got[tuple(bad[0])])} for the reference's {int(want[tuple(bad[0])])}")


@pytest.mark.parametrize("name,preprocess", _cases("unet"))
def test_predict2d_is_the_references(golden, name, preprocess):
    from bio_image_unet_amd.workflow import Predict2D
    z, _ = golden["unet"]
    geo = S.GEOMETRIES["unet"][name]
    p = Predict2D(_input(z, name, geo), None, S.checkpoint("unet", geo), network=S.StubU8, resize_dim=geo["resize_dim"], invert=geo["invert"],
                  normalization_mode=geo["mode"], add_tile=geo["add_tile"], show_progress=False, device="cuda", batch_size=5,
                  preprocess=preprocess)
    assert (p.N_x, p.N_y) == (int(z[f"{name}.N_x"]), int(z[f"{name}.N_y"]))
    assert p.X_start.tolist() == z[f"{name}.X_start"].tolist() and p.Y_start.tolist() == z[f"{name}.Y_start"].tolist()
    assert len(p.origins) == int(z[f"{name}.n_patches"])
    _equal(p.imgs_result, z[f"{name}.result"], f"unet {name} {preprocess}")


@pytest.mark.parametrize("name,preprocess", _cases("unet3d"))
def test_predict3d_is_the_references(golden, name, preprocess):
    from bio_image_unet_amd.workflow import Predict3D
    z, _ = golden["unet3d"]
    geo = S.GEOMETRIES["unet3d"][name]
    p = Predict3D(_input(z, name, geo), None, S.checkpoint("unet3d", geo), network=S.StubU8, resize_dim=geo["resize_dim"], invert=geo["invert"],
                  add_patch=geo["add_patch"], progress_bar=False, device="cuda", preprocess=preprocess)
    assert (p.N_z, p.N_x, p.N_y, p.N) == tuple(int(z[f"{name}.{k}"]) for k in ("N_z", "N_x", "N_y", "n_patches"))
    for ax in ("Z_start", "X_start", "Y_start"):
        assert getattr(p, ax).tolist() == z[f"{name}.{ax}"].tolist(), ax
    _equal(p.vol_result, z[f"{name}.result"], f"unet3d {name} {preprocess}")
    # the three overwrite layers decide: the nan-mean over all covering patches is another volume, in the number of voxels the recipe found
    differs = int((p.vol_result != z[f"{name}.plain_mean"]).sum())
    assert differs == int(z[f"{name}.plain_mean_differs"]) and (differs > 0 or p.N <= 3)


@pytest.mark.parametrize("name,preprocess", _cases("siam"))
def test_predict_siam_is_the_references(golden, monkeypatch, name, preprocess):
    import bio_image_unet_amd.workflow as W
    monkeypatch.setattr(W, "Siam_UNet", S.StubSiam)                 # the family's model class is fixed
    z, _ = golden["siam"]
    geo = S.GEOMETRIES["siam"][name]
    p = W.PredictSiam(_input(z, name, geo), None, S.checkpoint("siam", geo), resize_dim=geo["resize_dim"], invert=geo["invert"],
                      normalization_mode=geo["mode"], add_tile=geo["add_tile"], show_progress=False, device="cuda", batch_size=4,
                      preprocess=preprocess)
    assert (p.N_x, p.N_y) == (int(z[f"{name}.N_x"]), int(z[f"{name}.N_y"])) and p.N * geo["shape"][0] == int(z[f"{name}.n_patches"])
    assert p.X_start.tolist() == z[f"{name}.X_start"].tolist() and p.Y_start.tolist() == z[f"{name}.Y_start"].tolist()
    _equal(p.imgs_result, z[f"{name}.result"], f"siam {name} {preprocess}")


@pytest.mark.parametrize("name,preprocess", [c for c in _cases("mo2d") if c[0] not in S.MO2D_REFUSED])
def test_predict_mo2d_is_the_references(golden, name, preprocess):
    from bio_image_unet_amd.workflow import PredictMo2d
    z, meta = golden["mo2d"]
    geo, facts = S.GEOMETRIES["mo2d"][name], meta["facts"][name]
    p = PredictMo2d(_input(z, name, geo), S.checkpoint("mo2d", geo), network=S.StubHeads2D, max_patch_size=geo["max_patch_size"],
                    batch_size=S.MO2D_BATCH, add_tile=geo["add_tile"], show_progress=False, device="cuda", preprocess=preprocess)
    assert list(p.patch_size) == facts["patch_size"] and (p.N_x, p.N_y) == (facts["N_x"], facts["N_y"])
    assert p.X_start.tolist() == facts["X_start"] and p.Y_start.tolist() == facts["Y_start"] and len(p.origins) == facts["n_patches"]
    n_img, h, w = geo["shape"]
    # the pixels without weight, from the start vectors and the safe margin alone
    ws = np.zeros((max(p.patch_size[0], h), max(p.patch_size[1], w)))
    for j, xs in enumerate(facts["X_start"]):
        for k, ys in enumerate(facts["Y_start"]):
            ws[xs:xs + p.patch_size[0], ys:ys + p.patch_size[1]] += PredictMo2d.weight_plane(j, k, p.N_x, p.N_y, p.patch_size)
    unweighted = ws[:h, :w] == 0
    assert int(unweighted.sum()) == facts["fill_pixels"] and facts["max_weighted_tiles"] <= 4
    ulp16 = 2.0 ** -11 if preprocess == "device" else 0.0
    for k, head in S.HEADS.items():
        want = z[f"{name}.result.{k}"]
        got = p.result[k]
        assert got.shape == want.shape and got.dtype == np.float32, (k, got.shape, got.dtype)
        g4, w4 = got.reshape(n_img, head["channels"], h, w).astype(np.float64), want.reshape(n_img, head["channels"], h, w).astype(np.float64)
        bound = 9 * 2.0 ** -24 * float(np.abs(want).max()) + ulp16
        assert abs(bound - ulp16 - facts["bound"][k]) < 1e-15
        dev = float(np.abs(g4 - w4)[:, :, ~unweighted].max())
        fill_dev = float(np.abs(g4 - w4)[:, :, unweighted].max()) if unweighted.any() else 0.0
        print(f"mo2d pin {name} ({preprocess}) head {k}: worst deviation {dev:.3e} (bound {bound:.3e}); fill pixels {int(unweighted.sum())}, "
              f"fill deviation {fill_dev:.3e} (allowed {ulp16:.3e})")
        assert dev <= bound, (name, k, dev, bound)
        assert fill_dev <= ulp16, (name, k, fill_dev)
        if unweighted.any() and preprocess == "host":
            assert np.all(got.reshape(n_img, head["channels"], h, w)[:, :, unweighted] == np.float32(facts["fill"][k]))
    # the weights and the origins decide: with every weight 1, or stitched where the windows were cut, head a is far outside the bound
    # (1000 x the blend bound is 4e-4; the distances are 0.3 and more, far beyond the device path's 2^-11 as well)
    assert (f"{name}.unweighted.a" in z) == (p.N_per_img > 1)
    if p.N_per_img > 1:
        assert float(np.abs(p.result["a"].astype(np.float64) - z[f"{name}.unweighted.a"]).max()) > 1000 * facts["bound"]["a"] > 0
    if name == "drift":
        assert float(np.abs(p.result["a"].astype(np.float64) - z["drift.cut_origin.a"]).max()) > 1000 * facts["bound"]["a"]


@pytest.mark.parametrize("name", S.MO2D_REFUSED)
def test_predict_mo2d_refuses_what_upstream_scrambles(golden, name):
    """The fixture records upstream's image for the column surplus (16 windows reshaped to 4 x 3 tiles); the port raises before any kernel."""
    from bio_image_unet_amd.workflow import PredictMo2d
    z, meta = golden["mo2d"]
    geo, facts = S.GEOMETRIES["mo2d"][name], meta["facts"][name]
    assert facts["n_patches"] > facts["N_x"] * facts["N_y"]
    for preprocess in ("host", "device"):
        with pytest.raises(ValueError, match="windows for N_y = 3 tiles"):
            PredictMo2d(_input(z, name, geo), S.checkpoint("mo2d", geo), network=S.StubHeads2D, max_patch_size=geo["max_patch_size"],
                        batch_size=S.MO2D_BATCH, add_tile=geo["add_tile"], show_progress=False, device="cuda", preprocess=preprocess)
