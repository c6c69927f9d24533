"""The host arithmetic of the Predict classes against fixtures written by the reference's own constructors
(``tests/golden/predict_pins_*.npz``, recipe ``tests/golden/make_golden_predict_pins.py``): before any kernel runs, the port's counts,
start vectors, patch count and the bytes of the patches it cuts from the normalised input are the reference's.  No GPU: bare objects
(``cls.__new__`` plus the attributes the constructor would set) and the host ``_split``s."""
import json
import os

import numpy as np
import pytest

from bio_image_unet_amd import workflow as W
from tests import predict_pin_stub as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(f, n) for f, fam in S.GEOMETRIES.items() for n in fam]


def load(family):
    z = np.load(os.path.join(GOLDEN, f"predict_pins_{family}.npz"))
    return z, json.loads(bytes(z["meta_json"]).decode())


def _bare(cls, **attrs):
    obj = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


@pytest.mark.parametrize("family", list(S.GEOMETRIES))
def test_pin_fixture_is_the_stubs(family):
    z, meta = load(family)
    want = json.loads(json.dumps(S.meta()))
    assert {k: meta[k] for k in want} == want and meta["family"] == family
    assert set(meta["facts"]) == set(S.GEOMETRIES[family])
    for name, geo in S.GEOMETRIES[family].items():
        x = S.make_input(geo)
        assert x.shape == geo["shape"] and x.dtype == np.dtype(geo["dtype"])
        assert int(z[f"{name}.input_crc32"]) == S.crc32(x) == meta["facts"][name]["input_crc32"]
        # the fixture can fail a wrong stitcher: where tiles overlap, at least a tenth of those pixels see tiles that disagree
        over, dis = int(z[f"{name}.overlapped"]), int(z[f"{name}.disagreeing"])
        assert over == 0 or dis * 10 >= over
    # each geometry reaches the branch it is there for
    f = meta["facts"]
    if family == "unet":
        assert (f["truncated_linspace"]["X_start"], f["truncated_linspace"]["Y_start"]) == ([0, 10, 21], [0, 17, 35, 53])
        assert z["reflect_rows_two_channels.result"].shape == (2, 20, 100)
        assert not np.array_equal(z["first.result"], z["all.result"])
    if family == "unet3d":
        g = f["compounded_add_patch"]
        assert (g["N_z"], g["N_x"], g["N_y"], g["n_patches"]) == (4, 6, 5, 120) and g["max_cover"] > 3 and g["plain_mean_differs"] > 0
        assert g["plain_mean_differs"] == int((z["compounded_add_patch.plain_mean"] != z["compounded_add_patch.result"]).sum())
        g = f["reflect_z_x"]
        assert (g["N_z"], g["N_x"], g["N_y"]) == (1, 1, 3)
    if family == "siam":
        assert f["pairs_2x2"]["n_patches"] == 12 and f["constant_padding"]["n_patches"] == 3 and f["one_frame"]["n_patches"] == 9
    if family == "mo2d":
        assert f["fill_2x2"]["fill_pixels"] > 0 and f["one_tile_reflect"]["fill_pixels"] == 0 and f["one_tile_reflect"]["patch_size"] == [32, 48]
        assert f["drift"]["X_start"] == [0, 26, 53] and f["drift"]["cut_origin_differs"] > 1000 * f["drift"]["bound"]["a"]
        assert (f["row_surplus"]["N_x"], f["row_surplus"]["N_y"], f["row_surplus"]["n_patches"]) == (3, 4, 16)
        assert (f["column_surplus"]["N_x"], f["column_surplus"]["N_y"], f["column_surplus"]["n_patches"]) == (4, 3, 16)
        for name, g in f.items():
            assert g["max_weighted_tiles"] <= 4
            for k, d in g["unweighted_differs"].items():
                assert d > 1000 * g["bound"][k], (name, k)


def _host_patches(family, geo):
    """(bare object after its host split, the patches): the constructor's host path up to the model, without a device."""
    x = S.make_input(geo)
    if family == "unet":
        p = _bare(W.Predict2D, imgs_shape=x.shape, resize_dim=tuple(geo["resize_dim"]), add_tile=geo["add_tile"])
        imgs = np.array(x, dtype=np.float64 if x.dtype.kind != "f" else x.dtype)
        return p, p._split(W.normalise_stack(imgs, geo["mode"], (0., 99.8), geo["invert"]))
    if family == "unet3d":
        p = _bare(W.Predict3D, vol_shape=x.shape, resize_dim=tuple(geo["resize_dim"]), add_patch=geo["add_patch"])
        return p, p._split(W.normalise_stack(x, "all", (0., 99.8), geo["invert"]))
    if family == "siam":
        p = _bare(W.PredictSiam, imgs_shape=list(x.shape), tif_len=x.shape[0], resize_dim=tuple(geo["resize_dim"]), add_tile=geo["add_tile"])
        return p, np.concatenate([p._pair_patches(x, i, geo["mode"], (0., 99.8), geo["invert"]) for i in range(x.shape[0])])
    p = _bare(W.PredictMo2d, imgs_shape=x.shape, max_patch_size=tuple(geo["max_patch_size"]), add_tile=geo["add_tile"])
    return p, p._split(W.PredictMo2d._preprocess(np.array(x, dtype="float32"), "single", (0., 99.98)))


@pytest.mark.parametrize("family,name", CASES)
def test_host_split_is_the_references(family, name):
    z, _ = load(family)
    geo = S.GEOMETRIES[family][name]
    if family == "mo2d" and name in S.MO2D_REFUSED:
        # upstream cut 16 windows for 4 x 3 tiles and reshaped the first 12: a scrambled image, which the port refuses, naming the geometry
        with pytest.raises(ValueError, match=r"4 windows for N_y = 3 tiles \(images \(1, 100, 51\), max_patch_size \(48, 48\), add_tile 1\)"):
            _host_patches(family, geo)
        return
    p, patches = _host_patches(family, geo)
    for key in ("N_z", "N_x", "N_y"):
        if f"{name}.{key}" in z:
            assert getattr(p, key) == int(z[f"{name}.{key}"]), key
    for key in ("Z_start", "X_start", "Y_start"):
        if f"{name}.{key}" in z:
            assert list(map(int, getattr(p, key))) == z[f"{name}.{key}"].tolist(), key
    if family == "mo2d":
        assert list(p.patch_size) == z[f"{name}.patch_size"].tolist()
    assert len(patches) == int(z[f"{name}.n_patches"])
    assert patches.dtype == (np.float32 if family == "mo2d" else np.uint8)
    assert S.crc32(patches) == int(z[f"{name}.patches_crc32"])


def test_mo2d_surplus_windows_are_predicted_and_not_stitched():
    """``row_surplus``: 4 x 4 windows for 3 x 4 tiles.  The surplus row is cut (it counts in the fill mean, as upstream's) and has no place."""
    geo = S.GEOMETRIES["mo2d"]["row_surplus"]
    p = _bare(W.PredictMo2d, imgs_shape=geo["shape"], max_patch_size=geo["max_patch_size"], add_tile=geo["add_tile"])
    origins = p._origins()
    assert len(origins) == 16 and p.N == p.N_per_img == 12
    assert [p._place(k) for k in range(12)] == [(0, (0, int(xs), int(ys))) for xs in p.X_start for ys in p.Y_start]
    assert [p._place(k) for k in range(12, 16)] == [None] * 4
    assert [o[2] for o in origins[12:]] == [3] * 4          # the fourth window row of the stride X_start[1] = 1


def test_mo2d_refuses_a_surplus_with_several_images():
    """Upstream separates the images by ``N_x * N_y`` while the patch list is longer: patches of image 0 would be stitched into image 1."""
    geo = S.GEOMETRIES["mo2d"]["row_surplus"]
    p = _bare(W.PredictMo2d, imgs_shape=(2,) + tuple(geo["shape"][1:]), max_patch_size=geo["max_patch_size"], add_tile=geo["add_tile"])
    with pytest.raises(ValueError, match=r"4 windows for N_x = 3 tiles \(images \(2, 51, 100\)"):
        p._origins()
