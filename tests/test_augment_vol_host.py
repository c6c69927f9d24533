"""Volume augmentation of the 3-D multi-output family, the parts that need no GPU: the float64 oracle (``tests/augment_vol_oracle.py``) against
``scipy.ndimage`` (``affine_transform(mode='mirror' | 'grid-constant')``, ``uniform_filter(mode='mirror')``), purity and statistics of
``AugmenterVol.draw``, its constructor, and ``TrainerMo3d``'s ``augment`` keyword where it cannot work."""
import inspect

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import bio_image_unet_amd._lib as L
from bio_image_unet_amd import augment as A
from bio_image_unet_amd.feed import TileStore
from tests import augment_vol_oracle as VO

# angle in degrees, scale: the geometries of tests/test_gpu_augment_vol.py
GEOMETRY = [(17.3, 1), (151, 0.7313), (203.7, 0.4137), (359, 0.2913), (77.7, 0.5519), (0, 0.6137), (0, 0.9137), (0, 0.3371)]
SHAPES = ((19, 37), (70, 130), (48, 80), (96, 96))
ids = lambda s: "x".join(map(str, s))


def _rec(h, w, g, **kw):
    return A.record_f32(0, h, w, angle=g[0] if g[0] else None, scale=g[1] if g[1] != 1 else None, **kw)


def _coords(h, w, r):
    return VO.source_coords(h, w, int(r["rot_k"]), float(r["angle"]), float(r["scale"]), float(r["dx"]), float(r["dy"]))


def test_library_exports_and_binds_the_volume_augmentation():
    assert hasattr(L.lib._c, "biu_augment_vol_f32") and "biu_augment_vol_f32" in L.SIGNATURES
    assert len(L.SIGNATURES["biu_augment_vol_f32"][1]) == 16
    assert A.AugmenterVol.params_dtype is A.PARAMS_F32_DTYPE and A.AugmenterVol.params_dtype.itemsize == 104
    hdr = open(L.os.path.join(L.os.path.dirname(L._HERE), "include", "biu.h")).read()
    for name, val in (("BIU_AUGV_REFLECT", VO.REFLECT), ("BIU_AUGV_CONSTANT", VO.CONSTANT)):
        assert f"#define {name} {val}" in hdr, name
    assert A.BORDERS_VOL == {"reflect": VO.REFLECT, "constant": VO.CONSTANT}


# ---- the oracle against scipy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_oracle_gathers_equal_scipy_affine_transform(shape):
    h, w = shape
    x = np.random.default_rng(1).random((h, w))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for g in GEOMETRY:
        r = _rec(h, w, g)
        sx, sy = _coords(h, w, r)
        m = r["m"]                                               # the matrix a record hands the kernel is the same map
        assert np.abs(m[0] * xx + m[1] * yy + m[2] - sx).max() < 1e-9 and np.abs(m[3] * xx + m[4] * yy + m[5] - sy).max() < 1e-9, g
        mat, off = [[m[4], m[3]], [m[1], m[0]]], [m[5], m[2]]     # scipy counts (row, column)
        for border, mode in ((VO.REFLECT, "mirror"), (VO.CONSTANT, "grid-constant")):
            near, safe = VO.gather_nearest(x, sx, sy, border)
            want = ndi.affine_transform(x, mat, off, order=0, mode=mode, cval=0.0)
            assert safe.mean() >= 0.99 and np.array_equal(near[safe], want[safe]), (g, mode)
            lin = VO.gather_bilinear(x, sx, sy, border)
            assert np.abs(lin - ndi.affine_transform(x, mat, off, order=1, mode=mode, cval=0.0)).max() <= 1e-12, (g, mode)
    # reflect-101 itself, far from the image and on a one-pixel axis
    assert VO.reflect101(np.arange(-7, 11), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert not VO.reflect101(np.arange(-3, 4), 1).any()


def test_oracle_share_left_out_by_the_nearest_gathers():
    """At most 1 % of the pixels lie within 1e-3 of a rounding tie, for every shape and geometry the GPU tests use."""
    worst = 0.0
    for h, w in SHAPES:
        for g in GEOMETRY:
            sx, sy = _coords(h, w, _rec(h, w, g))
            worst = max(worst, 1.0 - VO.gather_nearest(np.zeros((h, w)), sx, sy, VO.REFLECT)[1].mean())
    print(f"largest share left out: {100 * worst:.3f} %")
    assert worst <= 0.01


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_oracle_box_blur_equals_uniform_filter_mirror(shape):
    h, w = shape
    x = np.random.default_rng(2).random((1, 2, h, w)).astype(np.float32)
    for k in (3, 5, 7, 15):
        for border in (VO.REFLECT, VO.CONSTANT):                  # the blur's border is the reflected output whatever the gather's border
            got, _ = VO.apply(x, A.record_f32(0, h, w, blur_k=k), VO.IMAGE, border, 0, 0, 0)
            for z in range(2):
                want = ndi.uniform_filter(x[0, z].astype(np.float64), size=k, mode="mirror")
                assert np.abs(got[0, z] - want).max() <= 1e-13, (k, z)


def test_oracle_stage_order_and_vector_pairs():
    h, w = 12, 20
    x = np.random.default_rng(3).random((1, 2, h, w)).astype(np.float32)
    r = A.record_f32(0, h, w, blur_k=3, bc=(1.3, 0.2))
    got, _ = VO.apply(x, r, VO.IMAGE, VO.REFLECT, 0, 0, 0)
    bc = np.clip(x.astype(np.float64) * float(np.float32(1.3)) + float(np.float32(0.2)), 0, 1)
    assert np.abs(got - VO.box_blur_reflect(bc, 3)).max() <= 1e-15          # brightness/contrast BEFORE the blur: the clip does not commute
    assert np.abs(got - np.clip(VO.box_blur_reflect(x.astype(np.float64), 3) * float(np.float32(1.3)) + float(np.float32(0.2)), 0, 1)).max() > 1e-3
    # the pair of a vector field is channels (2 j, 2 j + 1), a volume apart
    phi = np.random.default_rng(4).uniform(0, 2 * np.pi, (2, 3, h, w))
    pair = np.stack([np.cos(phi[0]), np.sin(phi[0]), np.cos(phi[1]), np.sin(phi[1])]).astype(np.float32)
    got, _ = VO.apply(pair, A.record_f32(0, h, w, rot_k=2), VO.VECTOR, VO.REFLECT, 0, 0, 0)
    for j in range(2):
        assert np.array_equal(got[2 * j], -np.rot90(pair[2 * j], 2, axes=(1, 2))) and np.array_equal(got[2 * j + 1], -np.rot90(pair[2 * j + 1], 2, axes=(1, 2)))


# ---- draw ------------------------------------------------------------------------------------------------------------------------------
def _aug(**kw):
    kw.setdefault("shape", (8, 64, 64))
    return A.AugmenterVol(**kw)


def test_defaults_are_the_reference_constructors():
    a = A.AugmenterVol()
    assert (a.scale_limit, a.rotate_limit, a.gauss_noise_lims, a.shot_noise_lims, a.brightness_contrast, a.blur_limit, a.border) == \
        ((-0.75, 0.0), (0.0, 360.0), (0.01, 0.1), (0.005, 0.01), (0.1, 0.1), (3, 7), "reflect")
    assert a.dst_dtype == torch.float32 and a.src_dtypes == (torch.float32, torch.uint8) and a.n_uniform == 13
    assert A.STAGE_P_MO3D == {"shift_scale_rotate": 0.8, "intensity": 0.8, "brightness_contrast": 0.5, "blur": 0.3, "shot_noise": 0.5, "gauss_noise": 0.5}
    d = a.describe()
    assert d["recipe"] == "mo3d" and d["border"] == "reflect" and d["stage_p"] == A.STAGE_P_MO3D and d["rotate_limit"] == (0.0, 360.0)
    # the two existing classes keep their layouts
    assert A.Augmenter.field_dims == A.AugmenterF32.field_dims == (3, 4) and A.AugmenterVol.field_dims == (4, 5)


def test_draw_is_a_pure_function_of_seed_epoch_index():
    a = _aug(seed=7)
    alone = [a.draw(3, [i]) for i in (5, 9, 2)]
    batch = a.draw(3, [5, 9, 2])
    other_order = a.draw(3, [2, 5, 9])
    for j, r in enumerate(alone):
        assert r[0].tobytes() == batch[j].tobytes()
    assert other_order[0].tobytes() == batch[2].tobytes() and other_order[1].tobytes() == batch[0].tobytes()
    assert _aug(seed=7).draw(3, [5])[0].tobytes() == batch[0].tobytes()
    idx = list(range(64))
    assert a.draw(3, idx).tobytes() != a.draw(4, idx).tobytes()
    assert a.draw(3, idx).tobytes() != _aug(seed=8).draw(3, idx).tobytes()
    assert np.array_equal(batch["index"], [5, 9, 2])
    # a drawn record says everything about itself: rebuilt from its logical fields it is the same bytes
    for r in a.draw(1, np.arange(300)):
        f = int(r["flags"])
        again = A.record_f32(int(r["index"]), 64, 64, angle=float(r["angle"]) if f & A.ROT_F else None, scale=float(r["scale"]) if f & A.SCALE_F else None,
                             blur_k=int(r["blur_k"]), shot_s=float(r["shot_s"]) if f & A.SHOT_F else None,
                             gauss_sigma=float(r["gauss_sigma"]) if f & A.GAUSS_F else None, bc=(float(r["alpha"]), float(r["beta"])) if f & A.BC_F else None)
        assert again.tobytes() == r.tobytes()


def test_draw_gate_frequencies_and_ranges():
    n = 20000
    a = _aug(seed=1, scale_limit=(-0.6, 0.1), rotate_limit=(-30, 200), gauss_noise_lims=(0.02, 0.2), shot_noise_lims=(0.002, 0.02),
             brightness_contrast=(0.15, 0.3), blur_limit=(3, 7))
    r = a.draw(0, np.arange(n))
    f = r["flags"]

    def within(count, total, p):
        print(f"count {count} of {total}, expected {total * p:.1f}, 4 sigma {4.0 * np.sqrt(total * p * (1 - p)):.1f}")
        assert abs(count - total * p) <= 4.0 * np.sqrt(total * p * (1 - p)), (count, total, p)
    ssr, blur, shot, gau, bc = ((f & b) != 0 for b in (A.ROT_F, A.BLUR_F, A.SHOT_F, A.GAUSS_F, A.BC_F))
    assert np.array_equal(ssr, (f & A.SCALE_F) != 0)                                    # one gate opens rotation and scale together
    for m, p in ((ssr, 0.8), (bc, 0.8 * 0.5), (blur, 0.8 * 0.3), (shot, 0.8 * 0.5), (gau, 0.8 * 0.5), (bc | blur | shot | gau, 0.8 * (1 - 0.5 * 0.7 * 0.5 * 0.5))):
        within(int(m.sum()), n, p)
    within(int((bc & shot).sum()), n, 0.8 * 0.25)                                       # inside the block the gates are independent
    within(int((ssr & bc).sum()), n, 0.8 * 0.4)                                         # and the block is independent of the geometry
    assert not r["rot_k"].any() and not r["dx"].any() and not r["dy"].any()             # shift_limit = 0, no quarter turns
    assert r["angle"][ssr].min() >= -30 and r["angle"][ssr].max() <= 200 and np.ptp(r["angle"][ssr]) > 229 and not r["angle"][~ssr].any()
    assert r["scale"][ssr].min() >= 0.4 - 1e-6 and r["scale"][ssr].max() <= 1.1 + 1e-6 and np.ptp(r["scale"][ssr]) > 0.69
    assert np.all(r["scale"][~ssr] == 1)
    assert set(np.unique(r["blur_k"][blur])) == {3, 5, 7} and not r["blur_k"][~blur].any()
    for k in (3, 5, 7):
        within(int((r["blur_k"][blur] == k).sum()), int(blur.sum()), 1 / 3)
    assert r["shot_s"][shot].min() >= 0.002 - 1e-9 and r["shot_s"][shot].max() <= 0.02 + 1e-9 and np.ptp(r["shot_s"][shot]) > 0.0178
    assert r["gauss_sigma"][gau].min() >= 0.02 - 1e-9 and r["gauss_sigma"][gau].max() <= 0.2 + 1e-8 and np.ptp(r["gauss_sigma"][gau]) > 0.178
    assert r["alpha"][bc].min() >= 0.7 - 1e-6 and r["alpha"][bc].max() <= 1.3 + 1e-6 and np.ptp(r["alpha"][bc]) > 0.59       # contrast limit 0.3
    assert np.abs(r["beta"][bc]).max() <= 0.15 + 1e-7 and np.abs(r["beta"][bc]).max() > 0.149                                # brightness limit 0.15
    assert np.all(r["alpha"][~bc] == 1) and np.all(r["beta"][~bc] == 0)
    still = ~ssr
    assert still.any() and np.array_equal(r["m"][still], np.broadcast_to(A.inverse_matrix(0, 0, 1, 0, 0, 64, 64), (int(still.sum()), 6)))
    # the angle turns about the plane centre with _matrix's sign, the scale is about the centre
    one = r[ssr][0]
    assert np.array_equal(one["m"], A.inverse_matrix(0, float(one["angle"]), float(one["scale"]), 0, 0, 64, 64))
    # the defaults: scale in [0.25, 1], angle in [0, 360]
    d = _aug(seed=2).draw(0, np.arange(4000))
    on = (d["flags"] & A.ROT_F) != 0
    assert d["scale"][on].min() >= 0.25 - 1e-6 and d["scale"][on].max() <= 1.0 and d["angle"][on].min() >= 0 and d["angle"][on].max() <= 360


class _Volumes(torch.utils.data.Dataset):
    """Items of the 3-D multi-output contract with the attributes ``DataProcess`` keeps."""
    dim_out, aug_factor, clip_threshold, scale_limit, rotate_limit = (4, 16, 16), 2, (0.0, 99.99), (-0.5, 0.0), (0, 180)
    gauss_noise_lims, shot_noise_lims, brightness_contrast, blur_limit, random_rotate = (0.02, 0.2), (0.002, 0.02), (0.15, 0.2), (3, 5), True

    def __init__(self, n):
        rng = np.random.default_rng(0)
        phi = rng.uniform(0, 2 * np.pi, (n, 4, 16, 16))
        self.items = [{"volume": torch.from_numpy(np.round(rng.random((4, 16, 16)) * 255).astype(np.float32) / np.float32(255)),
                       "mask": torch.from_numpy((rng.random((4, 16, 16)) > 0.5).astype(np.float32)),
                       "orientation": torch.from_numpy(np.stack([np.cos(phi[i]), np.sin(phi[i])]).astype(np.float32))} for i in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_from_store_reads_the_attributes(tmp_path):
    ds = _Volumes(5)
    st = TileStore.from_dataset(str(tmp_path / "v"), ds, dtypes={"mask": "f32", "orientation": "f32"})
    assert st.dtypes == {"volume": "u8", "mask": "f32", "orientation": "f32"} and st.attrs["rotate_limit"] == [0, 180]
    a = A.AugmenterVol.from_store(st, seed=9)
    assert (a.scale_limit, a.rotate_limit, a.gauss_noise_lims, a.shot_noise_lims, a.brightness_contrast, a.blur_limit) == \
        ((-0.5, 0.0), (0.0, 180.0), (0.02, 0.2), (0.002, 0.02), (0.15, 0.2), (3, 5))
    assert a.shape == (4, 16, 16) and a.seed == 9 and a.blur_sizes == [3, 5] and a.border == "reflect"
    assert A.AugmenterVol.from_store(st, border="constant", blur_limit=(3, 7)).describe()["border"] == "constant"
    # the shape comes from `volume` (or `image`), not from whichever field is first
    st2 = TileStore.create(str(tmp_path / "w"), 2, {"orientation": (2, 4, 8, 12), "volume": (4, 8, 12)}, {"dim_out": [4, 8, 12]}, dtypes={"orientation": "f32"})
    assert A.AugmenterVol.from_store(st2).shape == (4, 8, 12)
    with pytest.raises(ValueError):
        A.AugmenterVol.from_store(st, "mo2d")


def test_augmenter_vol_arguments_and_kinds():
    a = _aug()
    assert (a.kind("volume"), a.kind("image"), a.kind("orientation"), a.kind("mask"), a.kind("distance")) == ("image", "image", "vector", "mask", "mask")
    assert A.AugmenterVol(kinds={"orientation": "mask"}).kind("orientation") == "mask"
    for bad in (dict(blur_limit=(3, 17)), dict(blur_limit=(4, 4)), dict(kinds={"x": "volume"}), dict(shot_noise_lims=(0.0, 0.1)), dict(scale_limit=(-1.5, 0.0)),
                dict(scale_limit=(0.2, 0.1)), dict(rotate_limit=(10, 0)), dict(rotate_limit=(0, float("inf"))), dict(gauss_noise_lims=(0.2, 0.1)),
                dict(border="wrap"), dict(brightness_contrast=(0.1, 0.1, 0.1))):
        with pytest.raises(ValueError):
            A.AugmenterVol(**bad)
    with pytest.raises(ValueError):
        A.AugmenterVol().draw(0, [0])                           # no tile shape


def test_trainer_mo3d_augment_keyword(tmp_path):
    from bio_image_unet_amd.workflow import TrainerMo3d
    par = list(inspect.signature(TrainerMo3d.__init__).parameters.values())
    assert par[-1].name == "augment" and par[-1].default is None
    assert [p.name for p in par[:-1]] == ["self", "dataset", "output_heads", "num_epochs", "network", "use_interpolation", "batch_size", "lr", "in_channels",
                                          "n_filter", "dilation", "val_split", "save_dir", "save_name", "save_iter", "load_weights", "loss_function",
                                          "loss_params", "time_loss_weight", "device", "fp32_products"]
    assert [p.default for p in par[5:-1]] == [False, 4, 1e-3, 1, 64, 1, 0.2, "./", "model.pt", False, False, "BCEDice", (0.5, 0.5), 0.1, "auto", None]
    heads = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0}}
    with pytest.raises(ValueError, match="TileStore"):
        TrainerMo3d(_Volumes(4), heads, 1, n_filter=4, save_dir=str(tmp_path / "a"), device="cuda", augment=True)
    st = TileStore.from_dataset(str(tmp_path / "st"), _Volumes(4), dtypes={"mask": "f32", "orientation": "f32"})
    with pytest.raises(ValueError, match="GPU"):
        TrainerMo3d(st, heads, 1, n_filter=4, save_dir=str(tmp_path / "b"), device="cpu", augment=True)
