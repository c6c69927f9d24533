"""Float augmentation and feed of the 2-D multi-output family, the parts that need no GPU: the float tile store, the float64 oracle
(``tests/augment_f32_oracle.py``) against the reference's own library calls (``scipy.ndimage.rotate(mode='grid-wrap')``, ``uniform_filter``,
``np.rot90``), purity and statistics of ``AugmenterF32.draw``, the oracle's Poisson sampler, and ``TrainerMo2d``'s refusal of ``augment=True``
where it cannot work."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import bio_image_unet_amd._lib as L
from bio_image_unet_amd import augment as A
from bio_image_unet_amd.feed import TileStore
from tests import augment_f32_oracle as FO

ANGLES = (17.3, 151.0, 203.7, 359.0)                     # away from multiples of 45 degrees: no exact rounding ties
SHAPES = ((64, 64), (48, 80), (256, 256))


def test_library_exports_and_binds_the_float_augmentation():
    assert hasattr(L.lib._c, "biu_augment_f32") and "biu_augment_f32" in L.SIGNATURES
    assert C.sizeof(L.biu_augf_params) == A.PARAMS_F32_DTYPE.itemsize == 104
    assert [n for n, _ in L.biu_augf_params._fields_] == list(A.PARAMS_F32_DTYPE.names)
    for name, _ in L.biu_augf_params._fields_:                     # the numpy record and the C struct agree field by field
        assert A.PARAMS_F32_DTYPE.fields[name][1] == getattr(L.biu_augf_params, name).offset, name
        assert A.PARAMS_F32_DTYPE.fields[name][0].itemsize == getattr(L.biu_augf_params, name).size, name
    assert (A.ROT_F, A.SCALE_F, A.BLUR_F, A.SHOT_F, A.GAUSS_F, A.BC_F) == (FO.ROT, FO.SCALE, FO.BLUR, FO.SHOT, FO.GAUSS, FO.BC)
    assert (A.KIND_IMAGE, A.KIND_MASK, A.KIND_VECTOR) == (FO.IMAGE, FO.MASK, FO.VECTOR)
    hdr = open(L.os.path.join(L.os.path.dirname(L._HERE), "include", "biu.h")).read()
    for name, val in (("BIU_AUGF_ROT", FO.ROT), ("BIU_AUGF_BLUR", FO.BLUR), ("BIU_AUGF_SHOT", FO.SHOT), ("BIU_AUGF_GAUSS", FO.GAUSS), ("BIU_AUGF_BC", FO.BC),
                      ("BIU_AUGF_STAGE_SHOT", FO.STAGE_SHOT), ("BIU_AUGF_STAGE_GAUSS", FO.STAGE_GAUSS), ("BIU_AUGF_POISSON_CAP", FO.POISSON_CAP),
                      ("BIU_AUGF_VECTOR", FO.VECTOR)):
        assert f"#define {name} {val}" in hdr, name


# ---- the float tile store ----------------------------------------------------------------------------------------------------------------
class _Items(torch.utils.data.Dataset):
    """Items of the multi-output contract: an image in [0, 1], a distance map beyond 1, a (cos, sin) field in [-1, 1]."""
    dim_out, aug_factor, clip_threshold, gauss_noise_lims, shot_noise_lims = (12, 20), 2, (0.0, 99.99), (0.02, 0.2), (0.002, 0.02)
    brightness_contrast, blur_limit, random_rotate, scale_limit = (0.15, 0.2), (3, 7), True, (-0.1, 0.2)

    def __init__(self, n, nan_at=None):
        rng = np.random.default_rng(0)
        phi = rng.uniform(0, 2 * np.pi, (n, 12, 20))
        self.items = [{"image": torch.from_numpy(np.round(rng.random((12, 20)) * 255).astype(np.float32) / np.float32(255)),
                       "distance": torch.from_numpy((rng.random((12, 20)) * 37.5 - 3.0).astype(np.float32)),
                       "orientation": torch.from_numpy(np.stack([np.cos(phi[i]), np.sin(phi[i])]).astype(np.float32))} for i in range(n)]
        if nan_at is not None:
            self.items[nan_at]["distance"][3, 4] = float("nan")

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_float_store_round_trip(tmp_path):
    ds = _Items(7)
    st = TileStore.from_dataset(str(tmp_path / "mo"), ds, dtypes={"distance": "f32", "orientation": "f32"})       # a mixed store: the image is bytes
    assert st.dtypes == {"image": "u8", "distance": "f32", "orientation": "f32"}
    assert st.fields == {"image": (12, 20), "distance": (12, 20), "orientation": (2, 12, 20)}
    assert (tmp_path / "mo.image.u8").exists() and (tmp_path / "mo.distance.f32").exists() and (tmp_path / "mo.orientation.f32").exists()
    st = TileStore(str(tmp_path / "mo"))                                                                          # reopened read-only
    for i in range(7):
        item = st[i]
        for k in ("image", "distance", "orientation"):
            assert item[k].dtype == torch.float32
            assert item[k].numpy().tobytes() == ds[i][k].numpy().tobytes(), (i, k)                                # bit for bit, sign and range included
    assert float(st[0]["orientation"].min()) < -0.5 and float(st[0]["distance"].max()) > 1.5
    idx = [5, 0, 3]
    got = st.batch_u8(idx)
    assert got["image"].dtype == torch.uint8 and got["distance"].dtype == torch.float32 and got["orientation"].shape == (3, 2, 12, 20)
    for j, i in enumerate(idx):
        assert got["distance"][j].numpy().tobytes() == ds[i]["distance"].numpy().tobytes()
        assert got["orientation"][j].numpy().tobytes() == ds[i]["orientation"].numpy().tobytes()
        assert np.array_equal(got["image"][j].numpy(), np.rint(ds[i]["image"].numpy() * 255).astype(np.uint8))
    into = {k: torch.empty((4,) + st.fields[k], dtype=got[k].dtype) for k in got}                                 # the feeder's gather into its own buffers
    res = st.batch_host(idx, out=into)
    assert all(res[k].numpy().tobytes() == got[k].numpy().tobytes() for k in got)
    # the multi-output attributes travel in the header
    for a in ("gauss_noise_lims", "shot_noise_lims", "blur_limit", "random_rotate", "scale_limit", "brightness_contrast", "clip_threshold"):
        assert st.attrs[a] == (list(getattr(ds, a)) if isinstance(getattr(ds, a), tuple) else getattr(ds, a)), a
    assert st.random_rotate is True and st.dim_out == (12, 20)
    # all fields as float
    sf = TileStore.from_dataset(str(tmp_path / "allf"), ds, dtypes="f32")
    assert set(sf.dtypes.values()) == {"f32"} and sf[2]["image"].numpy().tobytes() == ds[2]["image"].numpy().tobytes()
    aug = A.AugmenterF32.from_store(st)
    assert aug.gauss_noise_lims == (0.02, 0.2) and aug.scale_limit == (-0.1, 0.2) and aug.blur_sizes == [3, 5, 7] and aug.shape == (12, 20)


def test_float_store_refuses_non_finite_values_and_unknown_dtypes(tmp_path):
    with pytest.raises(ValueError, match="distance"):
        TileStore.from_dataset(str(tmp_path / "nan"), _Items(4, nan_at=2), dtypes={"distance": "f32", "orientation": "f32"})
    with pytest.raises(ValueError):
        TileStore.create(str(tmp_path / "bad"), 2, {"image": (4, 4)}, dtypes={"image": "f16"})
    with pytest.raises(ValueError):
        TileStore.create(str(tmp_path / "bad2"), 2, {"image": (4, 4)}, dtypes={"mask": "f32"})


def test_uint8_stores_keep_their_header(tmp_path):
    st = TileStore.create(str(tmp_path / "u"), 3, {"image": (8, 8), "mask": (8, 8)}, {"dim_out": [8, 8]})
    st.maps["image"][:] = np.arange(3 * 64, dtype=np.uint8).reshape(3, 8, 8)
    st.flush()
    hdr = json.load(open(str(tmp_path / "u.json")))
    assert sorted(hdr) == ["attrs", "fields", "magic", "n"] and hdr["magic"] == "biu-tilestore-1"                # exactly the keys of every earlier store
    assert st.dtypes == {"image": "u8", "mask": "u8"}
    # a header written before float fields existed (no dtype key) opens as all-uint8
    with open(str(tmp_path / "old.json"), "w") as f:
        json.dump({"magic": "biu-tilestore-1", "n": 3, "fields": {"image": [8, 8]}, "attrs": {}}, f)
    np.arange(3 * 64, dtype=np.uint8).tofile(str(tmp_path / "old.image.u8"))
    old = TileStore(str(tmp_path / "old"))
    assert old.dtypes == {"image": "u8"} and old.maps["image"].dtype == np.uint8
    assert torch.equal(old[1]["image"], torch.from_numpy(np.arange(64, 128, dtype=np.float32).reshape(8, 8) / 255.0))
    # a store with float fields names them in the optional key
    TileStore.create(str(tmp_path / "f"), 2, {"image": (4, 4), "d": (4, 4)}, dtypes={"d": "f32"})
    assert json.load(open(str(tmp_path / "f.json")))["dtypes"] == {"image": "u8", "d": "f32"}


# ---- the oracle against the reference's library calls -------------------------------------------------------------------------------------
def _rec(h, w, **kw):
    return A.record_f32(0, h, w, **kw)


def _coords(h, w, r, halo=0):
    return FO.source_coords(h, w, int(r["rot_k"]), float(r["angle"]), float(r["scale"]), float(r["dx"]), float(r["dy"]), halo)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_gathers_equal_scipy_rotate_grid_wrap(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    h, w = shape
    x = np.random.default_rng(1).random((h, w))
    for angle in ANGLES:
        a32 = float(np.float32(angle))                           # the angle a record carries
        sx, sy = _coords(h, w, _rec(h, w, angle=angle))
        near, _ = FO.gather_nearest(x, sx, sy)
        assert np.array_equal(near, ndi.rotate(x, a32, reshape=False, mode="grid-wrap", order=0)), angle
        lin = FO.gather_bilinear(x, sx, sy)
        assert np.abs(lin - ndi.rotate(x, a32, reshape=False, mode="grid-wrap", order=1)).max() <= 1e-12, angle
        # ... and the matrix a record hands the kernel is the same map
        m = _rec(h, w, angle=angle)["m"]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        assert np.abs(m[0] * xx + m[1] * yy + m[2] - sx).max() < 1e-9 and np.abs(m[3] * xx + m[4] * yy + m[5] - sy).max() < 1e-9
    if h == w:
        for k in range(4):
            sx, sy = _coords(h, w, _rec(h, w, rot_k=k))
            assert np.array_equal(FO.gather_nearest(x, sx, sy)[0], np.rot90(x, k))
        assert np.array_equal(ndi.rotate(x, 90, reshape=False, mode="grid-wrap", order=0), np.rot90(x, 1))
    # scale, shift and quarter turns: the record's matrix against the oracle's coordinates
    for kw in (dict(scale=1.0731, shift=(5, -3)), dict(angle=151.0, scale=0.9137, shift=(-4, 6)), dict(rot_k=2, angle=17.3, scale=1.19, shift=(2, 1)),
               dict(rot_k=1 if h == w else 2, scale=0.8, shift=(0, 7))):
        r = _rec(h, w, **kw)
        sx, sy = _coords(h, w, r)
        m = r["m"]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        assert np.abs(m[0] * xx + m[1] * yy + m[2] - sx).max() < 1e-9 and np.abs(m[3] * xx + m[4] * yy + m[5] - sy).max() < 1e-9, kw
    # a whole-pixel shift wraps: np.roll
    sx, sy = _coords(h, w, _rec(h, w, shift=(5, -3)))
    assert np.array_equal(FO.gather_nearest(x, sx, sy)[0], np.roll(x, (-3, 5), axis=(0, 1)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_box_blur_equals_uniform_filter_grid_wrap(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    h, w = shape
    x = np.random.default_rng(2).random((1, h, w)).astype(np.float32)
    for k in (3, 5, 7, 15):
        got, _ = FO.apply(x, _rec(h, w, blur_k=k), FO.IMAGE, 0, 0, 0)
        want = ndi.uniform_filter(x[0].astype(np.float64), size=k, mode="grid-wrap")
        assert np.abs(got[0] - want).max() <= 1e-13, k


def test_oracle_vector_rule_equals_the_rotated_angle_field():
    ndi = pytest.importorskip("scipy.ndimage")
    h = w = 64
    phi = np.random.default_rng(3).uniform(0, 2 * np.pi, (h, w))
    pair = np.stack([np.cos(phi), np.sin(phi)]).astype(np.float32)
    for angle in ANGLES:
        r = _rec(h, w, angle=angle)
        a32 = float(r["angle"])
        got, _ = FO.apply(pair, r, FO.VECTOR, 0, 0, 0)
        rot = ndi.rotate(phi, a32, reshape=False, mode="grid-wrap", order=0) - np.radians(a32)        # data.py:268-273 with order=0
        # fp32 pair in, fp32 (cos t, sin t) in the record: 3 roundings of 2^-24 on numbers <= sqrt(2)
        assert np.abs(got[0] - np.cos(rot)).max() <= 4e-7 and np.abs(got[1] - np.sin(rot)).max() <= 4e-7, angle
    for k in range(4):
        r = _rec(h, w, rot_k=k)
        got, _ = FO.apply(pair, r, FO.VECTOR, 0, 0, 0)
        rot = np.rot90(phi, k) - k * np.pi / 2                                                       # data.py:276-282
        assert np.abs(got[0] - np.cos(rot)).max() <= 4e-7 and np.abs(got[1] - np.sin(rot)).max() <= 4e-7, k
        c, s = np.rot90(pair[0], k).astype(np.float64), np.rot90(pair[1], k).astype(np.float64)
        want = [(c, s), (s, -c), (-c, -s), (-s, c)][k]                                               # sign-and-swap, bit for bit
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (float(r["cos_t"]), float(r["sin_t"])) == [(1, 0), (0, 1), (-1, 0), (0, -1)][k]
    zero = np.zeros((2, h, w), dtype=np.float32)                                                     # nan_to_val = 0 stays (0, 0)
    assert not FO.apply(zero, _rec(h, w, angle=17.3), FO.VECTOR, 0, 0, 0)[0].any()


# ---- draw ------------------------------------------------------------------------------------------------------------------------------
def _aug(**kw):
    kw.setdefault("shape", (64, 64))
    kw.setdefault("scale_limit", (-0.2, 0.25))
    kw.setdefault("blur_limit", (3, 7))
    return A.AugmenterF32(**kw)


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
        again = A.record_f32(int(r["index"]), 64, 64, rot_k=int(r["rot_k"]), angle=float(r["angle"]) if f & A.ROT_F else None,
                             scale=float(r["scale"]) if f & A.SCALE_F else None, shift=(int(r["dx"]), int(r["dy"])), blur_k=int(r["blur_k"]),
                             shot_s=float(r["shot_s"]) if f & A.SHOT_F else None, gauss_sigma=float(r["gauss_sigma"]) if f & A.GAUSS_F else None,
                             bc=(float(r["alpha"]), float(r["beta"])) if f & A.BC_F else None)
        assert again.tobytes() == r.tobytes()


def test_draw_stage_frequencies_and_limits():
    n = 20000
    a = _aug(seed=1, gauss_noise_lims=(0.02, 0.2), shot_noise_lims=(0.002, 0.02), brightness_contrast=(0.15, 0.3))
    r = a.draw(0, np.arange(n))
    f = r["flags"]

    def within(count, total, p):
        assert abs(count - total * p) <= 5.0 * np.sqrt(total * p * (1 - p)), (count, total, p)
    rot, scl, blur, shot, gau, bc = ((f & b) != 0 for b in (A.ROT_F, A.SCALE_F, A.BLUR_F, A.SHOT_F, A.GAUSS_F, A.BC_F))
    for m, p in ((rot, 0.5), (scl, 0.75), (blur, 0.25), (shot, 0.25), (gau, 0.25), (bc, 0.5)):
        within(m.sum(), n, p)
    assert not r["rot_k"][rot].any()                                         # either an arbitrary angle or a quarter turn
    for k in range(4):
        within((r["rot_k"][~rot] == k).sum(), int((~rot).sum()), 0.25)
    assert r["angle"][rot].min() >= 0 and r["angle"][rot].max() <= 360 and np.ptp(r["angle"][rot]) > 359 and not r["angle"][~rot].any()
    assert r["scale"][scl].min() >= 0.8 - 1e-6 and r["scale"][scl].max() <= 1.25 + 1e-6 and np.ptp(r["scale"][scl]) > 0.44
    assert np.all(r["scale"][~scl] == 1) and not r["dx"][~scl].any() and not r["dy"][~scl].any()
    # the crop offset: whole pixels, inside what the up-scaled tile leaves over, none for a down-scaled one
    assert np.array_equal(r["dx"], np.rint(r["dx"])) and np.array_equal(r["dy"], np.rint(r["dy"]))
    room = np.maximum(np.rint(64 * r["scale"].astype(np.float64)) - 64, 0)
    assert np.all(np.abs(r["dx"]) <= room / 2 + 0.5) and np.all(np.abs(r["dy"]) <= room / 2 + 0.5) and np.abs(r["dx"]).max() >= 7
    assert set(np.unique(r["blur_k"][blur])) == {3, 5, 7} and not r["blur_k"][~blur].any()
    for k in (3, 5, 7):
        within((r["blur_k"][blur] == k).sum(), int(blur.sum()), 1 / 3)
    assert r["shot_s"][shot].min() >= 0.002 - 1e-9 and r["shot_s"][shot].max() <= 0.02 + 1e-9 and np.ptp(r["shot_s"][shot]) > 0.0178
    assert r["gauss_sigma"][gau].min() >= 0.02 - 1e-9 and r["gauss_sigma"][gau].max() <= 0.2 + 1e-8 and np.ptp(r["gauss_sigma"][gau]) > 0.178
    assert r["alpha"][bc].min() >= 0.7 - 1e-6 and r["alpha"][bc].max() <= 1.3 + 1e-6 and np.ptp(r["alpha"][bc]) > 0.59       # contrast limit 0.3
    assert np.abs(r["beta"][bc]).max() <= 0.15 + 1e-7 and np.abs(r["beta"][bc]).max() > 0.149                                # brightness limit 0.15
    assert np.all(r["alpha"][~bc] == 1) and np.all(r["beta"][~bc] == 0)
    # the identity where nothing was drawn
    still = ~rot & ~scl & (r["rot_k"] == 0)
    assert still.any() and np.array_equal(r["m"][still], np.broadcast_to(A.inverse_matrix(0, 0, 1, 0, 0, 64, 64), (int(still.sum()), 6)))
    # random_rotate=False draws no rotation at all; odd quarter turns only on square tiles
    s = _aug(seed=2, random_rotate=False).draw(0, np.arange(2000))
    assert not (s["flags"] & A.ROT_F).any() and not s["rot_k"].any() and np.all(s["cos_t"] == 1) and np.all(s["sin_t"] == 0)
    assert set(np.unique(_aug(seed=3).draw(0, np.arange(2000), shape=(64, 96))["rot_k"])) == {0, 2}


def test_augmenter_f32_arguments_and_kinds():
    a = _aug()
    assert (a.kind("image"), a.kind("orientation"), a.kind("mask"), a.kind("distance")) == ("image", "vector", "mask", "mask")
    assert A.AugmenterF32(kinds={"flow": "vector"}).kind("flow") == "vector"
    assert a.describe()["recipe"] == "mo2d" and a.describe()["scale_limit"] == (-0.2, 0.25)
    for bad in (dict(blur_limit=(3, 17)), dict(kinds={"x": "volume"}), dict(shot_noise_lims=(0.0, 0.1)), dict(scale_limit=(-1.5, 0.0))):
        with pytest.raises(ValueError):
            A.AugmenterF32(**bad)
    with pytest.raises(ValueError):
        A.record_f32(0, 8, 8, blur_k=4)
    with pytest.raises(ValueError):
        A.record_f32(0, 8, 12, rot_k=1)
    with pytest.raises(ValueError):
        A.AugmenterF32().draw(0, [0])                           # no tile shape


# ---- the oracle's Poisson sampler ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.5, 5.0, 31.9, 32.0, 400.0])
def test_oracle_poisson_sampler_mean_and_variance(lam):
    n = 1 << 18
    u1, u2 = FO.stage_uniforms(n, 0xC0FFEE, 11, 2, 99, FO.STAGE_SHOT)
    k = FO.poisson(np.full(n, lam), u1, u2)
    var = lam if lam < 32 else lam + 1.0 / 12.0                # rounding a normal to integers adds the variance of a uniform on one unit
    mu4 = lam * (1 + 3 * lam)                                  # fourth central moment of a Poisson variable
    se_mean, se_var = np.sqrt(var / n), np.sqrt((mu4 - var * var) / n)
    print(f"lambda {lam}: mean {k.mean():.5f} (se {se_mean:.5f}), variance {k.var():.5f} (se {se_var:.5f}), max {k.max()}")
    assert np.array_equal(k, np.rint(k)) and k.min() >= 0
    assert abs(k.mean() - lam) <= 5 * se_mean
    assert abs(k.var() - var) <= 5 * se_var


def test_trainer_mo2d_refuses_augment_without_store_or_gpu(tmp_path):
    from bio_image_unet_amd.workflow import TrainerMo2d
    heads = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0}}
    with pytest.raises(ValueError, match="TileStore"):
        TrainerMo2d(_Items(4), 1, output_heads=heads, n_filter=4, save_dir=str(tmp_path / "a"), device="cuda", augment=True)
    st = TileStore.from_dataset(str(tmp_path / "st"), _Items(4), dtypes="f32")
    with pytest.raises(ValueError, match="GPU"):
        TrainerMo2d(st, 1, output_heads=heads, n_filter=4, save_dir=str(tmp_path / "b"), device="cpu", augment=True)
