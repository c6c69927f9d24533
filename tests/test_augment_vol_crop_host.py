"""Host side of the whole-volume crop augmentation, without a GPU: the oracle (``tests/augment_vol_crop_oracle.py``) against ``scipy.ndimage``,
``augment.vol_crop_matrix`` against the oracle's coordinates, ``feed.VolumeStore``, ``AugmenterVol.draw_crops`` and every refusal of
``dataprep.prepare_mo3d`` and of the Trainer that needs no device."""
import math

import numpy as np
import pytest
import torch

from bio_image_unet_amd import augment as A
from bio_image_unet_amd import dataprep
from bio_image_unet_amd.feed import CropFeeder, ImageStore, VolumeStore
from tests import augment_vol_crop_oracle as CO

GEOMETRY = [(17.3, 1), (151, 0.7313), (203.7, 0.4137), (359, 0.2913), (77.7, 0.5519), (0, 0.6137), (0, 0.9137), (0, 0.3371)]
ITEM, TILE = (7, 70, 90), (3, 50, 61)


def _rec(i, hw, g, **kw):
    return A.record_vol_crop(i, hw, angle=g[0] if g[0] else None, scale=g[1] if g[1] != 1 else None, **kw)


def _scipy_map(rec, h, w):
    """(matrix, offset) of ``scipy.ndimage.affine_transform`` in (row, column) order for the inverse of the forward map the module docstring of
    ``augment.py`` states, written down here from that formula and the record's logical fields."""
    t, sc = math.radians(float(rec["angle"])), float(rec["scale"])
    c, s = math.cos(t) / sc, math.sin(t) / sc
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    mat = np.array([[c, s], [-s, c]])                 # sy = c (y - cy) + s (x - cx) + cy, sx = -s (y - cy) + c (x - cx) + cx
    return mat, np.array([cy, cx]) - mat @ np.array([cy, cx])


@pytest.mark.parametrize("border,mode", [(CO.REFLECT, "mirror"), (CO.CONSTANT, "grid-constant")])
def test_oracle_gathers_equal_scipy_then_slice(border, mode):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    item = rng.random((2,) + ITEM).astype(np.float32)
    d, h, w = ITEM
    origins = [(0, 0, 0), (d - TILE[0], h - TILE[1], w - TILE[2]), (2, 11, 17)]
    for i, g in enumerate(GEOMETRY):
        z0, oy, ox = origins[i % 3]
        rec = _rec(i, (h, w), g, origin=(ox, oy))
        mat, off = _scipy_map(rec, h, w)
        for kind, order in ((CO.IMAGE, 1), (CO.MASK, 0)):
            whole = np.stack([[ndimage.affine_transform(item[c, z].astype(np.float64), mat, off, order=order, mode=mode, cval=0.0) for z in range(d)]
                              for c in range(2)])
            want = whole[:, z0:z0 + TILE[0], oy:oy + TILE[1], ox:ox + TILE[2]]
            got, safe = CO.apply(item, rec, z0, TILE, kind, border, 0.0, 1, 2, 3)
            diff = np.abs(got - want)
            if kind == CO.IMAGE:
                print(f"scipy {mode} {g} order 1: max |diff| {diff.max():.3e}")
                assert diff.max() <= 1e-12
            else:
                print(f"scipy {mode} {g} order 0: left out {100 * (1 - safe.mean()):.3f} %, differing safe voxels {int((diff[..., safe] > 0).sum())}")
                assert safe.mean() >= 0.99 and (diff[..., safe] == 0).all()


def test_blur_halo_is_the_output_tile():
    """Far-corner crop: blurring the slice (reflect of the tile) differs from slicing a blurred, larger gather."""
    rng = np.random.default_rng(1)
    item = rng.random((1,) + ITEM).astype(np.float32)
    d, h, w = ITEM
    rec = A.record_vol_crop(0, (h, w), origin=(w - TILE[2], h - TILE[1]), blur_k=7)
    got, _ = CO.apply(item, rec, d - TILE[0], TILE, CO.IMAGE, CO.REFLECT, 0.0, 1, 2, 3)
    sl = item[:, d - TILE[0]:, h - TILE[1]:, w - TILE[2]:].astype(np.float64)
    assert np.allclose(got, CO.VO.box_blur_reflect(sl, 7), atol=1e-15)
    wider = CO.VO.box_blur_reflect(item.astype(np.float64), 7)[:, d - TILE[0]:, h - TILE[1]:, w - TILE[2]:]
    assert np.abs(got - wider)[..., :8, :8].max() > 1e-3          # the near edge of the far-corner crop: tile reflection vs. real neighbours


def test_vol_crop_matrix_equals_the_oracle_coordinates():
    d, h, w = ITEM
    ys, xs = np.mgrid[0:TILE[1], 0:TILE[2]].astype(np.float64)
    for i, g in enumerate(GEOMETRY):
        for ox, oy in ((0, 0), (w - TILE[2], h - TILE[1]), (17, 11)):
            rec = _rec(i, (h, w), g, origin=(ox, oy))
            m = A.vol_crop_matrix(float(rec["angle"]), float(rec["scale"]), (ox, oy), (h, w))
            assert np.array_equal(m, rec["m"])
            sx, sy = CO.plane_coords(rec, h, w)
            ex = np.abs(m[0] * xs + m[1] * ys + m[2] - sx[oy:oy + TILE[1], ox:ox + TILE[2]]).max()
            ey = np.abs(m[3] * xs + m[4] * ys + m[5] - sy[oy:oy + TILE[1], ox:ox + TILE[2]]).max()
            print(f"matrix {g} origin {(ox, oy)}: max coordinate difference {max(ex, ey):.3e}")
            assert max(ex, ey) <= 1e-9
    assert np.array_equal(A.vol_crop_matrix(0, 1, (17, 11), (h, w)), [1, 0, 17, 0, 1, 11])                      # whole-pixel crop: exact
    assert np.array_equal(A.vol_crop_matrix(33, 0.7, (0, 0), (h, w)), A.inverse_matrix(0, 33, 0.7, 0, 0, h, w))  # origin 0: draw's map
    assert A.SOURCE_VOL_DTYPE.itemsize == 24
    with pytest.raises(ValueError):
        A.vol_crop_matrix(0, 0, (0, 0), (h, w))
    with pytest.raises(ValueError):
        A.record_vol_crop(0, (h, w), blur_k=4)


SIZES = [(3, 20, 24), (7, 70, 90), (6, 64, 64)]


def _store(tmp_path, dim_out=(2, 16, 16), aug_factor=3, **attrs):
    return VolumeStore.create(str(tmp_path / "s"), SIZES, {"volume": 1, "mask": 1, "orientation": 2},
                              {"dim_out": dim_out, "aug_factor": aug_factor, "nan_to_val": -1.0, "clip_threshold": (0.0, 99.99), **attrs},
                              dtypes={"volume": "u8", "mask": "f32", "orientation": "f32"}, squeeze={"volume": True, "mask": True, "orientation": True})


def test_volume_store(tmp_path):
    st = _store(tmp_path, scale_limit=(-0.5, 0))
    assert isinstance(st, ImageStore) and st.recipe == "mo3d"
    assert len(st) == 9 and st.n_items == 3 and st.aug_factor == 3 and st.nan_to_val == -1.0 and st.dim_out == (2, 16, 16)
    assert st.locate(0) == 0 and st.locate(8) == 2 and st.locate([0, 2, 3, 5, 6]).tolist() == [0, 0, 1, 1, 2]
    with pytest.raises(IndexError):
        st.locate(9)
    assert st.fields == {"volume": (2, 16, 16), "mask": (2, 16, 16), "orientation": (2, 2, 16, 16)}       # two channels are never squeezed
    assert st.offsets["mask"].tolist() == [0, 3 * 20 * 24, 3 * 20 * 24 + 7 * 70 * 90] and st.offsets["orientation"][1] == 2 * 3 * 20 * 24
    rng = np.random.default_rng(0)
    mask = rng.random(SIZES[1]).astype(np.float32)
    mask[2, 5:9, 7:30] = np.nan
    mask[0, 0, 0] = np.float32(np.frombuffer(np.uint32(0x7FC01234).tobytes(), dtype=np.float32)[0])      # a NaN with a payload
    st.put(1, "mask", mask)
    vol = rng.integers(0, 256, SIZES[1], dtype=np.uint8)
    st.put(1, "volume", vol)
    st.put(2, "volume", np.full(SIZES[2], 0.5))
    st.flush()
    back = VolumeStore(str(tmp_path / "s"))
    assert back.item(1, "mask").shape == (1,) + SIZES[1] and back.item(1, "mask").tobytes() == mask.tobytes()      # NaN bit for bit
    assert np.array_equal(back.item(1, "volume")[0], vol) and (back.item(2, "volume") == 128).all()
    assert back.scale_limit == [-0.5, 0] and back.clip_threshold == [0.0, 99.99]
    with pytest.raises(ValueError, match="non-finite"):
        st.put(0, "volume", np.full(SIZES[0], np.nan, dtype=np.float32))
    with pytest.raises(ValueError, match="expected"):
        st.put(0, "mask", np.zeros((3, 20, 25), dtype=np.float32))
    with pytest.raises(RuntimeError, match="device only"):
        st[0]
    with pytest.raises(RuntimeError, match="GPU"):
        st.to_device("cpu")
    ImageStore.create(str(tmp_path / "i"), [(8, 8)], {"image": 1}, {"dim_out": (4, 4)})
    with pytest.raises(ValueError, match="not a volume store"):
        VolumeStore(str(tmp_path / "i"))
    with pytest.raises(ValueError, match="not an image store"):
        ImageStore(str(tmp_path / "s"))


def test_volume_store_refusals(tmp_path):
    mk = lambda sizes, attrs, fields=None: VolumeStore.create(str(tmp_path / "r"), sizes, fields or {"volume": 1}, attrs)
    with pytest.raises(ValueError, match="item 1.*smaller than dim_out"):
        mk([(4, 32, 32), (3, 32, 32)], {"dim_out": (4, 16, 16)})
    with pytest.raises(ValueError, match="item 0.*smaller than dim_out"):
        mk([(4, 32, 15)], {"dim_out": (4, 16, 16)})
    with pytest.raises(ValueError, match="2\\^31"):
        mk([(1 << 9, 1 << 11, 1 << 11)], {"dim_out": (4, 16, 16)})
    with pytest.raises(ValueError, match="2\\^31"):
        mk([(1 << 9, 1 << 10, 1 << 11)], {"dim_out": (4, 16, 16)}, {"volume": 1, "orientation": 2})
    with pytest.raises(ValueError, match="dim_out"):
        mk([(4, 32, 32)], {"dim_out": (16, 16)})
    with pytest.raises(ValueError, match="dim_out"):
        mk([(4, 32, 32)], {})
    with pytest.raises(ValueError, match="aug_factor"):
        mk([(4, 32, 32)], {"dim_out": (4, 16, 16), "aug_factor": 0})
    with pytest.raises(ValueError, match="aug_factor"):
        mk([(4, 32, 32)], {"dim_out": (4, 16, 16), "aug_factor": 2.5})
    with pytest.raises(ValueError, match="positive extent"):
        mk([(4, 32)], {"dim_out": (4, 16, 16)})
    with pytest.raises(ValueError, match="positive extent"):
        mk([], {"dim_out": (4, 16, 16)})


LOGICAL = ("flags", "rot_k", "blur_k", "index", "cos_t", "sin_t", "alpha", "beta", "shot_s", "gauss_sigma", "angle", "scale")


def test_draw_crops(tmp_path):
    st = _store(tmp_path, dim_out=(2, 16, 20), aug_factor=1500)
    aug = A.AugmenterVol.from_store(st, seed=11)
    assert aug.n_uniform == 13 and aug.n_uniform_crop == 16
    idx = np.arange(len(st))
    recs, sources = aug.draw_crops(4, idx, st)
    again, sources2 = A.AugmenterVol.from_store(st, seed=11).draw_crops(4, idx[::-1].copy(), st)
    assert recs.tobytes() == again[::-1].tobytes() and all(sources[k].tobytes() == sources2[k][::-1].tobytes() for k in sources)     # pure
    one, src1 = aug.draw_crops(4, [1234], st)
    assert one[0].tobytes() == recs[1234].tobytes() and src1["mask"][0] == sources["mask"][1234]
    assert aug.draw_crops(5, idx, st)[0].tobytes() != recs.tobytes()
    assert A.AugmenterVol.from_store(st, seed=12).draw_crops(4, idx, st)[0].tobytes() != recs.tobytes()
    items = st.locate(idx)
    for i, (d, h, w) in enumerate(SIZES):
        sel = items == i
        plain = aug.draw(4, idx[sel], shape=(h, w))
        for f in LOGICAL:
            assert np.array_equal(plain[f], recs[f][sel]), f                        # the same gates and values as draw's record
        assert (plain["dx"] == 0).all() and (plain["dy"] == 0).all()
        src = sources["orientation"][sel]
        assert (src["d"] == d).all() and (src["h"] == h).all() and (src["w"] == w).all()
        assert (src["offset"] == st.offsets["orientation"][i]).all() and (sources["mask"][sel]["offset"] == st.offsets["mask"][i]).all()
        for name, v, e, t in (("z0", src["z0"], d, 2), ("oy", recs["dy"][sel], h, 16), ("ox", recs["dx"][sel], w, 20)):
            print(f"draw_crops item {i} {name}: {int(v.min())} .. {int(v.max())} of 0 .. {e - t}, {sel.sum()} draws")
            assert v.min() == 0 and v.max() == e - t and (v == np.floor(v)).all()   # always inside, and both ends occur
        # the record's map is the crop of the whole-plane map
        for j in np.flatnonzero(sel)[:20]:
            r = recs[j]
            assert np.array_equal(r["m"], A.vol_crop_matrix(float(r["angle"]), float(r["scale"]), (r["dx"], r["dy"]), (h, w)))
    assert all((sources[k]["z0"] == sources["mask"]["z0"]).all() for k in sources)     # every field of a patch shares the placement
    assert aug.draw(4, idx[:50], shape=(20, 24)).tobytes() == A.AugmenterVol.from_store(st, seed=11).draw(4, idx[:50], shape=(20, 24)).tobytes()


def _raw(sizes=SIZES, seed=0):
    rng = np.random.default_rng(seed)
    vols = [rng.integers(0, 4096, s).astype(np.uint16) for s in sizes]
    masks = [rng.random(s) > 0.5 for s in sizes]
    return vols, masks


def test_prepare_mo3d_refusals_need_no_device(tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(dataprep, "_device", no_device)
    vols, masks = _raw()
    path, kw = str(tmp_path / "p"), dict(dim_out=(2, 16, 16))
    from bio_image_unet_amd.multi_output_unet3d import prepare
    assert prepare is dataprep.prepare_mo3d
    with pytest.raises(ValueError, match="2 items for 3 volumes"):
        prepare(vols, {"mask": masks[:2]}, path, **kw)
    with pytest.raises(ValueError, match="Shape mismatch: mask has shape"):
        prepare(vols, {"mask": [masks[0], masks[1][:, :-1], masks[2]]}, path, **kw)
    with pytest.raises(ValueError, match="Shape mismatch: orientation"):
        prepare(vols, {"orientation": [np.zeros((2,) + s) for s in SIZES]}, path, **kw)
    with pytest.raises(ValueError, match='named "volume"'):
        prepare(vols, {"volume": masks}, path, **kw)
    with pytest.raises(ValueError, match="nan_to_val"):
        prepare(vols, {"mask": masks}, path, nan_to_val=float("nan"), **kw)
    with pytest.raises(ValueError, match="aug_factor"):
        prepare(vols, {"mask": masks}, path, aug_factor=0, **kw)
    with pytest.raises(ValueError, match="item 0.*smaller than dim_out"):
        prepare(vols, {"mask": masks}, path, dim_out=(4, 16, 16))
    with pytest.raises(ValueError, match="in_channels"):
        prepare(vols, {"mask": masks}, path, in_channels=2, **kw)
    with pytest.raises(ValueError, match="volume_dtype"):
        prepare(vols, {"mask": masks}, path, volume_dtype="f16", **kw)
    with pytest.raises(ValueError, match="dim_out"):
        prepare(vols, {"mask": masks}, path, dim_out=(16, 16))
    with pytest.raises(ValueError, match="no targets"):
        prepare(vols, {}, path, **kw)
    with pytest.raises(ValueError, match="real dtype"):
        prepare(vols, {"mask": [m.astype(np.complex64) for m in masks]}, path, **kw)
    with pytest.raises(AssertionError, match="a device was asked for"):     # nothing else stands in the way
        prepare(vols, {"mask": masks}, path, **kw)
    import inspect
    sig = inspect.signature(prepare)
    want = dict(dim_out=(128, 128, 128), in_channels=1, nan_to_val=0, clip_threshold=(0., 99.99), aug_factor=10, scale_limit=(-0.75, 0), rotate_limit=(0, 360),
                gauss_noise_lims=(0.01, 0.1), shot_noise_lims=(0.005, 0.01), brightness_contrast=(0.1, 0.1), blur_limit=(3, 7), volume_dtype="f32", device="auto")
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == want


HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0}}


def test_a_volume_store_needs_a_gpu_and_its_own_trainer(tmp_path):
    from bio_image_unet_amd.workflow import TrainerMo2d, TrainerMo3d, _resolve_augment
    st = _store(tmp_path)
    with pytest.raises(ValueError, match="GPU device"):
        TrainerMo3d(st, HEADS, 1, n_filter=8, batch_size=1, save_dir=str(tmp_path / "o"), device="cpu")
    with pytest.raises(ValueError, match="mo3d"):
        TrainerMo2d(st, 1, output_heads=HEADS, n_filter=8, batch_size=1, save_dir=str(tmp_path / "o"), device="cpu")
    for bad in (False, "yes", A.AugmenterF32()):
        with pytest.raises(ValueError, match="AugmenterVol"):
            _resolve_augment(bad, st, torch.device("cuda"), "mo3d")
    own = A.AugmenterVol(seed=3)
    assert _resolve_augment(own, st, torch.device("cuda"), "mo3d") is own
    made = _resolve_augment(None, st, torch.device("cuda"), "mo3d")
    assert isinstance(made, A.AugmenterVol) and made.shape == (2, 16, 16)
    assert isinstance(_resolve_augment(True, st, torch.device("cuda"), "mo3d"), A.AugmenterVol)
    with pytest.raises(RuntimeError, match="GPU"):
        CropFeeder(st, range(4), 2, "cpu", own)
