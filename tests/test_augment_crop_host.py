"""Whole-image stores and crop augmentation, the parts that need no GPU: the oracle's geometry and NaN rule pinned to scipy, ``crop_matrix``,
the patch count, ``draw_crops``' purity, the ``ImageStore`` round trip and ``prepare``'s argument errors."""
import ctypes as C

import numpy as np
import pytest

from bio_image_unet_amd import augment as A
from bio_image_unet_amd import feed
from tests import augment_crop_oracle as CO
from tests import augment_f32_oracle as FO

ITEMS = [(70, 90), (64, 64), (50, 130)]              # the last is narrower than the tile in one axis: the crop wraps
TILE = (64, 64)
ANGLES = [17.3, 151.0, 203.7, 331.9]                 # none a multiple of 45 degrees
ORIGIN = {(70, 90): (13, 5), (64, 64): (0, 0), (50, 130): (41, 0)}        # (ox, oy)


def test_symbols_are_bound_and_records_have_their_sizes():
    import bio_image_unet_amd._lib as L
    assert hasattr(L.lib._c, "biu_augment_f32_crop") and "biu_augment_f32_crop" in L.SIGNATURES
    assert len(L.SIGNATURES["biu_augment_f32_crop"][1]) == 17
    assert C.sizeof(L.biu_augf_source) == A.SOURCE_DTYPE.itemsize == 16
    assert C.sizeof(L.biu_augf_params) == A.PARAMS_F32_DTYPE.itemsize == 104          # the record is unchanged
    hdr = open(L.os.path.join(L.os.path.dirname(L._HERE), "include", "biu.h")).read()
    assert "int biu_augment_f32_crop(" in hdr and "} biu_augf_source;" in hdr


def _wrapped_crop(r, ox, oy, th, tw):
    h, w = r.shape[-2:]
    return r[..., np.mod(oy + np.arange(th), h)[:, None], np.mod(ox + np.arange(tw), w)[None, :]]


@pytest.mark.parametrize("hw", ITEMS, ids=lambda s: "x".join(map(str, s)))
def test_geometry_equals_scipy_rotate_and_crop(hw):
    """scale = 1: the oracle's tile is the crop ``[oy:oy+th, ox:ox+tw]`` of ``scipy.ndimage.rotate(item, angle, reshape=False,
    mode='grid-wrap')``: exact off rounding ties at order 0, to 1e-12 at order 1.  Where the item is smaller than the tile (50 x 130) the
    slice ends with the item, as numpy's does: rows 50 .. 63 of the tile are the padding.  There ONE affine map and ONE wrap continue the
    rotated periodic plane, where the reference wrap-pads the rotated array ("Whole-image stores": the departure; without a
    rotation the two are the same pixels, ``test_quarter_turns_equal_rot90_of_non_square_items``); the padding only has to be finite
    values of the item."""
    from scipy.ndimage import rotate
    h, w = hw
    ox, oy = ORIGIN[hw]
    item = np.random.default_rng(h * w).random((1, h, w)).astype(np.float32)
    for i, angle in enumerate(ANGLES):
        rec = A.record_crop(i, hw, angle=angle, origin=(ox, oy))
        angle = float(rec["angle"])                                                   # the fp32 number the record keeps
        assert float(rec["dx"]) == ox and float(rec["dy"]) == oy                      # the stored dx, dy document the origin
        got, safe = CO.apply(item, rec, CO.IMAGE, TILE, 0.0, 1, 0, 1)
        want = rotate(item[0].astype(np.float64), angle, reshape=False, mode="grid-wrap", order=0)[oy:oy + TILE[0], ox:ox + TILE[1]]
        ih, iw = want.shape                                                           # (64, 64), or (50, 64) of the 50 x 130 item
        assert (ih, iw) == (min(h - oy, TILE[0]), TILE[1])
        safe_in = safe[:ih, :iw]
        print(f"{hw} angle {angle}: order 0 left out {100 * (1 - safe.mean()):.3f} %, differing safe pixels {int((got[0, :ih, :iw] != want)[safe_in].sum())}")
        assert safe.mean() >= 0.99 and np.array_equal(got[0, :ih, :iw][safe_in], want[safe_in])
        assert np.isin(got[0, ih:], item[0].astype(np.float64)).all()                # the padding: pixels of the item
        got, _ = CO.apply(item, rec, CO.MASK, TILE, 0.0, 1, 0, 1)
        want = rotate(item[0].astype(np.float64), angle, reshape=False, mode="grid-wrap", order=1)[oy:oy + TILE[0], ox:ox + TILE[1]]
        print(f"{hw} angle {angle}: order 1 max |diff| {np.abs(got[0, :ih, :iw] - want).max():.3e}")
        assert np.abs(got[0, :ih, :iw] - want).max() <= 1e-12
        # the matrix the kernel consumes describes the same coordinates as the oracle's chain
        sx, sy = CO.source_coords(hw, TILE, *CO.geometry_of(rec))
        y, x = np.meshgrid(np.arange(TILE[0], dtype=np.float64), np.arange(TILE[1], dtype=np.float64), indexing="ij")
        m = rec["m"]
        assert np.abs(m[0] * x + m[1] * y + m[2] - sx).max() < 1e-9 and np.abs(m[3] * x + m[4] * y + m[5] - sy).max() < 1e-9


@pytest.mark.parametrize("hw", [(70, 90), (50, 130)], ids=lambda s: "x".join(map(str, s)))
def test_quarter_turns_equal_rot90_of_non_square_items(hw):
    h, w = hw
    rng = np.random.default_rng(3)
    item = rng.random((2, h, w)).astype(np.float32)
    for k in range(4):
        turned = np.rot90(item, k, axes=(1, 2))
        ox, oy = (7, 3) if min(turned.shape[1:]) >= 64 else (11, 0)
        rec = A.record_crop(k, hw, rot_k=k, origin=(ox, oy))
        want = _wrapped_crop(turned, ox, oy, *TILE)
        for kind in (CO.IMAGE, CO.MASK):
            got, safe = CO.apply(item, rec, kind, TILE, 0.0, 1, 0, 1)
            assert safe.all() and np.array_equal(got, want.astype(np.float64))
        got, _ = CO.apply(item, rec, CO.VECTOR, TILE, 0.0, 1, 0, 1)
        c, s = want[0].astype(np.float64), want[1].astype(np.float64)
        wc, ws = [(c, s), (s, -c), (-c, -s), (-s, c)][k]
        assert np.array_equal(got[0], wc) and np.array_equal(got[1], ws)
        # whole-pixel cases of the matrix are exact integers
        m = A.crop_matrix(k, 0.0, 1.0, (ox, oy), hw, TILE)
        assert np.array_equal(m, np.rint(m)) and m.tobytes() == rec["m"].tobytes() and not (np.signbit(m) & (m == 0)).any()
        sx, sy = CO.source_coords(hw, TILE, k, 0.0, 1.0, ox, oy)
        y, x = np.meshgrid(np.arange(64.0), np.arange(64.0), indexing="ij")
        assert np.array_equal(m[0] * x + m[1] * y + m[2], sx) and np.array_equal(m[3] * x + m[4] * y + m[5], sy)


def _nan_item(hw, seed):
    """Values in [0, 1) with a NaN blob, isolated NaN pixels, and a full row and column that cross the wrap seam."""
    h, w = hw
    rng = np.random.default_rng(seed)
    x = rng.random((h, w)).astype(np.float32)
    yy, xx = np.mgrid[:h, :w]
    x[(yy - h // 3) ** 2 + (xx - w // 2) ** 2 < 81] = np.nan
    x[rng.integers(0, h, 40), rng.integers(0, w, 40)] = np.nan
    x[h - 1, :] = np.nan
    x[:, 0] = np.nan
    return x


@pytest.mark.parametrize("hw", ITEMS, ids=lambda s: "x".join(map(str, s)))
def test_nan_rule_equals_the_references_rotate_array(hw):
    """The oracle's bilinear NaN rule against the restated ``rotate_array(x, angle, order=1)`` on every pixel with ``|w_nan - 0.5| > 1e-6``;
    at most 1 % of the pixels may be left out (a condition on these inputs)."""
    x = _nan_item(hw, 11)
    for i, angle in enumerate(ANGLES):
        rec = A.record_crop(i, hw, angle=angle)
        angle = float(rec["angle"])
        got, safe = CO.apply(x[None], rec, CO.MASK, hw, -7.0, 1, 0, 1)
        want = CO.rotate_array_restated(x.astype(np.float64), angle, order=1)
        got, safe = got[0], safe[0]
        left_out = 1.0 - safe.mean()
        nan_got, nan_want = got == -7.0, np.isnan(want)
        both = safe & ~nan_want & ~nan_got
        print(f"NaN rule {hw} angle {angle}: left out {100 * left_out:.4f} %, NaN share {100 * nan_want.mean():.2f} %, "
              f"decisions differing on safe pixels {int((nan_got != nan_want)[safe].sum())}, max |diff| {np.abs(got - want)[both].max():.3e}")
        assert left_out <= 0.01
        assert nan_want.any() and np.array_equal(nan_got[safe], nan_want[safe])
        assert np.abs(got - want)[both].max() <= 1e-12


def test_nearest_and_vector_nan_rules_of_the_oracle():
    x = _nan_item((64, 64), 5)
    rec = A.record_crop(0, (64, 64), rot_k=1)
    got, _ = CO.apply(x[None], rec, CO.MASK, TILE, -1.0, 1, 0, 1)
    want = np.rot90(x, 1)
    assert np.array_equal(got[0], np.where(np.isnan(want), -1.0, want.astype(np.float64))) and not np.isnan(got).any()
    pair = np.stack([x, np.roll(_nan_item((64, 64), 6), 5, axis=1)])
    got, _ = CO.apply(pair, rec, CO.VECTOR, TILE, -1.0, 1, 0, 1)
    gone = np.isnan(np.rot90(pair[0], 1)) | np.isnan(np.rot90(pair[1], 1))
    assert (got[0][gone] == -1.0).all() and (got[1][gone] == -1.0).all() and not np.isnan(got).any()
    assert np.array_equal(got[0][~gone], np.rot90(pair[1], 1).astype(np.float64)[~gone])          # k = 1: (s, -c)
    assert np.array_equal(got[1][~gone], -np.rot90(pair[0], 1).astype(np.float64)[~gone])


# ---- records and counts ------------------------------------------------------------------------------------------------------------------
def test_crop_matrix_whole_pixel_cases_are_exact():
    assert np.array_equal(A.crop_matrix(0, 0, 1, (0, 0), (70, 90), TILE), [1, 0, 0, 0, 1, 0])
    assert np.array_equal(A.crop_matrix(0, 0, 1, (13, 5), (70, 90), TILE), [1, 0, 13, 0, 1, 5])
    assert np.array_equal(A.crop_matrix(1, 0, 1, (2, 3), (70, 90), TILE), [0, -1, 90 - 1 - 3, 1, 0, 2])
    assert np.array_equal(A.crop_matrix(2, 0, 1, (2, 3), (70, 90), TILE), [-1, 0, 90 - 1 - 2, 0, -1, 70 - 1 - 3])
    assert np.array_equal(A.crop_matrix(3, 0, 1, (2, 3), (70, 90), TILE), [0, 1, 3, -1, 0, 70 - 1 - 2])
    assert np.array_equal(A.crop_matrix(0, 0, 2, (4, 6), (70, 90), TILE), [0.5, 0, 1.75, 0, 0.5, 2.75])     # (X + 0.5) / 2 - 0.5
    with pytest.raises(ValueError):
        A.crop_matrix(0, 0, 0, (0, 0), (70, 90), TILE)


def _store(tmp_path, sizes=((70, 90), (64, 64), (50, 130)), aug_factor=2, name="s", fill=True, **attrs):
    st = feed.ImageStore.create(str(tmp_path / name), sizes, {"image": 1, "mask": 1, "orientation": 2},
                                {"dim_out": list(TILE), "aug_factor": aug_factor, "nan_to_val": 0.0, **attrs},
                                dtypes={"image": "u8", "mask": "f32", "orientation": "f32"}, squeeze={"image": True, "mask": True})
    if fill:
        rng = np.random.default_rng(0)
        for i, (h, w) in enumerate(sizes):
            st.put(i, "image", rng.integers(0, 256, (h, w), dtype=np.uint8))
            st.put(i, "mask", _nan_item((h, w), i))
            phi = _nan_item((h, w), 10 + i) * 6.28
            st.put(i, "orientation", np.stack([np.cos(phi), np.sin(phi)]))
        st.flush()
    return st


def test_patch_count_is_the_references_and_locate_inverts_it(tmp_path):
    sizes = [(70, 90), (64, 64), (50, 130), (20, 20), (300, 200)]
    for aug_factor in (2, 0.5, 3.7):
        st = _store(tmp_path, sizes, aug_factor, name=f"c{aug_factor}", fill=False)
        want = [max(int((h * w) / (64 * 64) * aug_factor), 2) for h, w in sizes]
        assert list(st.counts) == want and len(st) == sum(want)
        assert min(want) == 2 and st.counts[3] == 2                                  # the floor of 2
        items = st.locate(np.arange(len(st)))
        assert np.array_equal(items, np.repeat(np.arange(len(sizes)), want))
        assert st.locate(0) == 0 and st.locate(len(st) - 1) == len(sizes) - 1 and st.locate(want[0]) == 1
        with pytest.raises(IndexError):
            st.locate(len(st))


def test_draw_crops_is_a_pure_function_of_seed_epoch_and_patch_index(tmp_path):
    st = _store(tmp_path, fill=False, scale_limit=[-0.3, 0.4])
    mk = lambda seed=9: A.AugmenterF32.from_store(st, seed=seed)
    assert mk().scale_limit == (-0.3, 0.4) and mk().shape == TILE
    idx = np.arange(len(st))
    recs, srcs = mk().draw_crops(4, idx, st)
    perm = np.random.default_rng(1).permutation(len(st))
    again, srcs_p = mk().draw_crops(4, perm, st)
    assert recs.tobytes() == again[np.argsort(perm)].tobytes()                        # order and batch composition do not matter
    one, _ = mk().draw_crops(4, [int(idx[7])], st)
    assert one.tobytes() == recs[7:8].tobytes()
    assert mk().draw_crops(5, idx, st)[0].tobytes() != recs.tobytes() and mk(10).draw_crops(4, idx, st)[0].tobytes() != recs.tobytes()
    assert np.array_equal(recs["index"], idx)
    items = st.locate(idx)
    for name in st.fields:
        assert np.array_equal(srcs[name]["offset"], st.offsets[name][items]) and np.array_equal(srcs[name]["h"], st.sizes[items, 0])
        assert np.array_equal(srcs_p[name]["w"], st.sizes[st.locate(perm), 1])
    assert srcs["orientation"]["offset"][-1] == 2 * (70 * 90 + 64 * 64)
    # quarter turns from {0, 1, 2, 3} whatever the item's shape; the crop lies inside the turned, scaled item or starts at 0 where it is smaller
    many = np.concatenate([mk().draw_crops(e, idx, st)[0] for e in range(40)])
    it = np.tile(items, 40)
    assert set(many["rot_k"][it == 0]) == {0, 1, 2, 3} and set(many["rot_k"][it == 2]) == {0, 1, 2, 3}
    for r, i in zip(many, it):
        h, w = st.sizes[i]
        ht, wt = (w, h) if r["rot_k"] % 2 else (h, w)
        hs, ws = int(round(ht * float(r["scale"]))), int(round(wt * float(r["scale"])))
        assert 0 <= r["dx"] <= max(ws - 64, 0) and 0 <= r["dy"] <= max(hs - 64, 0)
        assert bool(r["flags"] & A.ROT_F) or r["angle"] == 0
        assert np.array_equal(r["m"], A.crop_matrix(r["rot_k"], r["angle"], r["scale"], (r["dx"], r["dy"]), (h, w), TILE))
    assert (many["dx"][it == 0] > 0).any() and (many["flags"] & A.SCALE_F == 0).any()   # u[5], u[6] place the crop, scale gate open or not
    assert ((many["flags"] & A.SCALE_F == 0) & (many["dx"] > 0)).any()


def test_existing_draw_keeps_its_bits():
    """``draw`` goes through the record stream ``draw_crops`` shares: its bytes equal a draw with the packer called directly on the same
    uniforms, sample by sample."""
    aug = A.AugmenterF32(seed=21, scale_limit=(-0.2, 0.3), shape=(48, 80))
    idx = [5, 0, 17, 2 ** 33 + 1]
    recs = aug.draw(3, idx)
    assert recs.tobytes() == aug.draw(3, idx).tobytes() and recs.tobytes() == aug.draw(3, idx, shape=(1, 48, 80)).tobytes()
    pack = aug._packer(48, 80)
    for j, i in enumerate(idx):
        g = np.random.Generator(np.random.Philox(key=[21, 3], counter=[0, i, 0, 0]))
        buf = bytearray(A.PARAMS_F32_DTYPE.itemsize)
        pack(buf, 0, i & 0xFFFFFFFF, g.random(16).tolist())
        assert bytes(buf) == recs[j:j + 1].tobytes()
    u8 = A.Augmenter("unet", seed=2, shape=(32, 32))
    assert u8.draw(1, [4, 9]).tobytes() == u8.draw(1, [9, 4])[::-1].tobytes()


# ---- the store ------------------------------------------------------------------------------------------------------------------------------
def test_image_store_round_trip_keeps_nan_bit_for_bit(tmp_path):
    st = _store(tmp_path)
    odd = np.array([0x7FC00001, 0xFFC12345, 0x7F800001], dtype=np.uint32).view(np.float32)       # NaNs with payloads
    m = np.array(st.item(1, "mask"))
    m[0, 0, :3] = odd
    st.put(1, "mask", m)
    st.flush()
    back = feed.ImageStore(str(tmp_path / "s"))
    assert back.n_items == 3 and len(back) == len(st) and back.dim_out == TILE and back.aug_factor == 2 and back.nan_to_val == 0.0
    assert back.fields == {"image": TILE, "mask": TILE, "orientation": (2,) + TILE} and back.dtypes["image"] == "u8"
    for i in range(3):
        for name in st.fields:
            assert np.asarray(back.item(i, name)).tobytes() == np.asarray(st.item(i, name)).tobytes()
    assert np.array_equal(np.asarray(back.item(1, "mask"))[0, 0, :3].view(np.uint32), odd.view(np.uint32))
    assert np.isnan(back.item(0, "mask")).any() and back.item(2, "orientation").shape == (2, 50, 130)
    with pytest.raises(RuntimeError, match="device"):
        back[0]
    with pytest.raises(ValueError):
        feed.TileStore(str(tmp_path / "s"))                                          # a magic of its own
    with pytest.raises(RuntimeError):
        back.to_device("cpu")


def test_image_store_refuses_nan_images_and_huge_items(tmp_path):
    st = feed.ImageStore.create(str(tmp_path / "f"), [(8, 8)], {"image": 1, "mask": 1}, {"dim_out": [4, 4]})
    bad = np.zeros((8, 8), dtype=np.float32)
    bad[2, 3] = np.nan
    with pytest.raises(ValueError, match="image"):
        st.put(0, "image", bad)
    st.put(0, "mask", bad)                                                           # a target may
    with pytest.raises(ValueError):
        st.put(0, "mask", np.zeros((9, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="2\\^31"):
        feed.ImageStore.create(str(tmp_path / "g"), [(8, 8), (2 ** 15, 2 ** 15)], {"image": 1, "pair": 2}, {"dim_out": [4, 4]})
    with pytest.raises(ValueError, match="2\\^31"):
        feed.ImageStore.create(str(tmp_path / "h"), [(2 ** 16, 2 ** 15 - 1), (1, 2 ** 31 - 4)], {"image": 1}, {"dim_out": [4, 4]})
    with pytest.raises(ValueError):
        feed.ImageStore.create(str(tmp_path / "i"), [(8, 8)], {"image": 1}, {})


def test_prepare_argument_errors_need_no_device(tmp_path):
    from bio_image_unet_amd import multi_output_unet as M
    from bio_image_unet_amd.dataprep import prepare_mo2d
    assert M.prepare is prepare_mo2d
    img = np.zeros((40, 50), dtype=np.uint16)
    p = str(tmp_path / "p")
    with pytest.raises(ValueError, match="Shape mismatch: mask has shape"):
        M.prepare([img], {"mask": [np.zeros((40, 51), dtype=bool)]}, p, dim_out=(32, 32), device="cpu")
    with pytest.raises(ValueError, match="Shape mismatch: orientation"):
        M.prepare([img], {"orientation": [np.zeros((2, 40, 50), dtype=np.float32)]}, p, dim_out=(32, 32), device="cpu")
    with pytest.raises(ValueError, match="in_channels"):
        M.prepare([np.zeros((3, 40, 50))], {"mask": [np.zeros((40, 50))]}, p, dim_out=(32, 32), device="cpu")
    with pytest.raises(ValueError):
        M.prepare([img, img], {"mask": [np.zeros((40, 50))]}, p, dim_out=(32, 32), device="cpu")
    with pytest.raises(ValueError):
        M.prepare([img], {"mask": [np.zeros((40, 50))]}, p, dim_out=(32, 32), image_dtype="f16", device="cpu")
    with pytest.raises(ValueError):
        M.prepare([img], {"mask": [np.zeros((40, 50), dtype=complex)]}, p, dim_out=(32, 32), device="cpu")
    with pytest.raises(RuntimeError):                                                # everything checked: only now is a device asked for
        M.prepare([img], {"mask": [np.zeros((40, 50))]}, p, dim_out=(32, 32), device="cpu")
    with pytest.raises(TypeError):
        M.prepare([img], {"mask": [np.zeros((40, 50))]}, p, add_tile=1)


def test_trainer_resolves_an_image_store(tmp_path):
    from bio_image_unet_amd.workflow import _resolve_augment
    st = _store(tmp_path, fill=False)
    with pytest.raises(ValueError):
        _resolve_augment(None, st, "cpu", "mo2d")                                    # no GPU device
    with pytest.raises(ValueError):
        _resolve_augment(True, st, "cuda", "unet")                                   # another family
    with pytest.raises(ValueError):
        _resolve_augment(False, st, "cuda", "mo2d")                                  # cannot be trained un-augmented
    aug = _resolve_augment(None, st, "cuda", "mo2d")
    assert isinstance(aug, A.AugmenterF32) and aug.shape == TILE
    own = A.AugmenterF32(seed=3)
    assert _resolve_augment(own, st, "cuda", "mo2d") is own
