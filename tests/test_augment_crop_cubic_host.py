"""Cubic-spline targets of whole-image stores, the parts that need no GPU: the oracle (``tests/augment_crop_cubic_oracle.py``) pinned to the
reference's ``rotate_array`` at ``order=3`` restated on scipy, the clip rule, the records, and what the table entry refuses."""
import ctypes as C

import numpy as np
import pytest

from bio_image_unet_amd import augment as A
from bio_image_unet_amd import feed
from tests import augment_crop_cubic_oracle as XO
from tests import augment_crop_oracle as CO

ITEMS = [(70, 90), (64, 64), (50, 130)]
ANGLES = [17.3, 151.0, 203.7, 331.9]                 # none a multiple of 45 degrees
ids = lambda s: "x".join(map(str, s))


def _nan_holes(x, rng):
    """``tests/test_gpu_augment_crop.py``'s pattern: a blob, isolated pixels, and a full row and column at the wrap seam."""
    h, w = x.shape[-2:]
    yy, xx = np.mgrid[:h, :w]
    x[..., (yy - h // 3) ** 2 + (xx - w // 2) ** 2 < 64] = np.nan
    x[..., rng.integers(0, h, 30), rng.integers(0, w, 30)] = np.nan
    x[..., h - 1, :] = np.nan
    x[..., :, 0] = np.nan
    return x


def test_symbols_are_bound_and_the_table_row_has_its_size():
    import bio_image_unet_amd._lib as L
    for name, args in (("biu_spline_prefilter_items", 10), ("biu_augment_f32_crop_cubic", 17)):
        assert hasattr(L.lib._c, name) and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == args
    assert C.sizeof(L.biu_spline_item) == feed.SPLINE_ITEM_DTYPE.itemsize == 16
    for name, _ in L.biu_spline_item._fields_:
        assert feed.SPLINE_ITEM_DTYPE.fields[name][1] == getattr(L.biu_spline_item, name).offset, name
    hdr = open(L.os.path.join(L.os.path.dirname(L._HERE), "include", "biu.h")).read()
    assert "int biu_spline_prefilter_items(" in hdr and "int biu_augment_f32_crop_cubic(" in hdr and "} biu_spline_item;" in hdr


@pytest.mark.parametrize("hw", ITEMS, ids=ids)
def test_oracle_equals_the_references_rotate_array_at_order_3(hw):
    """On the item's own extent: the NaN decisions equal wherever ``|w_nan - 0.5| > 1e-6`` with NO pixel left out, values within 1e-12."""
    rng = np.random.default_rng(hw[0] * hw[1])
    x = _nan_holes(rng.random(hw).astype(np.float32), rng)
    for i, angle in enumerate(ANGLES):
        rec = A.record_crop(i, hw, angle=angle)
        angle = float(rec["angle"])                                                   # the fp32 number the record keeps
        got, safe, w_nan = XO.apply(x[None], rec, hw, -7.0)
        want = XO.reference_rotate_array(x.astype(np.float64), angle)
        got, safe, w_nan = got[0], safe[0], w_nan[0]
        nan_got, nan_want = got == -7.0, np.isnan(want)
        both = ~nan_got & ~nan_want
        print(f"order 3 {hw} angle {angle}: left out {int((~safe).sum())} pixels, nearest |w_nan - 0.5| {np.abs(w_nan - 0.5).min():.3e}, NaN share "
              f"{100 * nan_want.mean():.2f} %, decisions differing {int((nan_got != nan_want).sum())}, max |diff| {np.abs(got - want)[both].max():.3e}, "
              f"clipped {int(((got == np.nanmin(x)) | (got == np.nanmax(x))).sum())}")
        assert safe.all()
        assert nan_want.any() and not nan_want.all() and np.array_equal(nan_got, nan_want)
        assert np.abs(got - want)[both].max() <= 1e-12


def test_clip_rule():
    """Applied iff ``nanmin >= 0`` and ``nanmax <= 1``: a 0 / 1 mask is clipped (the spline overshoots), a distance-like target in [0, 5]
    is not, a target with a negative value is not; an item of nothing but NaN renders ``nan_to_val`` everywhere."""
    hw = (64, 64)
    rng = np.random.default_rng(2)
    rec = A.record_crop(0, hw, angle=30.0)
    mask = _nan_holes((rng.random(hw) > 0.5).astype(np.float32), rng)
    got, _, _ = XO.apply(mask[None], rec, hw, -1.0)
    free = XO.QO.gather_cubic(XO.coefficients(mask[None])[0], *CO.source_coords(hw, hw, *CO.geometry_of(rec)))
    shown = got[got != -1.0]
    print(f"clip: 0/1 mask, unclipped spline in [{free.min():.3f}, {free.max():.3f}], rendered in [{shown.min():.3f}, {shown.max():.3f}], "
          f"at the bounds {int(((shown == 0) | (shown == 1)).sum())} of {shown.size}")
    assert free.min() < -0.05 and free.max() > 1.05 and shown.min() == 0.0 and shown.max() == 1.0
    assert np.abs(got[0] - np.nan_to_num(XO.reference_rotate_array(mask.astype(np.float64), float(rec["angle"])), nan=-1.0)).max() <= 1e-12
    distance = _nan_holes((5.0 * (rng.random(hw) > 0.5)).astype(np.float32), rng)           # steps of 5: the spline leaves [0, 5]
    got, _, _ = XO.apply(distance[None], rec, hw, -1.0)
    shown = got[got != -1.0]
    print(f"clip: distance target in [0, 5] rendered in [{shown.min():.3f}, {shown.max():.3f}]")
    assert shown.min() < 0.0 and shown.max() > 5.0 and XO.item_range(distance[None]) == (0.0, 5.0)
    assert np.abs(got[0] - np.nan_to_num(XO.reference_rotate_array(distance.astype(np.float64), float(rec["angle"])), nan=-1.0)).max() <= 1e-12
    signed = (rng.random(hw).astype(np.float32) - 0.25)
    got, _, _ = XO.apply(signed[None], rec, hw, -1.0)
    assert got.min() < signed.min() or got.max() > signed.max()                             # nothing holds it back
    # the range is over ALL planes of the item: a second plane that reaches 2 switches the clip off for the first
    got, _, _ = XO.apply(np.stack([np.nan_to_num(mask), 2 * np.nan_to_num(mask)]), rec, hw, -1.0)
    assert got[0].min() < 0.0 and got[0].max() > 1.0
    empty = np.full((1,) + hw, np.nan, dtype=np.float32)
    for dtype in (np.float64, np.float32):
        got, safe, w_nan = XO.apply(empty, rec, hw, -3.0, dtype=dtype)
        assert (got == -3.0).all() and safe.all() and np.abs(w_nan - 1.0).max() < 1e-5
    assert XO.item_range(empty) == (np.inf, -np.inf)


def _store(tmp_path):
    st = feed.ImageStore.create(str(tmp_path / "s"), ITEMS, {"image": 1, "mask": 1}, {"dim_out": [64, 64], "scale_limit": [-0.2, 0.3]})
    rng = np.random.default_rng(0)
    for i, hw in enumerate(ITEMS):
        st.put(i, "image", rng.random(hw).astype(np.float32))
        st.put(i, "mask", _nan_holes(rng.random(hw).astype(np.float32), rng))
    st.flush()
    return st


def test_records_do_not_depend_on_the_interpolation(tmp_path):
    st = _store(tmp_path)
    lin, cub = A.AugmenterF32.from_store(st, seed=5), A.AugmenterF32.from_store(st, seed=5, target_interp="cubic")
    idx = np.arange(len(st))
    for epoch in (0, 3, A.VALIDATION_EPOCH):
        ra, sa = lin.draw_crops(epoch, idx, st)
        rb, sb = cub.draw_crops(epoch, idx, st)
        assert ra.tobytes() == rb.tobytes() and all(sa[k].tobytes() == sb[k].tobytes() for k in sa)
    assert (ra["flags"] & A.ROT_F).any() and cub.spline_fields(st) == ["mask"] and cub.rot_flag == A.ROT_F
    assert cub.describe()["target_interp"] == "cubic"


def test_the_table_entry_refuses_a_cpu_device(tmp_path):
    st = _store(tmp_path)
    with pytest.raises(RuntimeError, match="GPU"):
        st.spline_tables("cpu", ["mask"])
    with pytest.raises(RuntimeError, match="GPU"):
        st.spline_tables("cpu", [])                                                   # before it looks at the names
    import torch
    with pytest.raises(ValueError, match="device tensor"):
        feed.SplineTables.build(torch.zeros(16), 1, [0], [(4, 4)])
