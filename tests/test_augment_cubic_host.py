"""Cubic-spline resampling of rotated targets, the parts that need no GPU: the float64 oracle (``tests/augment_cubic_oracle.py``) against the
reference's own library calls (``scipy.ndimage.spline_filter`` and ``rotate(order=3, mode='grid-wrap')``), the reference's clip rule, the
truncation the kernel's contract allows, and ``AugmenterF32(target_interp=...)``."""
import ctypes as C  # noqa: F401

import numpy as np
import pytest

import bio_image_unet_amd._lib as L
from bio_image_unet_amd import augment as A
from bio_image_unet_amd.feed import TileStore
from tests import augment_cubic_oracle as CO
from tests import augment_f32_oracle as FO

ANGLES = (17.3, 101.9, 200.2, 333.3)
SHAPES = ((5, 7), (8, 12), (16, 16), (33, 20), (64, 48))
ids = lambda s: "x".join(map(str, s))


def _coords(h, w, r):
    return FO.source_coords(h, w, int(r["rot_k"]), float(r["angle"]), float(r["scale"]), float(r["dx"]), float(r["dy"]))


def test_library_exports_and_binds_the_cubic_path():
    for name in ("biu_spline_prefilter_f32", "biu_augment_f32_cubic"):
        assert hasattr(L.lib._c, name) and name in L.SIGNATURES, name
    hdr = open(L.os.path.join(L.os.path.dirname(L._HERE), "include", "biu.h")).read()
    assert f"#define BIU_SPLINE_R {CO.R}" in hdr
    assert 2 * np.sqrt(3.0) * abs(CO.POLE) ** (CO.R + 1) / (1 - abs(CO.POLE)) < 2.0 ** -26        # the tail the contract drops, per axis


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_oracle_equals_scipy_spline_filter_and_rotate_order_3(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    h, w = shape
    x = np.random.default_rng(1).random((h, w))
    c = CO.prefilter_periodic(x)
    d = np.abs(c - ndi.spline_filter(x, order=3, mode="grid-wrap", output=np.float64)).max()
    print(f"prefilter {shape}: max |diff| from scipy.ndimage.spline_filter {d:.3e}")
    assert d <= 1e-12
    for angle in ANGLES:
        a32 = float(np.float32(angle))                           # the angle a record carries
        sx, sy = _coords(h, w, A.record_f32(0, h, w, angle=angle))
        d = np.abs(CO.gather_cubic(c, sx, sy) - ndi.rotate(x, a32, reshape=False, mode="grid-wrap", order=3)).max()
        print(f"rotate {shape} {angle}: max |diff| from scipy.ndimage.rotate(order=3) {d:.3e}")
        assert d <= 1e-12, angle
    # on a float32 input scipy computes in float64 and rounds once
    x32 = x.astype(np.float32)
    assert np.array_equal(ndi.rotate(x32, 17.3, reshape=False, mode="grid-wrap", order=3),
                          ndi.rotate(x32.astype(np.float64), 17.3, reshape=False, mode="grid-wrap", order=3).astype(np.float32))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_truncated_prefilter_is_within_the_dropped_tail(shape):
    """Cut at ``|j| <= R`` the coefficients of a field in [0, 1) move by at most the dropped tail of the x pass, amplified by the y pass's
    absolute gain of 3, plus the y pass's own tail on x-pass values of at most 3: ``(3 + 3) tail``."""
    x = np.random.default_rng(2).random(shape)
    tail = 2 * np.sqrt(3.0) * abs(CO.POLE) ** (CO.R + 1) / (1 - abs(CO.POLE))
    d = np.abs(CO.prefilter_truncated(x, CO.R) - CO.prefilter_periodic(x)).max()
    print(f"truncation {shape}: R = {CO.R}, max |diff| {d:.3e}, bound {6 * tail:.3e}")
    assert 0 < d <= 6 * tail
    assert np.abs(CO.prefilter_truncated(x, 40) - CO.prefilter_periodic(x)).max() <= 1e-13      # the tail is all that differs


def _fields(shape, seed=3):
    rng = np.random.default_rng(seed)
    return {"[0.02, 0.98]": (0.02 + 0.96 * rng.random((1,) + shape)).astype(np.float32),
            "0/1 mask": (rng.random((1,) + shape) > 0.5).astype(np.float32),
            "[-3, 5]": (-3.0 + 8.0 * rng.random((1,) + shape)).astype(np.float32)}


@pytest.mark.parametrize("shape", SHAPES[2:], ids=ids)
def test_clip_rule_against_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    h, w = shape
    for what, f in _fields(shape).items():
        r = A.record_f32(0, h, w, angle=30.0)
        raw = ndi.rotate(f[0].astype(np.float64), float(r["angle"]), reshape=False, mode="grid-wrap", order=3)
        lo, hi = float(f.min()), float(f.max())
        clips = lo >= 0 and hi <= 1
        want = np.clip(raw, lo, hi) if clips else raw
        got, safe = CO.apply_mask_cubic(f, r)
        d = np.abs(got[0] - want).max()
        print(f"clip {shape} {what}: clip {clips}, unclipped range [{raw.min():.3f}, {raw.max():.3f}], max |diff| {d:.3e}")
        assert d <= 1e-12 and safe.all()
        assert (CO.clip_range(f) is not None) == clips == (what != "[-3, 5]")
        if what == "0/1 mask":
            assert raw.min() < -0.05 and raw.max() > 1.05                      # the clip is what this case is about
            assert got.min() == 0.0 and got.max() == 1.0
    assert CO.clip_range(np.array([True, False])) == (0.0, 1.0)
    assert CO.clip_range(np.array([0.25, np.nan, 0.5])) == (0.25, 0.5)
    # a record without the arbitrary angle takes the nearest gather of the linear path
    f = _fields(shape)["[-3, 5]"]
    r = A.record_f32(0, h, w, rot_k=2, scale=1.07, shift=(2, -1))
    assert np.array_equal(CO.apply_mask_cubic(f, r)[0], FO.apply(f, r, FO.MASK, 0, 0, 0)[0])


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_zero_angle_with_the_flag_set_is_the_identity(shape):
    """Prefilter and interpolation are inverse on the grid."""
    h, w = shape
    r = A.record_f32(0, h, w, angle=0.0)
    assert int(r["flags"]) & A.ROT_F
    for what, f in _fields(shape).items():
        d = np.abs(CO.apply_mask_cubic(f, r)[0] - f.astype(np.float64)).max()
        print(f"identity {shape} {what}: max |diff| {d:.3e}")
        assert d <= 1e-12


def test_augmenter_target_interp(tmp_path):
    lin, cub = A.AugmenterF32(shape=(32, 32), seed=4), A.AugmenterF32(shape=(32, 32), seed=4, target_interp="cubic")
    assert lin.target_interp == "linear" and cub.target_interp == "cubic"
    assert lin.describe()["target_interp"] == "linear" and cub.describe()["target_interp"] == "cubic"
    for bad in ("nearest", "", None, 3):
        with pytest.raises(ValueError):
            A.AugmenterF32(target_interp=bad)
    idx = np.arange(200)
    assert lin.draw(2, idx).tobytes() == cub.draw(2, idx).tobytes()              # the mode draws no uniform
    st = TileStore.create(str(tmp_path / "s"), 2, {"image": (8, 8), "distance": (8, 8)}, {"dim_out": [8, 8], "scale_limit": [-0.1, 0.2]},
                          dtypes={"distance": "f32"})
    assert A.AugmenterF32.from_store(st).target_interp == "linear"
    own = A.AugmenterF32.from_store(st, target_interp="cubic")
    assert own.target_interp == "cubic" and own.scale_limit == (-0.1, 0.2) and own.shape == (8, 8)
    assert {k: v for k, v in own.describe().items() if k != "target_interp"} == {k: v for k, v in A.AugmenterF32.from_store(st).describe().items()
                                                                                 if k != "target_interp"}
