"""Host side of the device front end of the Predict pipelines (``bio_image_unet_amd/preprocess.py``): the binding, the percentile formula the
finalize kernel evaluates, the reflect rule the tile kernel applies, and the tile origins the ``_split`` methods now share with it."""
import numpy as np
import pytest

import bio_image_unet_amd._lib as L
from bio_image_unet_amd import preprocess as P
from bio_image_unet_amd import workflow as Wf


def test_new_symbols_are_bound():
    for name in ("biu_order_stats_workspace", "biu_order_stats", "biu_prep_finalize", "biu_prep_tiles"):
        assert name in L.SIGNATURES and hasattr(L.lib._c, name)
    assert L.lib.biu_order_stats_workspace(3, 6) >= 3 * 6 * 256 * 4
    assert L.lib.biu_order_stats_workspace(3, 9) == 0 and L.lib.biu_order_stats_workspace(0, 6) == 0


def _data(kind, n, rng):
    if kind == "f64":
        return rng.standard_normal(n) * 1e3
    if kind == "u16":
        return rng.integers(0, 65536, n).astype(np.float64)
    if kind == "f32":
        return rng.standard_normal(n).astype(np.float32).astype(np.float64)
    return rng.integers(0, 4, n).astype(np.float64) * 37.0          # long runs of ties


@pytest.mark.parametrize("n", [1, 2, 3, 255, 4099])
@pytest.mark.parametrize("kind", ["f64", "u16", "f32", "ties"])
def test_percentile_from_neighbours_is_numpys(n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    x = _data(kind, n, rng)
    s = np.sort(x)
    for q in (0, 0.2, 50, 99.8, 99.98, 100):
        k, k1 = P.percentile_ranks(q, n)
        assert 0 <= k <= k1 <= n - 1 and k1 - k <= 1
        got = P.percentile_from_neighbours(s[k], s[k1], q, n)
        assert isinstance(got, np.float64)
        want, wantn = np.percentile(x, q), np.nanpercentile(x, q)
        assert got == want and got == wantn, (n, kind, q, float(got), float(want), float(wantn))


def test_percentile_ranks_refuses_out_of_range():
    with pytest.raises(ValueError):
        P.percentile_ranks(100.5, 10)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_reflect_index_is_numpys_reflect(n):
    a = np.arange(n)
    padded = np.pad(a, (0, 25), "reflect")
    assert [P.reflect_index(i, n) for i in range(n + 25)] == list(padded)


def _gather(stack4, origins, tile, pad):
    """The device front end's tile rule restated in numpy: stack4 [images, D, H, W]; beyond the image reflect (or zero)."""
    out = np.zeros((len(origins),) + tile, dtype=stack4.dtype)
    D, H, W = stack4.shape[1:]
    for t, (i, z0, y0, x0) in enumerate(origins):
        for dz in range(tile[0]):
            for dy in range(tile[1]):
                for dx in range(tile[2]):
                    z, y, x = z0 + dz, y0 + dy, x0 + dx
                    if pad == "zero":
                        if z < D and y < H and x < W:
                            out[t, dz, dy, dx] = stack4[i, z, y, x]
                    else:
                        out[t, dz, dy, dx] = stack4[i, P.reflect_index(z, D), P.reflect_index(y, H), P.reflect_index(x, W)]
    return out


def _bare(cls, **attrs):
    obj = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


@pytest.mark.parametrize("resize_dim,add_tile", [((8, 12), 0), ((8, 12), 1), ((24, 32), 0)])
def test_origins_reproduce_split_2d(resize_dim, add_tile):
    imgs = np.random.default_rng(0).integers(0, 256, (3, 19, 27)).astype(np.float64)
    p = _bare(Wf.Predict2D, imgs_shape=imgs.shape, resize_dim=resize_dim, add_tile=add_tile)
    want = p._split(imgs.copy())
    got = _gather(imgs[:, None], p._origins(), (1,) + resize_dim, "reflect").astype("uint8")
    assert want.shape == got.shape and np.array_equal(want, got)


@pytest.mark.parametrize("resize_dim", [(4, 8, 8), (12, 8, 24)])
def test_origins_reproduce_split_3d(resize_dim):
    vol = np.random.default_rng(1).integers(0, 256, (10, 20, 18)).astype(np.float64)
    p = _bare(Wf.Predict3D, vol_shape=vol.shape, resize_dim=resize_dim, add_patch=0)
    want = p._split(vol.copy())
    got = _gather(vol[None], p._origins(), resize_dim, "reflect").astype("uint8")
    assert want.shape == got.shape and np.array_equal(want, got)


@pytest.mark.parametrize("resize_dim", [(8, 12), (24, 32)])
def test_origins_reproduce_split_siam(resize_dim):
    pair = np.random.default_rng(2).integers(0, 256, (2, 19, 27)).astype("uint8")
    p = _bare(Wf.PredictSiam, imgs_shape=[5, 19, 27], resize_dim=resize_dim, add_tile=0)
    want = p._split(pair.copy())
    o = p._origins()
    cur = _gather(pair[1][None, None], o, (1,) + resize_dim, "zero")
    prev = _gather(pair[0][None, None], o, (1,) + resize_dim, "zero")
    assert np.array_equal(want, np.concatenate([cur, prev], axis=1))


def test_origins_reproduce_split_mo3d():
    vols = np.random.default_rng(3).random((2, 10, 20, 18)).astype("float32")
    p = _bare(Wf.PredictMo3d, max_patch_size=(4, 8, 8), overlap_factor=0.25)
    want = p._split(vols)
    got = _gather(vols, p._origins(vols.shape), p.patch_size, "reflect")
    assert want.shape == (len(got), 1) + p.patch_size and np.array_equal(want[:, 0], got)


@pytest.mark.parametrize("shape,max_patch,add_tile", [((2, 50, 80), (48, 48), 0), ((2, 30, 41), (64, 64), 0), ((1, 50, 80), (32, 32), 1)])
def test_origins_reproduce_split_mo2d(shape, max_patch, add_tile):
    imgs = np.random.default_rng(4).random(shape).astype("float32")
    p = _bare(Wf.PredictMo2d, imgs_shape=imgs.shape, max_patch_size=max_patch, add_tile=add_tile)
    want = p._split(imgs)
    got = _gather(imgs[:, None], p._origins(), (1,) + p.patch_size, "reflect")
    assert want.shape == got[:, 0].shape and np.array_equal(want, got[:, 0])


def _with_origins(cls, shape=None, **attrs):
    p = _bare(cls, **attrs)
    return p, (p._origins() if shape is None else p._origins(shape))


STITCH_CASES = {
    "2d": lambda: _with_origins(Wf.Predict2D, imgs_shape=(3, 19, 27), resize_dim=(8, 12), add_tile=1),
    "3d": lambda: _with_origins(Wf.Predict3D, vol_shape=(10, 20, 18), resize_dim=(4, 8, 8), add_patch=1),
    "siam": lambda: _with_origins(Wf.PredictSiam, imgs_shape=[5, 19, 27], resize_dim=(8, 12), add_tile=0),
    "mo3d": lambda: _with_origins(Wf.PredictMo3d, shape=(2, 10, 20, 18), max_patch_size=(4, 8, 8), overlap_factor=0.25),
    "mo2d": lambda: _with_origins(Wf.PredictMo2d, imgs_shape=(2, 50, 80), max_patch_size=(48, 48), add_tile=0),
    "mo2d_add_tile": lambda: _with_origins(Wf.PredictMo2d, imgs_shape=(1, 50, 80), max_patch_size=(32, 32), add_tile=1),
}


@pytest.mark.parametrize("case", list(STITCH_CASES))
def test_stitch_origins_are_the_cut_origins(case):
    """Patch k is stitched into the image its cut origin names, at that origin without the leading index: one list states the tile order for
    the cut (``_split``, the device front end) and for the stitch (``_place``)."""
    p, origins = STITCH_CASES[case]()
    assert len(origins) > 4 and origins is p.origins
    assert [p._place(k) for k in range(len(origins))] == [(o[0], tuple(o[1:])) for o in origins]
    assert len({o[0] for o in origins}) == {"2d": 3, "3d": 1, "siam": 1, "mo3d": 2, "mo2d": 2, "mo2d_add_tile": 1}[case]


def test_mo2d_stitches_on_the_start_grid_where_the_stride_drifts():
    """``PredictMo2d`` keeps upstream's pair of rules: windows are cut on the stride ``X_start[1]`` and stitched at ``X_start``.  With up to
    two tiles per axis, or a stride that divides the extent (the cases above), the two are one grid; 100 rows in four tiles of 32 are not
    (``linspace(0, 68, 4)`` truncates to 0, 22, 45, 68 against 0, 22, 44, 66), and there the stitch follows ``X_start``."""
    p, origins = _with_origins(Wf.PredictMo2d, imgs_shape=(1, 100, 80), max_patch_size=(32, 32), add_tile=0)
    assert list(p.X_start) == [0, 22, 45, 68] and sorted({o[2] for o in origins}) == [0, 22, 44, 66]
    placed = [p._place(k) for k in range(len(origins))]
    assert placed == [(0, (0, int(xs), int(ys))) for xs in p.X_start for ys in p.Y_start]
    assert [at[2] for _, at in placed] == [o[3] for o in origins]           # the columns (0, 24, 48) agree
