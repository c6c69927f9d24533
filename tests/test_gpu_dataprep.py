"""Data preparation on the device (``bio_image_unet_amd/dataprep.py``, ``csrc/biu_dataprep.hip``) against the numpy oracle
(``tests/dataprep_oracle.py``): grey morphology, Zhang-Suen thinning, the uint8 tile gather, and the three entry points end to end -- store
fields byte for byte, the recorded limits, and a Trainer that takes the store with ``augment=True``.  Every comparison is an equality."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bio_image_unet_amd.siam_unet as siam  # noqa: E402
import bio_image_unet_amd.unet as unet  # noqa: E402
import bio_image_unet_amd.unet3d as unet3d  # noqa: E402
from bio_image_unet_amd import dataprep as DP  # noqa: E402
from bio_image_unet_amd._lib import BiuError  # noqa: E402
from tests import dataprep_oracle as DO  # noqa: E402

FOOTPRINTS = [("disk", 1), ("disk", 2), ("disk", 3), ("disk", 7), ("square", 1), ("square", 2), ("square", 3), ("square", 4)]
MORPH_SHAPES = [(1, 37, 53), (3, 64, 64), (2, 130, 70), (1, 1, 9), (1, 5, 1)]       # ragged last tile, two tile rows, degenerate planes


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- morphology --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,size", FOOTPRINTS)
@pytest.mark.parametrize("shape", MORPH_SHAPES)
def test_morphology_equals_oracle(shape, kernel, size):
    rng = np.random.default_rng(size + 100 * shape[1])
    grey = rng.integers(0, 256, shape, dtype=np.uint8)
    binary = ((rng.random(shape) < 0.5) * 255).astype(np.uint8)
    binary[:, shape[1] // 2:, :] = np.where(rng.random(binary[:, shape[1] // 2:, :].shape) < 0.97, 255, 0)    # sparse holes: structures wider than a pixel
    for name, x in (("grey", grey), ("binary", binary)):
        for op in ("erosion", "dilation"):
            got = DP.morph(_dev(x), op, kernel, size).cpu().numpy()
            assert np.array_equal(got, DO.morph(x, op, kernel, size)), (name, op, kernel, size, shape)


def test_morphology_refuses_larger_footprints_and_unknown_kernels():
    x = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    for kernel, size in (("disk", 8), ("square", 16), ("disk", 0), ("square", 0)):
        with pytest.raises(BiuError, match=rf"{kernel}\({size}\) is not supported"):
            DP.morph(x, "erosion", kernel, size)
    with pytest.raises(ValueError, match="^Dilate kernel star unknown!$"):
        DP.morph(x, "erosion", "star", 1)
    for kernel, size in (("disk", 7), ("square", 15), ("square", 14)):              # the largest ones run
        assert int(DP.morph(x + 7, "dilation", kernel, size).min()) == 7


# ---- thinning ----------------------------------------------------------------------------------------------------------------------------
def _thin_case(name):
    if name == "empty":
        return np.zeros((1, 33, 45), dtype=np.uint8)
    if name == "all_ones":                                   # the border matters: outside is 0
        return np.ones((1, 65, 67), dtype=np.uint8)
    if name == "square_at_two_edges":
        x = np.zeros((1, 70, 70), dtype=np.uint8)
        x[0, :64, :64] = 1
        return x
    if name == "ring":
        y, c = np.mgrid[:90, :150]
        r = np.hypot(y - 44.5, c - 70.0)
        return ((r < 40) & (r > 25)).astype(np.uint8)[None]
    if name == "blobs":
        import scipy.ndimage as ndi
        return ndi.binary_dilation(np.random.default_rng(7).random((97, 131)) < 0.03, iterations=3).astype(np.uint8)[None]
    if name == "line":
        return np.ones((1, 1, 40), dtype=np.uint8)
    if name == "three_planes":
        x = np.zeros((3, 40, 140), dtype=np.uint8)
        x[0, 5:11, 5:11] = 1
        x[1, 4:34, 100:136] = 1                              # (beyond the first 128-column tile)
        x[2, 20, 3:130] = 1
        return x
    raise KeyError(name)


THIN_CASES = ["empty", "all_ones", "square_at_two_edges", "ring", "blobs", "line", "three_planes"]


@functools.lru_cache(maxsize=None)
def _thin_ref(name):
    out, its = DO.thin(_thin_case(name), return_iterations=True)
    out.setflags(write=False)
    return out, tuple(its)


@pytest.mark.parametrize("name", THIN_CASES)
def test_thinning_equals_oracle(name):
    if name == "blobs":
        pytest.importorskip("scipy.ndimage")
    x = _thin_case(name)
    want, its = _thin_ref(name)
    print(f"{name}: {int(x.sum())} -> {int(want.sum())} pixels, oracle iterations per plane {its}")
    if name == "square_at_two_edges":
        assert its == (33,)
    if name == "three_planes":
        assert len(set(its)) == 3                            # the planes converge after different iteration counts
    got8 = DP.thin(_dev(x))
    assert got8.dtype == torch.uint8 and np.array_equal(got8.cpu().numpy(), want)
    got1 = DP.thin(_dev(x), block=1)
    assert torch.equal(got1, got8)                           # the result does not depend on the block of iterations between two reads
    assert torch.equal(DP.thin(got8), got8)                  # a fixed point
    assert np.array_equal(DP.thin(_dev(x * 255)).cpu().numpy(), want)       # nonzero counts as set


def test_thin_step_counts_what_it_cleared():
    import ctypes as C

    from bio_image_unet_amd._lib import check, lib
    x = _thin_case("three_planes")
    src, dst = _dev(x), torch.empty(x.shape, dtype=torch.uint8, device="cuda")
    table, counter = _dev(DP.thin_table()), torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    total = 0
    for sub in (0, 1):
        check(lib.biu_thin_step_u8(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), *x.shape, sub, C.c_void_p(table.data_ptr()),
                                   C.c_void_p(counter.data_ptr()), stream), "thin_step_u8")
        want = np.stack([DO.thin_step(p, sub)[0] for p in src.cpu().numpy()])
        total += int((src.cpu().numpy() != want).sum())
        assert np.array_equal(dst.cpu().numpy(), want)
        assert int(counter.item()) == total and total > 0    # one counter per call, summed over the planes
        src, dst = dst, src


# ---- gather ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("shape,tile", [((20, 300), (32, 64)), ((20, 300), (32, 128)), ((5, 40, 70), (8, 32, 32)), ((3, 33, 50), (2, 16, 24))])
def test_gather_equals_pad_and_slice(shape, tile, add, invert):
    x = np.random.default_rng(len(shape) + add).integers(0, 256, shape, dtype=np.uint8)
    if len(shape) == 2:
        org = [(0, y, c) for y, c in DP.origins_2d(shape, tile, add)]
        got = DP.gather(_dev(x[None]), 1, org, (1,) + tile, invert)[:, 0]
        want = DO.split(x, tile, add)
    else:
        org = DP.origins_3d(shape, tile, add)
        got = DP.gather(_dev(x), shape[0], org, tile, invert)
        want = DO.split(x, tile, add, quirk_3d=True)
    if shape == (20, 300) and add == 0:
        assert len(org) == (5 if tile[1] == 64 else 3)       # reflect on one axis, several tiles on the other
    assert np.array_equal(got.cpu().numpy(), 255 - want if invert else want)


def test_gather_keeps_tiles_inside_their_volume():
    x = np.random.default_rng(9).integers(0, 256, (6, 10, 20), dtype=np.uint8)      # two volumes of three planes
    got = DP.gather(_dev(x), 3, [(0, 0, 0), (3, 0, 4), (4, 2, 0)], (4, 8, 16)).cpu().numpy()
    for t, (v, z, y, c) in enumerate([(0, 0, 0, 0), (1, 0, 0, 4), (1, 1, 2, 0)]):
        want = np.pad(x[3 * v:3 * v + 3], ((0, 4), (0, 8), (0, 16)), "reflect")[z:z + 4, y:y + 8, c:c + 16]
        assert np.array_equal(got[t], want), t


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def _blobs(shape, seed, grey=False):
    """Label masks: filled ellipses at 255 (with ``grey``: a ramp of grey levels over them, some of them 1 and 2 -- the binarisation edge)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:shape[-2], :shape[-1]]
    m = np.zeros(shape, dtype=np.uint8)
    for p in m.reshape((-1,) + shape[-2:]):
        for _ in range(4):
            cy, cx, a, b = rng.uniform(0, shape[-2]), rng.uniform(0, shape[-1]), rng.uniform(3, 9), rng.uniform(3, 9)
            p[((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2 < 1] = 255
    if grey:
        m = np.where(m > 0, rng.integers(1, 256, shape), rng.integers(0, 3, shape)).astype(np.uint8)
    return m


def _raw(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.gamma(2.0, 900.0, shape)).clip(0, 65535).astype(np.uint16)


RUNS = [dict(skeletonize=True, dilate_mask=-1), dict(dilate_mask=2, dilate_kernel="square", invert=True)]
LIMITS = dict(clip_threshold=(0.5, 99.5), shiftscalerotate=(0.1, 0.2, 30), brightness_contrast=(0.2, 0.3))


def _check_store(store, want, n_fields, dim_out, **limits):
    assert set(store.fields) == set(want) and len(store.fields) == n_fields
    for k, v in want.items():
        assert store.fields[k] == v.shape[1:] and store.n == v.shape[0], (k, store.fields[k], v.shape)
        got = np.asarray(store.maps[k])
        assert got.dtype == np.uint8 and np.array_equal(got, v), f"field {k}: {int((got != v).sum())} of {v.size} bytes differ"
    assert store.attrs["dim_out"] == list(dim_out) and store.dim_out == tuple(dim_out)
    for k, v in limits.items():
        assert store.attrs[k] == list(v) if isinstance(v, tuple) else store.attrs[k] == v, (k, store.attrs[k], v)


def _train(T, store, tmp_path, recipe, **kw):
    torch.manual_seed(0)
    tr = T(store, 1, n_filter=4, batch_size=2, augment=True, save_dir=str(tmp_path / "out"), **kw)
    assert tr.augmenter.recipe == recipe and tr.augmenter.shiftscalerotate == (0.1, 0.2, 30.0) and tr.augmenter.brightness_contrast == (0.2, 0.3)
    tr.start()
    ck = torch.load(str(tmp_path / "out" / "model.pt"), weights_only=False)
    print(f"{T.__name__}(store, 1, n_filter=4, batch_size=2, augment=True): validation loss {float(ck['best_loss']):.6f}")
    assert torch.isfinite(torch.as_tensor(ck["best_loss"]))
    assert ck["clip_threshold"] == [0.5, 99.5]
    return tr


@pytest.mark.parametrize("run", [0, 1])
def test_prepare_unet_end_to_end(tmp_path, run):
    c = 1 + run                                              # the second run carries a channel axis on both fields
    shapes = [(40, 70), (20, 50)]                            # the second item is smaller than dim_out on its first axis
    images = [_raw(s if c == 1 else (c,) + s, 10 + i) for i, s in enumerate(shapes)]
    masks = [_blobs(s if c == 1 else (c,) + s, 20 + i, grey=bool(run)) for i, s in enumerate(shapes)]
    kw = RUNS[run]
    store = unet.prepare(images, masks, str(tmp_path / "st"), dim_out=(32, 32), in_channels=c, out_channels=c, add_tile=1 - run, noise_lims=(0.6, 1.1),
                         blur_limit=(3, 5), device="cuda", **kw, **LIMITS)
    want = DO.pipeline_unet(images, masks, (32, 32), add_tile=1 - run, clip=LIMITS["clip_threshold"], **kw)
    assert want["image"].shape[1:] == ((32, 32) if c == 1 else (c, 32, 32)) and want["mask"].shape[0] == (15 if run == 0 else 8)
    _check_store(store, want, 2, (32, 32), noise_lims=(0.6, 1.1), blur_limit=(3, 5), **LIMITS)
    assert 0 < want["mask"].mean() < 255
    if run == 0:
        tr = _train(unet.Trainer, store, tmp_path, "unet")
        assert tr.augmenter.noise_lims == (0.6, 1.1) and tr.augmenter.blur_limit == (3, 5)


@pytest.mark.parametrize("run", [0, 1])
def test_prepare_unet3d_end_to_end(tmp_path, run):
    shapes = [(10, 20, 40), (5, 16, 30)]                     # the second volume is shallower than dim_out
    volumes = [_raw(s, 30 + i) for i, s in enumerate(shapes)]
    masks = [_blobs(s, 40 + i, grey=bool(run)) for i, s in enumerate(shapes)]
    kw = RUNS[run]
    store = unet3d.prepare(volumes, masks, str(tmp_path / "st"), dim_out=(8, 16, 16), add_patch=1 - run, noise_amp=12, device="cuda", **kw, **LIMITS)
    want = DO.pipeline_unet3d(volumes, masks, (8, 16, 16), add_patch=1 - run, clip=LIMITS["clip_threshold"], **kw)
    assert want["volume"].shape[0] == (2 * 4 * 4 + 3 if run == 0 else 2 * 2 * 3 + 2)     # N_x grows twice under add_patch: unet3d/data.py:188-189
    _check_store(store, want, 2, (8, 16, 16), noise_amp=12, **LIMITS)
    if run == 0:
        assert _train(unet3d.Trainer, store, tmp_path, "unet3d").augmenter.noise_amp == 12.0


@pytest.mark.parametrize("run", [0, 1])
def test_prepare_siam_end_to_end(tmp_path, run):
    pairs = [_raw((2, 70, 70), 50), _raw((20, 100), 51)]     # (previous, current) stacked; previous on the left, and lower than dim_out
    masks = [_blobs((70, 70), 60), _blobs((20, 50), 61)]
    kw = dict(skeletonize=True, dilate_mask=-1) if run == 0 else dict(dilate_mask=2, dilate_kernel="square", invert_masks=True, threshold_masks=50)
    store = siam.prepare(pairs, masks, str(tmp_path / "st"), dim_out=(32, 32), noise_amp=12, device="cuda", **kw, **LIMITS)
    want = DO.pipeline_siam(pairs, masks, (32, 32), clip=LIMITS["clip_threshold"], **kw)
    assert want["image"].shape == (11, 32, 32) and not np.array_equal(want["image"], want["prev_image"])
    _check_store(store, want, 3, (32, 32), noise_amp=12, **LIMITS)
    if run == 0:
        assert _train(siam.Trainer, store, tmp_path, "siam", mode="max").augmenter.noise_amp == 12.0
    else:
        assert 0 < want["mask"].mean() < 255 and set(np.unique(want["mask"])) == {0, 255}
        grey = [_blobs((70, 70), 62, grey=True), _blobs((20, 50), 63, grey=True)]
        means = []
        for j, kw in enumerate((dict(dilate_mask=-1), dict(), dict(dilate_mask=1))):       # a negative radius ERODES here; none: the masks as they are
            got = np.asarray(siam.prepare(pairs, grey, str(tmp_path / f"g{j}"), dim_out=(32, 32), device="cuda", **kw).maps["mask"])
            assert np.array_equal(got, DO.pipeline_siam(pairs, grey, (32, 32), **kw)["mask"]), kw
            means.append(got.mean())
        assert means[0] < means[1] < means[2]
