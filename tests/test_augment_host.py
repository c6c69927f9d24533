"""On-device augmentation, the parts that need no GPU: exported symbols, the Philox restatement against published known answers, purity and
statistics of ``Augmenter.draw``, sanity of the float64 oracle against numpy / scipy (so the checker of the GPU tests is not checked only
against itself), and the Trainers' refusal of ``augment=True`` where it cannot work."""
import ctypes as C

import numpy as np
import pytest
import torch

import bio_image_unet_amd._lib as L
from bio_image_unet_amd import augment as A
from tests import augment_oracle as AO


def test_library_exports_and_binds_the_augmentation_symbols():
    for name in ("biu_augment_u8", "biu_philox_u32"):
        assert hasattr(L.lib._c, name) and name in L.SIGNATURES
    assert C.sizeof(L.biu_aug_params) == A.PARAMS_DTYPE.itemsize == 96
    for name, _ in L.biu_aug_params._fields_:                      # the numpy record and the C struct agree field by field
        assert A.PARAMS_DTYPE.fields[name][1] == getattr(L.biu_aug_params, name).offset
    assert (A.GATE, A.SSR, A.BC, A.BLUR, A.MULT, A.GAUSS) == (AO.GATE, AO.SSR, AO.BC, AO.BLUR, AO.MULT, AO.GAUSS)


def test_numpy_philox_reproduces_the_known_answers():
    h = lambda s: np.array([int(v, 16) for v in s.split()], dtype=np.uint32)
    kat = [("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert np.array_equal(AO.philox4x32_10(h(ctr)[None], h(key))[0], h(want))
    # the uniform is (u >> 8) * 2^-24: in [0, 1), the low byte does not count
    assert AO.uniform24(np.uint32(0xFFFFFFFF)) == 1.0 - 2.0 ** -24 and AO.uniform24(np.uint32(0xFF)) == 0.0


def _aug(recipe="unet", **kw):
    kw.setdefault("shiftscalerotate", (0.1, 0.2, 30))
    kw.setdefault("shape", (64, 64))
    return A.Augmenter(recipe, **kw)


def test_draw_is_a_pure_function_of_seed_epoch_index():
    a = _aug(seed=7)
    alone = [a.draw(3, [i]) for i in (5, 9, 2)]
    batch = a.draw(3, [5, 9, 2])
    other_order = a.draw(3, [2, 5, 9])
    for j, r in enumerate(alone):
        assert r[0].tobytes() == batch[j].tobytes()
    assert other_order[0].tobytes() == batch[2].tobytes() and other_order[1].tobytes() == batch[0].tobytes()
    assert _aug(seed=7).draw(3, [5])[0].tobytes() == batch[0].tobytes()              # a second object, the same record
    idx = list(range(64))
    assert a.draw(3, idx).tobytes() != a.draw(4, idx).tobytes()
    assert a.draw(3, idx).tobytes() != _aug(seed=8).draw(3, idx).tobytes()
    assert np.array_equal(batch["index"], [5, 9, 2])
    # a drawn record says everything about itself: rebuilt from its logical fields it is the same bytes (matrix included)
    for r in a.draw(1, np.arange(300)):
        f = int(r["flags"])
        again = A.record(int(r["index"]), 64, 64, gate=bool(f & A.GATE), rot_k=int(r["rot_k"]),
                         ssr=(r["angle"], r["scale"], r["dx"], r["dy"]) if f & A.SSR else None,
                         bc=(float(r["alpha"]), float(r["beta"]) / 255.0) if f & A.BC else None, blur_k=int(r["blur_k"]),
                         mult=(float(r["noise_a"]), float(r["noise_a"]) + float(r["noise_b"])) if f & A.MULT else None)
        assert np.array_equal(again["m"], r["m"]) and int(again["flags"]) == f and again["alpha"] == r["alpha"]


def test_draw_gate_frequencies_and_parameter_ranges():
    n = 20000
    a = _aug(seed=1, blur_limit=(3, 7))
    r = a.draw(0, np.arange(n))
    f = r["flags"]
    gate = (f & A.GATE) != 0

    def within(count, total, p):
        assert abs(count - total * p) <= 4.0 * np.sqrt(total * p * (1 - p)), (count, total, p)
    within(gate.sum(), n, 0.8)
    ng = int(gate.sum())
    for bit, p in ((A.SSR, 0.5), (A.BC, 0.5), (A.BLUR, 0.2), (A.MULT, 0.3)):
        within(((f & bit) != 0).sum(), ng, p)                                      # a stage only ever runs behind the gate
        assert not ((f & bit) != 0)[~gate].any()
    assert not (f & A.GAUSS).any()
    for k in range(4):
        within((r["rot_k"][gate] == k).sum(), ng, 0.25)
    ssr, bc, blur, mult = ((f & b) != 0 for b in (A.SSR, A.BC, A.BLUR, A.MULT))
    assert np.abs(r["angle"][ssr]).max() <= 30 and np.abs(r["angle"][ssr]).max() > 29
    assert r["scale"][ssr].min() >= 0.8 - 1e-6 and r["scale"][ssr].max() <= 1.2 + 1e-6 and np.ptp(r["scale"][ssr]) > 0.39
    for d in ("dx", "dy"):
        assert np.abs(r[d][ssr]).max() <= 0.1 + 1e-7 and np.abs(r[d][ssr]).max() > 0.099
    assert r["alpha"][bc].min() >= 0.75 and r["alpha"][bc].max() <= 1.25 and np.ptp(r["alpha"][bc]) > 0.49
    assert np.abs(r["beta"][bc]).max() <= 0.25 * 255 + 1e-4 and np.abs(r["beta"][bc]).max() > 0.249 * 255
    assert set(np.unique(r["blur_k"][blur])) == {3, 5, 7}
    for k in (3, 5, 7):
        within((r["blur_k"][blur] == k).sum(), int(blur.sum()), 1 / 3)
    assert np.allclose(r["noise_a"][mult], 0.5) and np.allclose(r["noise_b"][mult], 0.7)
    # samples behind a closed gate, and stages not drawn, leave the identity
    ident = A.inverse_matrix(0, 0, 1, 0, 0, 64, 64)
    assert np.array_equal(r["m"][~gate], np.broadcast_to(ident, ((~gate).sum(), 6)))
    assert np.all(r["alpha"][~bc] == 1) and np.all(r["beta"][~bc] == 0)
    # the siam / unet3d recipes: gauss noise of variance noise_amp with p = 0.3, no blur, no multiplicative noise; odd turns only on squares
    s = A.Augmenter("unet3d", noise_amp=10, seed=2).draw(0, np.arange(n), shape=(8, 64, 96))
    g = (s["flags"] & A.GATE) != 0
    within(((s["flags"] & A.GAUSS) != 0).sum(), int(g.sum()), 0.3)
    assert not (s["flags"] & (A.BLUR | A.MULT)).any()
    assert np.allclose(s["noise_a"][(s["flags"] & A.GAUSS) != 0], np.sqrt(10.0))
    assert set(np.unique(s["rot_k"])) == {0, 2}


def test_augmenter_arguments_are_validated():
    with pytest.raises(ValueError):
        A.Augmenter("unet", blur_limit=(3, 17))
    with pytest.raises(ValueError):
        A.Augmenter("nested")
    with pytest.raises(ValueError):
        A.Augmenter("unet", kinds={"image": "label"})
    with pytest.raises(ValueError):
        A.Augmenter("unet").draw(0, [0])                                             # no tile shape anywhere
    with pytest.raises(ValueError):
        A.inverse_matrix(1, 0, 1, 0, 0, 64, 96)
    d = A.Augmenter("siam", noise_amp=4, seed=3).describe()
    assert d["recipe"] == "siam" and d["noise_amp"] == 4 and d["p"] == 0.8 and d["seed"] == 3


def _noise_image(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _blob_mask(shape, seed=0):
    p, h, w = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros(shape, dtype=bool)
    for q in range(p):
        for _ in range(6):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, min(h, w) / 5)
            m[q] |= (y - cy) ** 2 + (x - cx) ** 2 < r * r
    return (m * 255).astype(np.uint8)


def _gather_by_matrix(f, m):
    """Nearest-neighbour gather through a record's 2x3 matrix (what the kernel is handed), in float64."""
    _, h, w = f.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    sx, sy = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    return f[:, AO.reflect101(np.rint(sy).astype(np.int64), h), AO.reflect101(np.rint(sx).astype(np.int64), w)]


def test_oracle_identity_rot90_and_whole_pixel_shifts():
    img, msk = _noise_image((2, 48, 48)), _blob_mask((2, 48, 48))
    ident = A.record(0, 48, 48, gate=False)
    for f, is_mask in ((img, False), (msk, True)):
        out, safe = AO.apply(f, ident, is_mask, AO.ORDER_UNET, 0, 0, 1)
        assert np.array_equal(out, f) and safe.all()
        for k in range(4):
            rec = A.record(0, 48, 48, rot_k=k)
            assert np.array_equal(AO.apply(f, rec, is_mask, AO.ORDER_UNET, 0, 0, 1)[0], np.rot90(f, k, axes=(1, 2)))
            # the matrix the kernel gets composes the same permutation, with exact integer entries
            assert np.array_equal(rec["m"], np.rint(rec["m"])) and np.array_equal(_gather_by_matrix(f, rec["m"]), np.rot90(f, k, axes=(1, 2)))
    # non-square tiles: half turns only
    ns = _noise_image((1, 32, 48), 1)
    rec = A.record(0, 32, 48, rot_k=2)
    assert np.array_equal(AO.apply(ns, rec, False, AO.ORDER_UNET, 0, 0, 1)[0], ns[:, ::-1, ::-1])
    assert np.array_equal(_gather_by_matrix(ns, rec["m"]), ns[:, ::-1, ::-1])
    # a shift by whole pixels == reflect-101 pad + crop: dx = 3/48 moves the content 3 pixels to the right, dy = -5/32 ... 5 rows up
    for (h, w, sx, sy) in ((48, 48, 3, 0), (48, 48, -4, 6), (32, 48, 3, -5)):
        f = _noise_image((2, h, w), 2)
        rec = A.record(0, h, w, ssr=(0.0, 1.0, sx / w, sy / h))
        pad = np.pad(f, ((0, 0), (8, 8), (8, 8)), mode="reflect")
        want = pad[:, 8 - sy:8 - sy + h, 8 - sx:8 - sx + w]
        for is_mask in (False, True):
            assert np.array_equal(AO.apply(f, rec, is_mask, AO.ORDER_UNET, 0, 0, 1)[0], want)
        assert np.array_equal(_gather_by_matrix(f, rec["m"]), want)
        # rot90 and a whole-pixel shift together: still one exact permutation matrix
        if h == w:
            rec = A.record(0, h, w, rot_k=3, ssr=(0.0, 1.0, sx / w, sy / h))
            assert np.array_equal(_gather_by_matrix(f, rec["m"]), AO.apply(f, rec, True, AO.ORDER_UNET, 0, 0, 1)[0])


def test_oracle_rotation_sign_convention():
    """+90 degrees through shift_scale_rotate == np.rot90(x, 1), -90 degrees == np.rot90(x, 3) (square tile)."""
    img, msk = _noise_image((1, 40, 40), 3), _blob_mask((1, 40, 40), 3)
    for angle, k in ((90.0, 1), (-90.0, 3)):
        rec = A.record(0, 40, 40, ssr=(angle, 1.0, 0.0, 0.0))
        assert np.array_equal(AO.apply(img, rec, False, AO.ORDER_SIAM, 0, 0, 1)[0], np.rot90(img, k, axes=(1, 2)))
        assert np.array_equal(_gather_by_matrix(msk, rec["m"].astype(np.float64)), np.rot90(msk, k, axes=(1, 2)))
    # a general rotation through the kernel's matrix agrees with the oracle's own geometry on every safe pixel
    for ssr in ((17.3, 1.07, 0.03, -0.05), (-151.0, 0.9, 1 / 16, 1 / 16), (3.7, 1.2, -0.1, 0.1)):
        for k in (0, 1, 2, 3):
            f = _blob_mask((1, 256, 256), 4)
            rec = A.record(0, 256, 256, rot_k=k, ssr=ssr)
            want, safe = AO.apply(f, rec, True, AO.ORDER_UNET, 0, 0, 1)
            got = _gather_by_matrix(f, rec["m"].astype(np.float64))
            assert (~safe).mean() <= 0.01 and np.array_equal(got[:, safe], want[:, safe])


def test_oracle_box_blur_equals_scipy_uniform_filter():
    from scipy import ndimage
    img = _noise_image((2, 40, 56), 5).astype(np.float64)
    for k in (3, 5, 7, 15):
        want = np.stack([ndimage.uniform_filter(p, size=k, mode="mirror") for p in img])
        assert np.array_equal(AO.box_blur(img, k), AO.quant8(want))
    rec = A.record(0, 40, 56, blur_k=5)
    assert np.array_equal(AO.apply(img.astype(np.uint8), rec, False, AO.ORDER_UNET, 0, 0, 1)[0], AO.box_blur(img, 5).astype(np.uint8))


def test_oracle_mask_keeps_its_histogram_under_rot90_and_ignores_intensity_stages():
    msk = _blob_mask((3, 64, 64), 6)
    for k in range(4):
        rec = A.record(11, 64, 64, rot_k=k, bc=(1.2, 0.1), blur_k=7, mult=(0.5, 1.2))
        out, _ = AO.apply(msk, rec, True, AO.ORDER_UNET, 5, 2, 9)
        assert np.array_equal(np.bincount(out.ravel(), minlength=256), np.bincount(msk.ravel(), minlength=256))
        assert np.array_equal(out, np.rot90(msk, k, axes=(1, 2)))


def test_oracle_noise_statistics():
    """The same bounds the GPU test sets for the kernel: they are >= 4 standard errors at 262 144 samples."""
    f = np.full((1, 512, 512), 100, dtype=np.uint8)
    m = AO.apply(f, A.record(3, 512, 512, mult=(0.5, 1.2)), False, AO.ORDER_UNET, 42, 1, 77)[0].astype(np.float64)
    assert abs(m.mean() - 85.0) < 0.2 and m.min() >= 50 and m.max() <= 120
    g = AO.apply(f, A.record(3, 512, 512, gauss_sigma=10.0), False, AO.ORDER_SIAM, 42, 1, 77)[0].astype(np.float64)
    assert abs(g.mean() - 100.0) < 0.1 and abs(g.std() - 10.0) < 0.1
    # another epoch, index, field or seed: another stream
    base = AO.noise_words(64, 4, 42, 3, 1, 77, AO.STAGE_MULT)
    for other in (AO.noise_words(64, 4, 43, 3, 1, 77, AO.STAGE_MULT), AO.noise_words(64, 4, 42, 4, 1, 77, AO.STAGE_MULT),
                  AO.noise_words(64, 4, 42, 3, 2, 77, AO.STAGE_MULT), AO.noise_words(64, 4, 42, 3, 1, 78, AO.STAGE_MULT)):
        assert not np.array_equal(base, other)


class _Floats(torch.utils.data.Dataset):
    dim_out = (16, 16)

    def __len__(self):
        return 8

    def __getitem__(self, i):
        return {"image": torch.zeros(16, 16), "mask": torch.zeros(16, 16)}


def test_trainers_refuse_augment_without_a_store_or_a_gpu(tmp_path):
    import bio_image_unet_amd.siam_unet as siam
    import bio_image_unet_amd.unet as unet
    import bio_image_unet_amd.unet3d as unet3d
    from bio_image_unet_amd.feed import TileStore
    st = TileStore.create(str(tmp_path / "s"), 8, {"image": (16, 16), "mask": (16, 16)}, {"dim_out": [16, 16], "blur_limit": [3, 5]})
    assert A.Augmenter.from_store(st, "unet").blur_limit == (3, 5) and A.Augmenter.from_store(st, "unet", seed=4).seed == 4
    for T in (unet.Trainer, unet3d.Trainer, siam.Trainer):
        with pytest.raises(ValueError, match="augment"):
            T(_Floats(), 1, n_filter=4, save_dir=str(tmp_path), device="cuda", augment=True)       # not a store
        with pytest.raises(ValueError, match="augment"):
            T(st, 1, n_filter=4, save_dir=str(tmp_path), device="cpu", augment=True)               # a store, but no GPU
        with pytest.raises(ValueError, match="augment"):
            T(st, 1, n_filter=4, save_dir=str(tmp_path), device="cpu", augment=A.Augmenter("unet"))
