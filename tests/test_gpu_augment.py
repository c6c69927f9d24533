"""On-device augmentation on the GPU: ``biu_augment_u8`` / ``biu_philox_u32`` through the C ABI against the float64 oracle
(``tests/augment_oracle.py``), then the feeder and the Trainers that carry it.

Bounds (set by the contract, not by what the kernel gives): masks agree on every pixel whose float64 source coordinate is farther than 1e-3
from a rounding boundary (<= 1 % of a field may be left out); images agree within 1 grey level everywhere and differ at all on <= 0.5 % of
the pixels (an fp32 restatement of the bilinear stage differs from float64 on 0.07-0.08 % of a noise image; the cap leaves six times that
for fused multiply-adds and another operation order).  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bio_image_unet_amd.siam_unet as siam  # noqa: E402
import bio_image_unet_amd.unet as unet  # noqa: E402
import bio_image_unet_amd.unet3d as unet3d  # noqa: E402
from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd._lib import check, lib  # noqa: E402
from bio_image_unet_amd.feed import DeviceFeeder, TileStore  # noqa: E402
from tests import augment_oracle as AO  # noqa: E402

SHAPES = [(1, 256, 256), (2, 96, 96), (16, 64, 64), (1, 64, 96)]       # [planes, H, W]: one plane, channels, z-planes, non-square
GEOMETRY = [(17.3, 1.07, 0.03, -0.05), (-151.0, 0.9, 1 / 16, 1 / 16), (3.7, 1.2, -0.1, 0.1)]      # angle, scale, dx, dy
SEED, EPOCH, FID = 0x1234567890ABCDEF, 3, A.field_id("image")


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


def _run(batch, recs, mask, order=A.ORDER_UNET, seed=SEED, epoch=EPOCH, fid=FID):
    """``batch`` [N, P, H, W] uint8, one record per sample -> the kernel's output as a numpy array."""
    recs = np.ascontiguousarray(recs, dtype=A.PARAMS_DTYPE)
    n, p, h, w = batch.shape
    src = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
    dst = torch.full_like(src, 7)
    par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    blurs = recs["blur_k"][(recs["flags"] & A.BLUR) != 0]
    check(lib.biu_augment_u8(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, p, h, w, int(mask), C.c_void_p(par.data_ptr()), order,
                             0 if mask or not len(blurs) else int(blurs.max()), seed, epoch, fid,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), "augment_u8")
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _oracle(batch, recs, mask, order=A.ORDER_UNET, seed=SEED, epoch=EPOCH, fid=FID):
    outs, safes = zip(*[AO.apply(batch[i], recs[i], mask, order, seed, epoch, fid) for i in range(len(batch))])
    return np.stack(outs), np.stack(safes)


def _rots(h, w):
    return (0, 1, 2, 3) if h == w else (0, 2)


@pytest.mark.timeout(300)
def test_philox_stream_matches_numpy():
    n = 4096
    for seed, c0, c1, c2, c3 in ((0, 0, 0, 0, 0), (SEED, 0xFFFFFFF0, 17, 3, 0xABCDEF12), (0xFFFFFFFFFFFFFFFF, 5, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        out = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
        check(lib.biu_philox_u32(C.c_void_p(out.data_ptr()), n, seed, c0, c1, c2, c3, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "philox")
        ctr = np.zeros((n, 4), dtype=np.uint32)
        ctr[:, 0] = (c0 + np.arange(n, dtype=np.uint64)).astype(np.uint32)            # the first word wraps
        ctr[:, 1], ctr[:, 2], ctr[:, 3] = c1, c2, c3
        want = AO.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(n, 4), want)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_cases(shape):
    """Gate off, rot90 for every k, whole-pixel shifts (alone and behind a rot90): images AND masks equal the oracle bit for bit, and
    two launches with the same arguments give the same bytes."""
    p, h, w = shape
    recs = [A.record(0, h, w, gate=False)]
    recs += [A.record(i + 1, h, w, rot_k=k) for i, k in enumerate(_rots(h, w))]
    recs += [A.record(10 + i, h, w, rot_k=k, ssr=(0.0, 1.0, sx / w, sy / h)) for i, (k, sx, sy) in
             enumerate([(0, 3, 0), (0, -4, 6), (2, 5, -7), (_rots(h, w)[1], w // 16, h // 16)])]
    recs = np.stack(recs)
    img = np.stack([_noise_image(shape, i) for i in range(len(recs))])
    msk = np.stack([_blob_mask(shape, i) for i in range(len(recs))])
    for batch, is_mask in ((img, False), (msk, True), (img, True)):
        got = _run(batch, recs, is_mask)
        want, _ = _oracle(batch, recs, is_mask)
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(want))
        assert np.array_equal(got[0], batch[0])                                       # the closed gate passes the sample unchanged
        assert torch.equal(torch.from_numpy(_run(batch, recs, is_mask)), torch.from_numpy(got))
    # the same through the tile kernel (a blurring neighbour in the batch sends the whole launch there), and with every noise stage drawn
    full = np.stack([A.record(0, h, w, rot_k=2, ssr=GEOMETRY[0], bc=(1.1, 0.05), blur_k=5, mult=(0.5, 1.2)), A.record(1, h, w, gate=False),
                     A.record(2, h, w, rot_k=2)])
    got = _run(img[:3], full, False)
    assert np.array_equal(got[1], img[1]) and np.array_equal(got[2], img[2, :, ::-1, ::-1])
    assert torch.equal(torch.from_numpy(_run(img[:3], full, False)), torch.from_numpy(got))
    siam_full = np.stack([A.record(0, h, w, rot_k=2, ssr=GEOMETRY[1], bc=(0.9, -0.05), gauss_sigma=10.0)] * 2)
    a, b = _run(img[:2], siam_full, False, A.ORDER_SIAM), _run(img[:2], siam_full, False, A.ORDER_SIAM)
    assert torch.equal(torch.from_numpy(a), torch.from_numpy(b))
    assert not np.array_equal(a, _run(img[:2], siam_full, False, A.ORDER_SIAM, epoch=EPOCH + 1))      # another epoch, another noise


@pytest.mark.timeout(600)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_nearest_gather(shape):
    p, h, w = shape
    recs = np.stack([A.record(i, h, w, rot_k=_rots(h, w)[i % len(_rots(h, w))], ssr=g) for i, g in enumerate(GEOMETRY)]
                    + [A.record(9, h, w, ssr=g) for g in GEOMETRY])
    msk = np.stack([_blob_mask(shape, i) for i in range(len(recs))])
    got = _run(msk, recs, True)
    want, safe = _oracle(msk, recs, True)
    for i in range(len(recs)):
        left_out = 1.0 - safe[i].mean()
        bad = (got[i] != want[i])[:, safe[i]].sum()
        print(f"mask {shape} rec {i}: left out {100 * left_out:.3f} %, mismatches on safe pixels {bad}, on all pixels {(got[i] != want[i]).sum()}")
        assert left_out <= 0.01
        assert bad == 0
    assert set(np.unique(got)) <= {0, 255}


def _image_check(what, got, want, rows):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((d > 0).mean())
    rows.append((what, int(d.max()), share))
    print(f"image {what}: max |diff| {d.max()}, differing {100 * share:.4f} %")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_image_stages_and_recipes(shape):
    """Every stage alone, then both whole recipes, within 1 grey level everywhere and differing on <= 0.5 % of the pixels."""
    p, h, w = shape
    rk = _rots(h, w)
    U, S = A.ORDER_UNET, A.ORDER_SIAM
    cases = [("bilinear", U, [A.record(i, h, w, ssr=g) for i, g in enumerate(GEOMETRY)]),
             ("rot90+bilinear", U, [A.record(i, h, w, rot_k=rk[(i + 1) % len(rk)], ssr=g) for i, g in enumerate(GEOMETRY)]),
             ("brightness_contrast", U, [A.record(0, h, w, bc=(1.25, 0.25)), A.record(1, h, w, bc=(0.75, -0.25)), A.record(2, h, w, bc=(1.1337, 0.0421))]),
             ("blur", U, [A.record(i, h, w, blur_k=k) for i, k in enumerate((3, 5, 7, 15))] + [A.record(7, h, w)]),
             ("mult_noise", U, [A.record(5, h, w, mult=(0.5, 1.2)), A.record(6, h, w, mult=(0.5, 1.2))]),
             ("gauss_noise", S, [A.record(5, h, w, gauss_sigma=np.sqrt(10.0)), A.record(6, h, w, gauss_sigma=10.0)]),
             ("recipe unet", U, [A.record(i, h, w, rot_k=rk[i % len(rk)], ssr=g, bc=(1.0 + 0.1 * (i - 1), 0.05 * (1 - i)), blur_k=(3, 7, 0)[i],
                                          mult=(0.5, 1.2)) for i, g in enumerate(GEOMETRY)]),
             ("recipe siam", S, [A.record(i, h, w, rot_k=rk[i % len(rk)], ssr=g, bc=(1.0 + 0.1 * (i - 1), 0.05 * (1 - i)), gauss_sigma=np.sqrt(10.0))
                                 for i, g in enumerate(GEOMETRY)])]
    rows = []
    for what, order, recs in cases:
        recs = np.stack(recs)
        img = np.stack([_noise_image(shape, 100 + i) for i in range(len(recs))])
        _image_check(f"{what} {shape}", _run(img, recs, False, order), _oracle(img, recs, False, order)[0], rows)
    for what, mx, share in rows:
        assert mx <= 1, (what, mx)
        assert share <= 0.005, (what, share)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("shape", [(3, 24, 40), (2, 19, 37), (1, 70, 130)], ids=lambda s: "x".join(map(str, s)))
def test_widths_that_are_no_multiple_of_16(shape):
    """Rows that do not divide into 16-byte groups (and tiles cut by the border) take the element-wise paths: same checks."""
    p, h, w = shape
    exact = np.stack([A.record(0, h, w, gate=False), A.record(1, h, w, rot_k=2), A.record(2, h, w, rot_k=2, ssr=(0.0, 1.0, 3 / w, -2 / h))])
    img = np.stack([_noise_image(shape, 50 + i) for i in range(3)])
    msk = np.stack([_blob_mask(shape, 50 + i) for i in range(3)])
    for batch, is_mask in ((img, False), (msk, True)):
        assert torch.equal(torch.from_numpy(_run(batch, exact, is_mask)), torch.from_numpy(_oracle(batch, exact, is_mask)[0]))
    geo = np.stack([A.record(i, h, w, rot_k=2 * (i % 2), ssr=g) for i, g in enumerate(GEOMETRY)])
    got, (want, safe) = _run(msk, geo, True), _oracle(msk, geo, True)
    for i in range(3):
        assert 1.0 - safe[i].mean() <= 0.01 and (got[i] != want[i])[:, safe[i]].sum() == 0
    rows = []
    for what, order, recs in (("unet", A.ORDER_UNET, [A.record(i, h, w, rot_k=2 * (i % 2), ssr=g, bc=(0.9, 0.05), blur_k=(5, 0, 15)[i], mult=(0.5, 1.0))
                                                     for i, g in enumerate(GEOMETRY)]),
                              ("unet, no blur", A.ORDER_UNET, [A.record(i, h, w, ssr=g, bc=(0.9, 0.05), mult=(0.5, 1.0)) for i, g in enumerate(GEOMETRY)]),
                              ("siam", A.ORDER_SIAM, [A.record(i, h, w, ssr=g, bc=(0.9, 0.05), gauss_sigma=5.0) for i, g in enumerate(GEOMETRY)])):
        recs = np.stack(recs)
        _image_check(f"{what} {shape}", _run(img, recs, False, order), _oracle(img, recs, False, order)[0], rows)
    for what, mx, share in rows:
        assert mx <= 1 and share <= 0.005, (what, mx, share)


@pytest.mark.timeout(300)
def test_noise_statistics_on_a_constant_image():
    f = np.full((1, 1, 512, 512), 100, dtype=np.uint8)
    m = _run(f, np.stack([A.record(3, 512, 512, mult=(0.5, 1.2))]), False).astype(np.float64)
    print(f"mult_noise: mean {m.mean():.4f} min {m.min()} max {m.max()}")
    assert abs(m.mean() - 85.0) <= 0.2 and m.min() >= 50 and m.max() <= 120
    g = _run(f, np.stack([A.record(3, 512, 512, gauss_sigma=10.0)]), False, A.ORDER_SIAM).astype(np.float64)
    print(f"gauss_noise: mean {g.mean():.4f} std {g.std():.4f}")
    assert abs(g.mean() - 100.0) <= 0.1 and abs(g.std() - 10.0) <= 0.1


def test_arguments_are_validated():
    t = torch.zeros(2, 1, 32, 32, dtype=torch.uint8, device="cuda")
    o = torch.zeros_like(t)
    par = torch.from_numpy(np.stack([A.record(0, 32, 32)] * 2).view(np.uint8).copy()).cuda()
    call = lambda src, dst, order, blur: lib.biu_augment_u8(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), 2, 1, 32, 32, 0,
                                                              C.c_void_p(par.data_ptr()), order, blur, 0, 0, 1, None)
    assert call(t, t, 0, 0) != 0                     # in place
    assert call(t, o, 2, 0) != 0                     # unknown stage order
    assert call(t, o, 0, 17) != 0 and b"blur" in lib.biu_last_error()
    assert call(t, o, 1, 3) != 0                     # the siam order has no blur
    aug = A.Augmenter("unet", shape=(32, 32))
    with pytest.raises(ValueError):
        aug({"image": t[:, 0]}, aug.draw(0, [0, 1]), 0, out={"image": t[:, 0]})
    with pytest.raises(ValueError):
        aug({"image": t[:, 0].float()}, aug.draw(0, [0, 1]), 0)
    torch.cuda.synchronize()


def _store(tmp_path, name, n, fields, seed=0, binary_copy=False, attrs=None):
    st = TileStore.create(str(tmp_path / name), n, fields, {"dim_out": list(next(iter(fields.values()))), **(attrs or {})})
    rng = np.random.default_rng(seed)
    for k, shp in fields.items():
        st.maps[k][:] = (rng.random((n,) + tuple(shp)) > 0.5) * 255 if k == "mask" else rng.integers(0, 256, (n,) + tuple(shp))
    if binary_copy:
        st.maps["image"][:] = st.maps["mask"][:]
    st.flush()
    return st


def _epoch(fd):
    return [{k: v.cpu().clone() for k, v in b.items()} for b in fd]


@pytest.mark.timeout(300)
def test_feeder_with_augmenter_is_reproducible(tmp_path):
    st = _store(tmp_path, "t", 12, {"image": (32, 32), "mask": (32, 32)})
    mk = lambda: A.Augmenter.from_store(st, "unet", shiftscalerotate=(0.1, 0.2, 30), seed=5)
    idx = [3, 1, 4, 11, 5, 9, 2, 6, 0, 8, 7, 10]
    fa, fb = DeviceFeeder(st, idx, 4, "cuda", depth=2, augmenter=mk()), DeviceFeeder(st, idx, 4, "cuda", depth=3, augmenter=mk())
    a0, b0 = _epoch(fa), _epoch(fb)
    assert len(a0) == 3 and fa.epoch == 1
    for x, y in zip(a0, b0):
        assert all(torch.equal(x[k], y[k]) for k in x)
    on_main = _epoch(DeviceFeeder(st, idx, 4, "cuda", augmenter=mk(), augment_stream="main"))      # the launches on the consumer's stream
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a0, on_main) for k in x)
    a1, b1 = _epoch(fa), _epoch(fb)
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a1, b1) for k in x)
    assert any(not torch.equal(x["image"], y["image"]) for x, y in zip(a0, a1))          # a fresh draw every epoch
    aug = mk()
    changed = 0
    for b, got in enumerate(a0):                                                        # == Augmenter.__call__ on the raw batch
        ids = idx[4 * b:4 * b + 4]
        raw = {k: v.cuda() for k, v in st.batch_u8(ids).items()}
        want = aug(raw, aug.draw(0, ids), 0)
        assert all(torch.equal(want[k].cpu(), got[k]) for k in got)
        changed += sum(int(not torch.equal(raw[k].cpu(), got[k])) for k in got)
        assert set(np.unique(got["mask"].numpy())) <= {0, 255}
    assert changed > 0
    # a feeder without an augmenter still hands the raw tiles over, byte for byte
    for b, got in enumerate(_epoch(DeviceFeeder(st, idx, 4, "cuda"))):
        assert all(torch.equal(st.batch_u8(idx[4 * b:4 * b + 4])[k], got[k]) for k in got)


@pytest.mark.timeout(300)
def test_every_field_of_a_sample_shares_the_geometry(tmp_path):
    st = _store(tmp_path, "g", 16, {"image": (64, 64), "mask": (64, 64)}, binary_copy=True)
    aug = A.Augmenter.from_store(st, "unet", shiftscalerotate=(0.1, 0.2, 45), seed=9, kinds={"image": "mask"})
    moved = 0
    for b, batch in enumerate(DeviceFeeder(st, list(range(16)), 4, "cuda", augmenter=aug)):
        assert torch.equal(batch["image"], batch["mask"])
        moved += int(not torch.equal(batch["mask"].cpu(), st.batch_u8(range(4 * b, 4 * b + 4))["mask"]))
    assert moved > 0


@pytest.mark.timeout(600)
def test_trainers_with_online_augmentation(tmp_path):
    cases = [(unet.Trainer, {"image": (32, 32), "mask": (32, 32)}, {}, "unet"),
             (unet3d.Trainer, {"volume": (8, 16, 16), "mask": (8, 16, 16)}, {}, "unet3d"),
             (siam.Trainer, {"image": (32, 32), "prev_image": (32, 32), "mask": (32, 32)}, {"mode": "max"}, "siam")]
    for j, (T, fields, kw, recipe) in enumerate(cases):
        st = _store(tmp_path, f"s{j}", 10, fields, seed=j, attrs={"shiftscalerotate": [0.1, 0.2, 30], "noise_amp": 10, "aug_factor": None})
        torch.manual_seed(j)
        tr = T(st, 1, batch_size=2, n_filter=4, save_dir=str(tmp_path / f"o{j}"), device="cuda", augment=True, **kw)
        assert tr.augmenter.recipe == recipe and tr.augmenter.shiftscalerotate == (0.1, 0.2, 30.0)
        assert tr.train_loader.augmenter is tr.augmenter and tr.val_loader.augmenter is None
        for b, batch in enumerate(tr.val_loader):                                      # validation sees the raw tiles
            ids = tr.val_loader.indices[2 * b:2 * b + 2]
            assert all(torch.equal(batch[k].cpu(), st.batch_u8(ids)[k]) for k in batch)
        loss = tr._forward_loss(next(iter(tr.train_loader)), validating=False)
        assert torch.isfinite(loss)
        tr.start()
        ck = torch.load(str(tmp_path / f"o{j}" / "model.pt"), weights_only=False)
        assert ck["online_augmentation"]["recipe"] == recipe and ck["online_augmentation"] == tr.augmenter.describe()
        assert torch.isfinite(torch.as_tensor(ck["best_loss"]))
        # an Augmenter instance is taken as it is
        own = A.Augmenter.from_store(st, recipe, seed=77)
        assert T(st, 1, batch_size=2, n_filter=4, save_dir=str(tmp_path / f"p{j}"), device="cuda", augment=own, **kw).augmenter is own


@pytest.mark.timeout(300)
def test_trainer_without_augment_is_unchanged(tmp_path):
    """The assertion of test_tile_store_feeder_and_trainer: fed from the store, without ``augment``, the first-step loss equals the one of
    the float data set; the checkpoint has no ``online_augmentation`` entry."""
    class U8Tiles(torch.utils.data.Dataset):
        """The reference data sets' item contract with uint8-valued tiles: float32 multiples of 1/255 in [0, 1]."""
        aug_factor, clip_threshold, noise_lims, brightness_contrast, shiftscalerotate, dim_out = 1, (0.2, 99.8), None, None, None, (32, 32)

        def __init__(self, n):
            g = torch.Generator().manual_seed(0)
            self.items = [{"image": torch.round(torch.rand(32, 32, generator=g) * 255) / 255,
                           "mask": (torch.rand(32, 32, generator=g) > 0.5).float()} for _ in range(n)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]
    ds = U8Tiles(12)
    st = TileStore.from_dataset(str(tmp_path / "tiles"), ds)
    torch.manual_seed(5)
    tr_a = unet.Trainer(ds, 1, batch_size=2, n_filter=4, save_dir=str(tmp_path / "a"), device="cuda")
    torch.manual_seed(5)
    tr_b = unet.Trainer(st, 1, batch_size=2, n_filter=4, save_dir=str(tmp_path / "b"), device="cuda")
    assert tr_b.augmenter is None and tr_b.train_loader.augmenter is None
    la = tr_a._forward_loss(next(iter(tr_a.train_loader)), validating=False)
    lb = tr_b._forward_loss(next(iter(tr_b.train_loader)), validating=False)
    assert abs(float(la) - float(lb)) < 1e-6
    tr_b.start()
    assert "online_augmentation" not in torch.load(str(tmp_path / "b" / "model.pt"), weights_only=False)
