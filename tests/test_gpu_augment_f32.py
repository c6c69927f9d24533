"""Float augmentation on the GPU: ``biu_augment_f32`` through the C ABI against the float64 oracle (``tests/augment_f32_oracle.py``), then the
feeder and ``TrainerMo2d`` that carry it.  Every test prints its figures before it asserts.

Bounds (none of them comes from what the kernel gives):

* exact cases (no-op record, quarter turns, whole-pixel shifts that wrap; all three kinds): bit for bit.
* nearest gathers: equal on every pixel whose float64 source coordinate is farther than 1e-3 from a rounding boundary; at most 1 % of a field
  may be left out (asserted first; these geometries leave out at most 0.59 %).  A VECTOR field under an arbitrary angle is gathered exactly but
  its pair is rotated in fp32: ``c cos_t + s sin_t`` with ``|c|, |s| <= 1`` is three roundings of 2^-24 (the fp32 ``cos_t`` / ``sin_t`` of the
  record, the products, the sum) on ``|c cos_t| + |s sin_t| <= sqrt(2)``: ``3 sqrt(2) 2^-24 = 2.53e-7``.
* bilinear MASK gathers, blur, Gauss noise, brightness/contrast, and the whole continuous chain: the largest deviation of the fp32 numpy
  restatement (``augment_f32_oracle`` with ``dtype=np.float32``) from the float64 oracle ON THE SAME INPUTS, computed by the test on the CPU,
  times six -- the margin ``tests/test_gpu_augment.py`` leaves over its fp32 restatement for fused multiply-adds and another operation order.
  Measured on the CPU for these inputs (``profiles/r08_augment_f32.txt``), the largest over shapes and sources: bilinear 2.98e-8, blur 1.54e-7,
  Gauss noise 2.79e-7, brightness/contrast 5.2e-8, chain 1.77e-7, i.e. bounds of at most 1.79e-7, 9.2e-7, 1.68e-6, 3.1e-7, 1.06e-6.
* shot noise: counts are discrete; no pixel may differ from the oracle by more than one count, and the share of differing pixels is capped at
  six times the share on which the fp32 restatement differs, pooled over all shapes, both source types and six noise scales (1 188 204 pixels;
  the restatement differs on 1 of them, 8.4e-7, so the cap is 5.05e-6 = 6 pixels).  Plus the distribution on constant images, ``lambda`` on
  both sides of 32: mean and variance of the counts within 5 standard errors (variance ``lambda + 1/12`` in the normal branch; its standard
  error from the Poisson fourth moment ``lambda (1 + 3 lambda)``).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd._lib import check, lib  # noqa: E402
from bio_image_unet_amd.feed import DeviceFeeder, TileStore  # noqa: E402
from tests import augment_f32_oracle as FO  # noqa: E402

SHAPES = [(1, 256, 256), (2, 96, 96), (1, 48, 80), (3, 19, 37), (1, 70, 130)]                    # [planes, H, W]
SOURCES = ["f32", "u8"]
# angle in degrees, scale, shift in pixels
GEOMETRY = [(17.3, 1, 0, 0), (151, 1.0731, 5, -3), (203.7, 0.9137, -4, 6), (359, 1.1913, 12, 12), (0, 1.0731, 3, -2), (0, 0.9137, 0, 0), (0, 1.1913, -7, 5)]
SEED, EPOCH, FID = 0x1234567890ABCDEF, 3, A.field_id("image")
KINDS = (FO.IMAGE, FO.MASK, FO.VECTOR)
VECTOR_BOUND = 3 * np.sqrt(2.0) * 2.0 ** -24
MARGIN = 6.0
ids = lambda s: s if isinstance(s, str) else "x".join(map(str, s))


def _field(shape, source, seed, lo=0.0, hi=1.0, vector=False):
    """A noise field of one sample: float32 in [lo, hi) or uint8; ``vector``: unit (cos, sin) plane pairs, twice the planes."""
    rng = np.random.default_rng(seed)
    p, h, w = shape
    if vector:
        phi = rng.uniform(0, 2 * np.pi, (p, h, w))
        f = np.stack([np.cos(phi), np.sin(phi)], axis=1).reshape(2 * p, h, w)
        return f.astype(np.float32) if source == "f32" else np.rint((f + 1) * 127.5).astype(np.uint8)
    if source == "u8":
        return rng.integers(int(lo * 255), max(int(hi * 255), 1) + 1, size=shape, dtype=np.uint8)
    return (lo + (hi - lo) * rng.random(shape)).astype(np.float32)


def _batch(shape, source, n, kind=FO.IMAGE, seed0=0, **kw):
    return np.stack([_field(shape, source, seed0 + i, vector=kind == FO.VECTOR, **kw) for i in range(n)])


def _geo(index, h, w, g, **kw):
    angle, scale, dx, dy = g
    return A.record_f32(index, h, w, angle=angle if angle else None, scale=scale if scale != 1 else None, shift=(dx, dy), **kw)


def _run(batch, recs, kind, seed=SEED, epoch=EPOCH, fid=FID):
    """``batch`` [N, P, H, W] float32 or uint8, one record per sample -> the kernel's output as a numpy array."""
    recs = np.ascontiguousarray(recs, dtype=A.PARAMS_F32_DTYPE)
    n, p, h, w = batch.shape
    src = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
    dst = torch.full(batch.shape, 7.0, dtype=torch.float32, device="cuda")
    par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    blurs = recs["blur_k"][(recs["flags"] & A.BLUR_F) != 0]
    check(lib.biu_augment_f32(C.c_void_p(src.data_ptr()), int(batch.dtype == np.uint8), C.c_void_p(dst.data_ptr()), n, p, h, w, kind,
                              C.c_void_p(par.data_ptr()), int(blurs.max()) if kind == FO.IMAGE and len(blurs) else 0, seed, epoch, fid,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream)), "augment_f32")
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _oracle(batch, recs, kind, dtype=np.float64, seed=SEED, epoch=EPOCH, fid=FID, **kw):
    outs, safes = zip(*[FO.apply(batch[i], recs[i], kind, seed, epoch, fid, dtype=dtype, **kw) for i in range(len(batch))])
    return np.stack(outs), np.stack(safes)


def _rots(h, w):
    return (0, 1, 2, 3) if h == w else (0, 2)


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_exact_cases(shape, source):
    """The no-op record, every quarter turn, whole-pixel shifts that wrap (alone and behind a quarter turn): all three kinds equal the oracle
    bit for bit, VECTOR quarter turns (sign-and-swap) included, and two launches give the same bytes; the same through the tile kernel."""
    p, h, w = shape
    rk = _rots(h, w)
    recs = [A.record_f32(0, h, w)]
    recs += [A.record_f32(i + 1, h, w, rot_k=k) for i, k in enumerate(rk)]
    recs += [A.record_f32(10 + i, h, w, rot_k=k, shift=(sx, sy)) for i, (k, sx, sy) in
             enumerate([(0, 3, 0), (0, -4, 6), (2, 5, -7), (rk[1], w // 16 + w, -h - 2), (rk[-1], -w + 1, h + 3)])]
    recs = np.stack(recs)
    for kind in KINDS:
        batch = _batch(shape, source, len(recs), kind)
        got = _run(batch, recs, kind)
        want, safe = _oracle(batch, recs, kind)
        diff = int((got.astype(np.float64) != want).sum())
        print(f"exact {shape} {source} kind {kind}: differing elements {diff}, unsafe pixels {int((~safe).sum())}")
        assert diff == 0 and safe.all()
        assert _same(got[0], FO.widen(batch[0]))                                       # nothing drawn: the sample passes unchanged
        assert _same(_run(batch, recs, kind), got)
    # VECTOR quarter turns are sign-and-swap of the gathered pair
    vec = _batch(shape, source, len(rk), FO.VECTOR, seed0=40)
    got = _run(vec, np.stack([A.record_f32(i, h, w, rot_k=k) for i, k in enumerate(rk)]), FO.VECTOR)
    for i, k in enumerate(rk):
        c, s = np.rot90(FO.widen(vec[i])[0::2], k, axes=(1, 2)), np.rot90(FO.widen(vec[i])[1::2], k, axes=(1, 2))
        wc, ws = [(c, s), (s, -c), (-c, -s), (-s, c)][k]
        assert _same(got[i][0::2], wc) and _same(got[i][1::2], ws), k
    # the same through the tile kernel: a blurring neighbour in the batch sends the whole launch there
    img = _batch(shape, source, len(recs) + 1, FO.IMAGE, seed0=20)
    tile = np.concatenate([np.stack([A.record_f32(99, h, w, blur_k=5, gauss_sigma=0.05, bc=(1.1, 0.02))]), recs])
    got = _run(img, tile, FO.IMAGE)
    want, _ = _oracle(img[1:], recs, FO.IMAGE)
    diff = int((got[1:].astype(np.float64) != want).sum())
    print(f"exact {shape} {source} through the tile kernel: differing elements {diff}")
    assert diff == 0
    assert _same(_run(img, tile, FO.IMAGE), got)
    assert not _same(_run(img, tile, FO.IMAGE, epoch=EPOCH + 1)[0], got[0])            # another epoch, another noise


@pytest.mark.timeout(600)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_nearest_gathers(shape, source):
    """IMAGE (no intensity stage), VECTOR, and MASK without rotation equal the oracle on every safe pixel; at most 1 % is left out."""
    p, h, w = shape
    for kind in KINDS:
        geos = [g for g in GEOMETRY if kind != FO.MASK or g[0] == 0]
        recs = np.stack([_geo(i, h, w, g) for i, g in enumerate(geos)])
        batch = _batch(shape, source, len(recs), kind, seed0=7)
        got = _run(batch, recs, kind)
        want, safe = _oracle(batch, recs, kind)
        for i, g in enumerate(geos):
            left_out = 1.0 - safe[i].mean()
            d = np.abs(got[i].astype(np.float64) - want[i])
            tol = VECTOR_BOUND if kind == FO.VECTOR and g[0] else 0.0
            bad = int((d > tol)[:, safe[i]].sum())
            print(f"nearest {shape} {source} kind {kind} {g}: left out {100 * left_out:.3f} %, beyond {tol:.3g} on safe pixels {bad}, "
                  f"on all pixels {int((d > tol).sum())}, max on safe {d[:, safe[i]].max():.3g}")
            assert left_out <= 0.01
            assert bad == 0


def _window_safe(safe_ext, k):
    """``safe_ext`` [H + k - 1, W + k - 1] -> [H, W]: every pixel of the k x k window is safe."""
    h, w = safe_ext.shape[0] - (k - 1), safe_ext.shape[1] - (k - 1)
    ok = np.ones((h, w), dtype=bool)
    for dy in range(k):
        for dx in range(k):
            ok &= safe_ext[dy:dy + h, dx:dx + w]
    return ok


def continuous_cases(shape):
    """(stage, kind, records, compare-where rule) of the continuous checks; shared with the script that wrote ``profiles/r08_augment_f32.txt``."""
    p, h, w = shape
    rot = [g for g in GEOMETRY if g[0]]
    return [("bilinear", FO.MASK, [_geo(i, h, w, g) for i, g in enumerate(rot)]),
            ("blur", FO.IMAGE, [A.record_f32(i, h, w, blur_k=k) for i, k in enumerate((3, 5, 7, 15))]
             + [A.record_f32(5, h, w, rot_k=2, shift=(w // 2 + 3, -5), blur_k=7), _geo(6, h, w, GEOMETRY[1], blur_k=5), _geo(7, h, w, GEOMETRY[6], blur_k=3)]),
            ("gauss_noise", FO.IMAGE, [A.record_f32(5, h, w, gauss_sigma=0.01), A.record_f32(6, h, w, gauss_sigma=0.1), A.record_f32(7, h, w, gauss_sigma=0.2)]),
            ("brightness_contrast", FO.IMAGE, [A.record_f32(0, h, w, bc=(1.1, 0.1)), A.record_f32(1, h, w, bc=(0.9, -0.1)), A.record_f32(2, h, w, bc=(1.0337, 0.0421))]),
            ("chain", FO.IMAGE, [A.record_f32(i, h, w, rot_k=_rots(h, w)[i % len(_rots(h, w))], shift=(i, -2 * i), blur_k=(3, 0, 5)[i], gauss_sigma=0.05,
                                              bc=(1.0 + 0.1 * (i - 1), 0.05 * (1 - i))) for i in range(3)])]


def compare_where(shape, recs):
    """[N, H, W] bool: the pixels a continuous case is compared on -- everywhere, except that behind a nearest gather at a non-trivial geometry
    a blurred pixel counts only when its whole k x k window was gathered away from rounding ties."""
    p, h, w = shape
    out = []
    for r in recs:
        k = int(r["blur_k"]) if int(r["flags"]) & A.BLUR_F else 1
        sx, sy = FO.source_coords(h, w, int(r["rot_k"]), float(r["angle"]), float(r["scale"]), float(r["dx"]), float(r["dy"]), halo=k // 2)
        out.append(_window_safe(FO._nearest_index(sx, sy, h, w)[2], k))
    return np.stack(out)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_bilinear_and_continuous_stages(shape, source):
    """Bilinear MASK gathers, blur, Gauss noise, brightness/contrast and a whole chain within six times the deviation of the fp32 numpy
    restatement from the float64 oracle on the same inputs (module docstring)."""
    rows = []
    for what, kind, recs in continuous_cases(shape):
        recs = np.stack(recs)
        batch = _batch(shape, source, len(recs), kind, seed0=100, lo=0.02, hi=0.98)
        want, _ = _oracle(batch, recs, kind)
        rest, _ = _oracle(batch, recs, kind, dtype=np.float32)
        where = np.broadcast_to(compare_where(shape, recs)[:, None] if kind == FO.IMAGE else np.ones((len(recs), 1) + shape[1:], dtype=bool), want.shape)
        measured = float(np.abs(rest.astype(np.float64) - want)[where].max())
        got = _run(batch, recs, kind)
        err = float(np.abs(got.astype(np.float64) - want)[where].max())
        rows.append((what, err, measured))
        print(f"continuous {what} {shape} {source}: kernel max |diff| {err:.3e}, fp32 restatement {measured:.3e}, bound {MARGIN * measured:.3e}, "
              f"compared {100 * where.mean():.2f} % of the pixels")
        assert where.mean() >= 0.8
    for what, err, measured in rows:
        assert measured > 0 and err <= MARGIN * measured, (what, err, measured)


SHOT_SCALES = (0.001, 0.002, 0.005, 0.01, 0.015, 0.02)      # lambda = v^2.2 / s with v <= 0.7: up to 456 ... 23 -- both samplers


def shot_cases():
    for shape in SHAPES:
        for source in SOURCES:
            p, h, w = shape
            recs = np.stack([A.record_f32(20 + i, h, w, shot_s=s) for i, s in enumerate(SHOT_SCALES)])
            yield shape, source, recs, _batch(shape, source, len(recs), FO.IMAGE, seed0=300, lo=0.05, hi=0.7)


def _counts(v, s):
    """The Poisson counts behind a shot-noise output (``n s < 1`` on these inputs, so the clip never bites)."""
    return np.rint(v.astype(np.float64) ** float(np.float32(2.2)) / float(np.float32(s)))


@pytest.mark.timeout(900)
def test_shot_noise_counts():
    """Counts differ from the oracle's by at most one, on at most six times the share of pixels on which the fp32 restatement differs (pooled)."""
    total = rest_diff = got_diff = 0
    worst = 0.0
    for shape, source, recs, batch in shot_cases():
        want, _ = _oracle(batch, recs, FO.IMAGE, shot_counts=True)
        rest, _ = _oracle(batch, recs, FO.IMAGE, dtype=np.float32, shot_counts=True)
        assert (want * recs["shot_s"][:, None, None, None].astype(np.float64)).max() < 1.0                  # the clip stays out of it
        got = np.stack([_counts(g, r["shot_s"]) for g, r in zip(_run(batch, recs, FO.IMAGE), recs)])
        d = np.abs(got - want)
        print(f"shot {shape} {source}: pixels {want.size}, restatement differs on {int((rest != want).sum())}, kernel on {int((d > 0).sum())}, "
              f"largest count difference {d.max():.0f}, largest count {want.max():.0f}")
        total, rest_diff, got_diff, worst = total + want.size, rest_diff + int((rest != want).sum()), got_diff + int((d > 0).sum()), max(worst, float(d.max()))
    cap = MARGIN * rest_diff / total
    print(f"shot pooled: {total} pixels, restatement share {rest_diff / total:.3e}, kernel share {got_diff / total:.3e}, cap {cap:.3e}")
    assert worst <= 1
    assert got_diff / total <= cap


@pytest.mark.timeout(600)
@pytest.mark.parametrize("lam", [5.0, 31.0, 33.0, 400.0])
def test_shot_noise_distribution_on_a_constant_image(lam):
    v = np.float32(0.5)
    lin = float(np.exp2(np.float32(2.2) * np.log2(v)))
    s = np.float32(lin / lam)
    lam = lin / float(s)                                       # what the kernel divides
    img = np.full((1, 1, 512, 512), v, dtype=np.float32)
    k = _counts(_run(img, np.stack([A.record_f32(3, 512, 512, shot_s=float(s))]), FO.IMAGE), s)
    n = k.size
    var = lam if lam < 32 else lam + 1.0 / 12.0
    se_mean, se_var = np.sqrt(var / n), np.sqrt((lam * (1 + 3 * lam) - var * var) / n)
    print(f"shot lambda {lam:.4f}: mean {k.mean():.5f} (se {se_mean:.5f}), variance {k.var():.5f} expected {var:.5f} (se {se_var:.5f}), "
          f"min {k.min():.0f} max {k.max():.0f}")
    assert abs(k.mean() - lam) <= 5 * se_mean
    assert abs(k.var() - var) <= 5 * se_var


def test_arguments_are_validated():
    t = torch.zeros(2, 2, 32, 32, dtype=torch.float32, device="cuda")
    o = torch.zeros_like(t)
    par = torch.from_numpy(np.stack([A.record_f32(0, 32, 32)] * 2).view(np.uint8).copy()).cuda()
    call = lambda src, dst, planes, kind, blur: lib.biu_augment_f32(C.c_void_p(src.data_ptr()), 0, C.c_void_p(dst.data_ptr()), 2, planes, 32, 32, kind,
                                                                    C.c_void_p(par.data_ptr()), blur, 0, 0, 1, None)
    assert call(t, t, 2, 0, 0) != 0                  # in place
    assert call(t, o, 2, 3, 0) != 0                  # unknown kind
    assert call(t, o, 1, 2, 0) != 0                  # a vector field with an odd number of planes
    assert call(t, o, 2, 0, 17) != 0 and b"blur" in lib.biu_last_error()
    assert call(t, o, 2, 2, 0) == 0
    aug = A.AugmenterF32(shape=(32, 32))
    with pytest.raises(ValueError):
        aug({"image": t}, aug.draw(0, [0, 1]), 0, out={"image": t})
    with pytest.raises(ValueError):
        aug({"image": t.half()}, aug.draw(0, [0, 1]), 0)
    with pytest.raises(ValueError):
        aug({"orientation": t[:, 0]}, aug.draw(0, [0, 1]), 0)
    torch.cuda.synchronize()


# ---- feeder ------------------------------------------------------------------------------------------------------------------------------
def _store(tmp_path, name, n, hw=(32, 32), seed=0, attrs=None):
    """A mixed store: the image as bytes, a copy of it, a mask, a distance map and an orientation pair as float32."""
    fields = {"image": hw, "copy": hw, "mask": (1,) + hw, "distance": hw, "orientation": (2,) + hw}
    st = TileStore.create(str(tmp_path / name), n, fields, {"dim_out": list(hw), **(attrs or {})},
                          dtypes={"copy": "f32", "mask": "f32", "distance": "f32", "orientation": "f32"})
    rng = np.random.default_rng(seed)
    st.maps["image"][:] = rng.integers(0, 256, (n,) + hw)
    st.maps["copy"][:] = st.maps["image"][:].astype(np.float32) / np.float32(255)
    st.maps["mask"][:] = rng.random((n, 1) + hw) > 0.5
    st.maps["distance"][:] = rng.random((n,) + hw) * 30 - 2
    phi = rng.uniform(0, 2 * np.pi, (n,) + hw)
    st.maps["orientation"][:] = np.stack([np.cos(phi), np.sin(phi)], axis=1)
    st.flush()
    return st


def _epoch(fd):
    return [{k: v.cpu().clone() for k, v in b.items()} for b in fd]


@pytest.mark.timeout(300)
def test_feeder_with_float_augmenter(tmp_path):
    st = _store(tmp_path, "t", 24)
    mk = lambda: A.AugmenterF32.from_store(st, scale_limit=(-0.1, 0.2), seed=5, kinds={"copy": "mask"})
    idx = [3, 1, 4, 11, 5, 9, 2, 6, 0, 8, 7, 10] + list(range(12, 24))
    fa, fb = DeviceFeeder(st, idx, 4, "cuda", depth=2, augmenter=mk()), DeviceFeeder(st, idx, 4, "cuda", depth=3, augmenter=mk())
    a0, b0 = _epoch(fa), _epoch(fb)
    assert len(a0) == 6 and fa.epoch == 1 and all(v.dtype == torch.float32 for v in a0[0].values())
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a0, b0) for k in x)               # same seed, same epoch: byte for byte
    on_main = _epoch(DeviceFeeder(st, idx, 4, "cuda", augmenter=mk(), augment_stream="main"))
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a0, on_main) for k in x)
    a1, b1 = _epoch(fa), _epoch(fb)
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a1, b1) for k in x)
    assert any(not torch.equal(x["image"], y["image"]) for x, y in zip(a0, a1))          # a fresh draw every epoch
    # every field of a sample shares the geometry: the MASK copy of the image, gathered nearest, is the IMAGE field before its intensity stages
    aug, rotated, plain, changed = mk(), 0, 0, 0
    for b, got in enumerate(a0):
        ids_b = idx[4 * b:4 * b + 4]
        recs = aug.draw(0, ids_b)
        raw = {k: v.cuda() for k, v in st.batch_u8(ids_b).items()}
        want = aug(raw, recs, 0)                                                        # == AugmenterF32.__call__ on the raw batch
        assert all(torch.equal(want[k].cpu(), got[k]) for k in got)
        geo = recs.copy()
        geo["flags"] &= A.ROT_F | A.SCALE_F
        before = aug({"image": raw["image"]}, geo, 0)["image"].cpu()
        for j, r in enumerate(recs):
            if int(r["flags"]) & A.ROT_F:
                rotated += 1
            else:
                plain += 1
                assert torch.equal(got["copy"][j], before[j])
        changed += int(not torch.equal(raw["distance"].cpu(), got["distance"]))
        pair = got["orientation"].double()
        assert float(((pair ** 2).sum(1) - 1).abs().max()) < 1e-6                        # a rotated unit pair stays a unit pair
        assert set(np.unique(got["mask"][torch.tensor([not int(r["flags"]) & A.ROT_F for r in recs])].numpy())) <= {0.0, 1.0}
    print(f"feeder: {rotated} samples under an arbitrary angle, {plain} without, {changed} of {len(a0)} batches changed")
    assert rotated > 0 and plain > 0 and changed > 0
    # validation batches (a feeder without an augmenter) equal the store, in the fields' own dtypes
    for b, got in enumerate(_epoch(DeviceFeeder(st, idx, 4, "cuda"))):
        raw = st.batch_u8(idx[4 * b:4 * b + 4])
        assert all(torch.equal(raw[k], got[k]) and raw[k].dtype == got[k].dtype for k in got)
    with pytest.raises(ValueError):
        DeviceFeeder(st, idx, 4, "cuda", augmenter=A.Augmenter("unet"))                 # the uint8 augmenter cannot take float fields


# ---- TrainerMo2d -------------------------------------------------------------------------------------------------------------------------
HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "distance": {"channels": 1, "activation": "relu", "loss": "WeightedDistanceGradientLoss", "weight": 0.25},
         "orientation": {"channels": 2, "activation": None, "loss": "WeightedVectorFieldLoss", "weight": 0.5}}


class _Items(torch.utils.data.Dataset):
    """The multi-output item contract: 'image' (H, W) a multiple of 1/255, one float target per head."""
    aug_factor, clip_threshold, gauss_noise_lims, shot_noise_lims, brightness_contrast, random_rotate = 1, (0., 99.98), (0.01, 0.1), (0.001, 0.01), (0.1, 0.1), True
    blur_limit, scale_limit, dim_out = (3, 5), (-0.1, 0.1), (32, 32)

    def __init__(self, n):
        g = torch.Generator().manual_seed(0)
        self.items = []
        for _ in range(n):
            phi = torch.rand((32, 32), generator=g) * 6.2831853
            on = (torch.rand((1, 32, 32), generator=g) < 0.6).float()
            self.items.append({"image": torch.round(torch.rand((32, 32), generator=g) * 255) / 255,
                               "mask": (torch.rand((1, 32, 32), generator=g) > 0.5).float(),
                               "distance": (torch.rand((32, 32), generator=g) < 0.6).float() * torch.rand((32, 32), generator=g),
                               "orientation": torch.stack([torch.cos(phi), torch.sin(phi)]) * on})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.mark.timeout(600)
def test_trainer_mo2d_with_online_augmentation(tmp_path):
    from bio_image_unet_amd.workflow import TrainerMo2d
    ds = _Items(12)
    st = TileStore.from_dataset(str(tmp_path / "mixed"), ds, dtypes={"mask": "f32", "distance": "f32", "orientation": "f32"})
    assert st.dtypes["image"] == "u8"
    torch.manual_seed(3)
    tr = TrainerMo2d(st, 2, batch_size=2, output_heads=HEADS, n_filter=8, save_dir=str(tmp_path / "o"), device="cuda", augment=True)
    assert isinstance(tr.augmenter, A.AugmenterF32) and tr.augmenter.scale_limit == (-0.1, 0.1) and tr.augmenter.gauss_noise_lims == (0.01, 0.1)
    assert tr.train_loader.augmenter is tr.augmenter and tr.val_loader.augmenter is None
    for b, batch in enumerate(tr.val_loader):                                          # validation sees the raw tiles
        raw = st.batch_u8(tr.val_loader.indices[2 * b:2 * b + 2])
        assert all(torch.equal(batch[k].cpu(), raw[k]) for k in batch)
    batch = next(iter(tr.train_loader))
    assert all(v.dtype == torch.float32 for v in batch.values())
    loss = tr._total_loss(batch, validating=False)
    print(f"TrainerMo2d(augment=True): first loss {float(loss):.6f}")
    assert torch.isfinite(loss)
    tr.start()
    ck = torch.load(str(tmp_path / "o" / "model.pt"), weights_only=False)
    print(f"TrainerMo2d(augment=True): best validation loss after two epochs {float(ck['best_loss']):.6f}")
    assert ck["online_augmentation"] == tr.augmenter.describe() and ck["online_augmentation"]["recipe"] == "mo2d"
    assert torch.isfinite(torch.as_tensor(ck["best_loss"])) and tr.train_loader.epoch == 3
    own = A.AugmenterF32.from_store(st, seed=77)
    assert TrainerMo2d(st, 1, batch_size=2, output_heads=HEADS, n_filter=8, save_dir=str(tmp_path / "p"), device="cuda", augment=own).augmenter is own
    with pytest.raises(ValueError):
        TrainerMo2d(st, 1, batch_size=2, output_heads=HEADS, n_filter=8, save_dir=str(tmp_path / "q"), device="cuda", augment=A.Augmenter("unet"))


@pytest.mark.timeout(600)
def test_trainer_mo2d_without_augment_is_unchanged(tmp_path):
    """Fed from an all-f32 store without ``augment``: the checkpoint keys and the first step's (forward-only) loss equal those of the same
    Trainer, seeded alike, fed by a ``DataLoader`` over the same float items."""
    from bio_image_unet_amd.workflow import TrainerMo2d
    ds = _Items(12)
    st = TileStore.from_dataset(str(tmp_path / "allf"), ds, dtypes="f32")
    kw = dict(batch_size=2, output_heads=HEADS, n_filter=8, device="cuda")
    torch.manual_seed(5)
    tr_a = TrainerMo2d(ds, 1, save_dir=str(tmp_path / "a"), **kw)
    torch.manual_seed(5)
    tr_b = TrainerMo2d(st, 1, save_dir=str(tmp_path / "b"), **kw)
    assert tr_b.augmenter is None and isinstance(tr_b.train_loader, DeviceFeeder) and tr_b.train_loader.augmenter is None
    la = float(tr_a._total_loss(next(iter(tr_a.train_loader)), validating=False))
    lb = float(tr_b._total_loss(next(iter(tr_b.train_loader)), validating=False))
    print(f"TrainerMo2d first-step loss: DataLoader {la!r}, float store {lb!r}")
    assert la == lb
    tr_a.start()
    tr_b.start()
    ka = set(torch.load(str(tmp_path / "a" / "model.pt"), weights_only=False))
    kb = set(torch.load(str(tmp_path / "b" / "model.pt"), weights_only=False))
    assert ka == kb and "online_augmentation" not in kb
