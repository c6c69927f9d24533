"""Crop augmentation of whole items on the GPU: ``biu_augment_f32_crop`` through the C ABI against the float64 oracle
(``tests/augment_crop_oracle.py``), then ``CropFeeder``, ``prepare`` and ``TrainerMo2d`` on an ``ImageStore``.  Every test prints its figures
before it asserts.

Shapes: items 70 x 90, 64 x 64 and 50 x 130 behind a first item in one arena (so every offset is non-zero), tiles 64 x 64 and 96 x 80 (a
partial 64 x 64 block in both axes; larger than every item in at least one axis, so every crop of it wraps), one and two planes, float32 and
uint8 arenas.

Bounds (none of them comes from what the kernel gives; they are those of ``tests/test_gpu_augment_f32.py``):

* exact cases (identity, quarter turns, whole-pixel crops that wrap; all three kinds; NaN -> ``nan_to_val`` in {0, -1}; the VECTOR pair rule):
  bit for bit.
* nearest gathers under an angle and a scale: equal on every pixel whose float64 source coordinate is farther than 1e-3 from a rounding tie;
  at most 1 % of a tile may be left out (asserted first, on the CPU).  A VECTOR pair under an arbitrary angle is rotated in fp32:
  ``3 sqrt(2) 2^-24`` (that file's reasoning: three roundings on ``|c cos_t| + |s sin_t| <= sqrt(2)``).
* bilinear MASK with NaN: the NaN decision equal wherever ``|w_nan - 0.5| > 1e-6``; values within six times the deviation of the fp32 numpy
  restatement from the float64 oracle on the same inputs; no NaN in ``dst``.  Blur, Gauss noise, brightness/contrast, a chain: the same margin.
* the equivalence law (items of the tile's extent, the same record bytes, NaN-free data in [0.05, 0.9] -> ``biu_augment_f32``'s bytes): bit for
  bit, but for the one rounding ``test_equivalence_law`` names, which is held to ``2 VECTOR_BOUND``.
* shot noise: counts differ from the oracle's by at most one, on at most six times the share of pixels on which the fp32 restatement differs,
  pooled over the cases.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd import feed  # noqa: E402
from bio_image_unet_amd._lib import lib  # noqa: E402
from tests import augment_crop_oracle as CO  # noqa: E402
from tests import augment_f32_oracle as FO  # noqa: E402

ITEMS = [(33, 47), (70, 90), (64, 64), (50, 130)]                 # the first only moves the others off offset 0
USED = (1, 2, 3)
TILES = [(64, 64), (96, 80)]
SOURCES = ["f32", "u8"]
SEED, EPOCH, FID = 0x1234567890ABCDEF, 3, A.field_id("image")
VECTOR_BOUND = 3 * np.sqrt(2.0) * 2.0 ** -24
MARGIN = 6.0
GEOMETRY = [(17.3, 1, 3, 2), (151, 1.0731, 5, 0), (203.7, 0.9137, 0, 6), (331.9, 1.1913, 12, 12), (0, 1.0731, 3, 1), (0, 0.9137, 0, 0)]   # angle, scale, ox, oy
ids = lambda s: s if isinstance(s, str) else "x".join(map(str, s))


def _nan_holes(x, rng):
    """A blob, isolated pixels, and a full row and column at the wrap seam."""
    h, w = x.shape[-2:]
    yy, xx = np.mgrid[:h, :w]
    x[..., (yy - h // 3) ** 2 + (xx - w // 2) ** 2 < 64] = np.nan
    x[..., rng.integers(0, h, 30), rng.integers(0, w, 30)] = np.nan
    x[..., h - 1, :] = np.nan
    x[..., :, 0] = np.nan
    return x


def _arena(planes, source, kind, seed=0, nan=False, lo=0.0, hi=1.0):
    """-> (arena 1-D, element offsets per item, the items ``[planes, h, w]``); ``nan``: float MASK / VECTOR items get NaN holes (a VECTOR item
    in one plane of the pair only, at different places per plane)."""
    rng = np.random.default_rng(seed)
    items = []
    for h, w in ITEMS:
        if kind == CO.VECTOR:
            phi = rng.uniform(0, 2 * np.pi, (planes // 2, h, w))
            f = np.stack([np.cos(phi), np.sin(phi)], axis=1).reshape(planes, h, w)
            f = f.astype(np.float32) if source == "f32" else np.rint((f + 1) * 127.5).astype(np.uint8)
        elif source == "u8":
            f = rng.integers(int(lo * 255), max(int(hi * 255), 1) + 1, size=(planes, h, w), dtype=np.uint8)
        else:
            f = (lo + (hi - lo) * rng.random((planes, h, w))).astype(np.float32)
        if nan and source == "f32" and kind != CO.IMAGE:
            for p in range(planes):
                _nan_holes(f[p], rng)
                f[p] = np.roll(f[p], 5 * p, axis=(0, 1))                             # other places in the second plane of a pair
        items.append(f)
    sizes = [f.size for f in items]
    return np.concatenate([f.reshape(-1) for f in items]), np.concatenate([[0], np.cumsum(sizes)[:-1]]), items


def _sources(offsets, which):
    src = np.empty(len(which), dtype=A.SOURCE_DTYPE)
    for j, i in enumerate(which):
        src[j] = (offsets[i], ITEMS[i][0], ITEMS[i][1])
    return src


def _call(arena_t, dst, n, planes, tile, kind, par, src, nan_to_val=0.0, blur=0, seed=SEED, epoch=EPOCH, fid=FID, u8=None, elems=None):
    return lib.biu_augment_f32_crop(C.c_void_p(arena_t.data_ptr()) if arena_t is not None else None, int(arena_t.dtype == torch.uint8) if u8 is None else u8,
                                    arena_t.numel() if elems is None else elems, C.c_void_p(dst.data_ptr()) if dst is not None else None, n, planes,
                                    tile[0], tile[1], kind, C.c_void_p(par.data_ptr()) if par is not None else None,
                                    C.c_void_p(src.data_ptr()) if src is not None else None, nan_to_val, blur, seed, epoch, fid,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _run(arena, offsets, which, recs, planes, tile, kind, nan_to_val=0.0, **kw):
    """Render ``len(which)`` patches ``[n, planes, th, tw]`` of the items ``which`` with one record each -> numpy."""
    recs = np.ascontiguousarray(recs, dtype=A.PARAMS_F32_DTYPE)
    assert len(recs) == len(which)
    a = torch.from_numpy(arena).cuda()
    dst = torch.full((len(which), planes) + tuple(tile), 7.0, dtype=torch.float32, device="cuda")
    par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    src = torch.from_numpy(_sources(offsets, which).view(np.uint8).copy()).cuda()
    blurs = recs["blur_k"][(recs["flags"] & A.BLUR_F) != 0]
    rc = _call(a, dst, len(which), planes, tile, kind, par, src, nan_to_val, int(blurs.max()) if kind == CO.IMAGE and len(blurs) else 0, **kw)
    assert rc == 0, lib.biu_last_error()
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _oracle(items, which, recs, tile, kind, nan_to_val=0.0, dtype=np.float64, seed=SEED, epoch=EPOCH, fid=FID, **kw):
    outs, safes = zip(*[CO.apply(items[i], r, kind, tile, nan_to_val, seed, epoch, fid, dtype=dtype, **kw) for i, r in zip(which, recs)])
    return np.stack(outs), np.stack([np.broadcast_to(s, o.shape) for s, o in zip(safes, outs)])


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _exact_records(tile):
    """Per used item: identity, the four quarter turns with an origin, whole-pixel crops whose origin lies beyond the item (they wrap)."""
    recs, which = [], []
    for i in USED:
        h, w = ITEMS[i]
        recs += [A.record_crop(len(recs), (h, w))]
        recs += [A.record_crop(10 + k, (h, w), rot_k=k, origin=(2 * k + 1, k)) for k in range(4)]
        recs += [A.record_crop(20, (h, w), origin=(w - 3, h - 2)), A.record_crop(21, (h, w), rot_k=3, origin=(w + h + 5, 3 * h + 1)),
                 A.record_crop(22, (h, w), rot_k=2, origin=(0, 2 * h))]
        which += [i] * 8
    return np.stack(recs), which


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("tile", TILES, ids=ids)
def test_exact_cases(tile, source):
    recs, which = _exact_records(tile)
    for kind, planes in ((CO.IMAGE, 1), (CO.IMAGE, 2), (CO.MASK, 1), (CO.MASK, 2), (CO.VECTOR, 2)):
        for nan_to_val in (0.0, -1.0):
            arena, off, items = _arena(planes, source, kind, seed=planes + kind, nan=True)
            got = _run(arena, off, which, recs, planes, tile, kind, nan_to_val)
            want, safe = _oracle(items, which, recs, tile, kind, nan_to_val)
            diff = int((got.astype(np.float64) != want).sum())
            holes = int((want == nan_to_val).sum()) if source == "f32" and kind != CO.IMAGE else 0
            print(f"exact {tile} {source} kind {kind} planes {planes} nan_to_val {nan_to_val}: differing {diff}, nan_to_val pixels {holes}, NaN in dst {int(np.isnan(got).sum())}")
            assert diff == 0 and safe.all() and not np.isnan(got).any()
            if source == "f32" and kind != CO.IMAGE:
                assert holes > 0
            assert _same(_run(arena, off, which, recs, planes, tile, kind, nan_to_val), got)
    # the identity record of the 64 x 64 item on the 64 x 64 tile is the item itself
    if tile == (64, 64):
        arena, off, items = _arena(1, source, CO.IMAGE, seed=9)
        got = _run(arena, off, [2], recs[:1], 1, tile, CO.IMAGE)
        assert _same(got[0], FO.widen(items[2]))
    # the VECTOR pair rule: where either plane is NaN both outputs are nan_to_val, elsewhere a quarter turn is sign-and-swap
    if source == "f32":
        arena, off, items = _arena(2, "f32", CO.VECTOR, seed=4, nan=True)
        r = np.stack([A.record_crop(0, ITEMS[2], rot_k=1)])
        got = _run(arena, off, [2], r, 2, (64, 64), CO.VECTOR, -1.0)[0]
        c, s = np.rot90(items[2][0], 1), np.rot90(items[2][1], 1)
        gone = np.isnan(c) | np.isnan(s)
        assert gone.any() and (np.isnan(c) != np.isnan(s)).any()
        assert (got[:, gone] == -1.0).all() and _same(got[0][~gone], s[~gone]) and _same(got[1][~gone], -c[~gone])
    # the same through the tile kernel: a blurring neighbour in the batch sends the whole launch there
    arena, off, items = _arena(2, source, CO.IMAGE, seed=20)
    both = np.concatenate([np.stack([A.record_crop(99, ITEMS[1], blur_k=5, gauss_sigma=0.05, bc=(1.1, 0.02))]), recs])
    got = _run(arena, off, [1] + which, both, 2, tile, CO.IMAGE)
    want, _ = _oracle(items, which, recs, tile, CO.IMAGE)
    diff = int((got[1:].astype(np.float64) != want).sum())
    print(f"exact {tile} {source} through the tile kernel: differing {diff}")
    assert diff == 0
    assert not _same(_run(arena, off, [1] + which, both, 2, tile, CO.IMAGE, epoch=EPOCH + 1)[0], got[0])       # another epoch, another noise


def _geo(index, hw, g, **kw):
    angle, scale, ox, oy = g
    return A.record_crop(index, hw, angle=angle if angle else None, scale=scale if scale != 1 else None, origin=(ox, oy), **kw)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("tile", TILES, ids=ids)
def test_nearest_gathers(tile, source):
    for kind, planes in ((CO.IMAGE, 1), (CO.VECTOR, 2), (CO.MASK, 2)):
        geos = [g for g in GEOMETRY if kind != CO.MASK or g[0] == 0]
        which = [USED[j % 3] for j in range(len(geos))] + [USED[(j + 1) % 3] for j in range(len(geos))]
        recs = np.stack([_geo(j, ITEMS[i], (geos + geos)[j]) for j, i in enumerate(which)])
        arena, off, items = _arena(planes, source, kind, seed=7, nan=True)
        want, safe = _oracle(items, which, recs, tile, kind, -1.0)
        left_out = 1.0 - safe.reshape(len(which), -1).mean(axis=1)
        print(f"nearest {tile} {source} kind {kind}: left out at most {100 * left_out.max():.3f} %")
        assert left_out.max() <= 0.01                                                # a condition on the inputs, before the GPU runs
        got = _run(arena, off, which, recs, planes, tile, kind, -1.0)
        assert not np.isnan(got).any()
        for j, g in enumerate(geos + geos):
            d = np.abs(got[j].astype(np.float64) - want[j])
            tol = VECTOR_BOUND if kind == CO.VECTOR and g[0] else 0.0
            bad = int((d > tol)[safe[j]].sum())
            print(f"nearest {tile} {source} kind {kind} item {ITEMS[which[j]]} {g}: beyond {tol:.3g} on safe pixels {bad}, on all {int((d > tol).sum())}")
            assert bad == 0


@pytest.mark.parametrize("tile", TILES, ids=ids)
def test_bilinear_mask_with_nan(tile):
    rot = [g for g in GEOMETRY if g[0]]
    which = [USED[j % 3] for j in range(len(rot))] + [USED[(j + 2) % 3] for j in range(len(rot))]
    recs = np.stack([_geo(j, ITEMS[i], (rot + rot)[j]) for j, i in enumerate(which)])
    for planes, nan_to_val in ((1, 0.0), (2, -1.0)):
        arena, off, items = _arena(planes, "f32", CO.MASK, seed=31, nan=True, lo=0.02, hi=0.98)
        want, safe = _oracle(items, which, recs, tile, CO.MASK, nan_to_val)
        rest, _ = _oracle(items, which, recs, tile, CO.MASK, nan_to_val, dtype=np.float32)
        assert safe.mean() >= 0.99
        got = _run(arena, off, which, recs, planes, tile, CO.MASK, nan_to_val)
        assert not np.isnan(got).any()
        holes_want, holes_got = want == nan_to_val, got == np.float32(nan_to_val)
        wrong = int((holes_want != holes_got)[safe].sum())
        where = safe & ~holes_want & ~holes_got
        measured = float(np.abs(rest.astype(np.float64) - want)[where].max())
        err = float(np.abs(got.astype(np.float64) - want)[where].max())
        print(f"bilinear NaN {tile} planes {planes}: left out {100 * (1 - safe.mean()):.4f} %, nan_to_val share {100 * holes_want.mean():.2f} %, wrong decisions "
              f"on safe pixels {wrong}, kernel max |diff| {err:.3e}, fp32 restatement {measured:.3e}, bound {MARGIN * measured:.3e}")
        assert holes_want.any() and wrong == 0
        assert measured > 0 and err <= MARGIN * measured
    # a uint8 arena has no NaN: the plain bilinear gather
    arena, off, items = _arena(1, "u8", CO.MASK, seed=32)
    want, _ = _oracle(items, which, recs, tile, CO.MASK)
    rest, _ = _oracle(items, which, recs, tile, CO.MASK, dtype=np.float32)
    got = _run(arena, off, which, recs, 1, tile, CO.MASK)
    measured, err = float(np.abs(rest.astype(np.float64) - want).max()), float(np.abs(got.astype(np.float64) - want).max())
    print(f"bilinear u8 {tile}: kernel max |diff| {err:.3e}, fp32 restatement {measured:.3e}")
    assert measured > 0 and err <= MARGIN * measured


def _continuous(tile):
    seam = ITEMS[3]                                                                 # 50 x 130
    return [("blur across the seam", [3, 3, 3, 1], [A.record_crop(0, seam, blur_k=5, origin=(128, 0)), A.record_crop(1, seam, rot_k=1, blur_k=5, origin=(48, 127)),
                                                     _geo(2, seam, GEOMETRY[1], blur_k=5), _geo(3, ITEMS[1], GEOMETRY[3], blur_k=3)]),
            ("gauss_noise", [1, 2, 3], [A.record_crop(5, ITEMS[1], gauss_sigma=0.01, origin=(4, 2)), A.record_crop(6, ITEMS[2], gauss_sigma=0.1),
                                        A.record_crop(7, ITEMS[3], gauss_sigma=0.2, origin=(100, 0))]),
            ("brightness_contrast", [1, 2, 3], [A.record_crop(0, ITEMS[1], bc=(1.1, 0.1)), A.record_crop(1, ITEMS[2], bc=(0.9, -0.1)),
                                                A.record_crop(2, ITEMS[3], bc=(1.0337, 0.0421))]),
            ("chain", [1, 2, 3], [A.record_crop(i, ITEMS[i + 1], rot_k=i + 1, origin=(i, 2 * i), blur_k=(3, 0, 5)[i], gauss_sigma=0.05,
                                                bc=(1.0 + 0.1 * (i - 1), 0.05 * (1 - i))) for i in range(3)])]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("tile", TILES, ids=ids)
def test_blur_and_continuous_stages(tile, source):
    rows = []
    for what, which, recs in _continuous(tile):
        recs = np.stack(recs)
        arena, off, items = _arena(2, source, CO.IMAGE, seed=100, lo=0.02, hi=0.98)
        want, _ = _oracle(items, which, recs, tile, CO.IMAGE)
        rest, _ = _oracle(items, which, recs, tile, CO.IMAGE, dtype=np.float32)
        where = np.broadcast_to(np.stack([CO.window_safe(ITEMS[i], tile, r) for i, r in zip(which, recs)])[:, None], want.shape)
        measured = float(np.abs(rest.astype(np.float64) - want)[where].max())
        got = _run(arena, off, which, recs, 2, tile, CO.IMAGE)
        err = float(np.abs(got.astype(np.float64) - want)[where].max())
        rows.append((what, err, measured))
        print(f"continuous {what} {tile} {source}: kernel max |diff| {err:.3e}, fp32 restatement {measured:.3e}, bound {MARGIN * measured:.3e}, "
              f"compared {100 * where.mean():.2f} % of the pixels")
        assert where.mean() >= 0.8
    for what, err, measured in rows:
        assert measured > 0 and err <= MARGIN * measured, (what, err, measured)


SHOT_SCALES = (0.001, 0.002, 0.005, 0.01, 0.015, 0.02)      # lambda = v^2.2 / s with v <= 0.7: up to 456 ... 23 -- both samplers


def _counts(v, s):
    return np.rint(v.astype(np.float64) ** float(np.float32(2.2)) / float(np.float32(s)))


def test_shot_noise_counts():
    total = rest_diff = got_diff = 0
    worst = 0.0
    for tile in TILES:
        for source in SOURCES:
            which = [USED[j % 3] for j in range(len(SHOT_SCALES))]
            recs = np.stack([A.record_crop(20 + j, ITEMS[i], shot_s=s, origin=(j, 2 * j)) for j, (i, s) in enumerate(zip(which, SHOT_SCALES))])
            arena, off, items = _arena(1, source, CO.IMAGE, seed=300, lo=0.05, hi=0.7)
            want, _ = _oracle(items, which, recs, tile, CO.IMAGE, shot_counts=True)
            rest, _ = _oracle(items, which, recs, tile, CO.IMAGE, dtype=np.float32, shot_counts=True)
            assert (want * recs["shot_s"][:, None, None, None].astype(np.float64)).max() < 1.0                  # the clip stays out of it
            got = np.stack([_counts(g, r["shot_s"]) for g, r in zip(_run(arena, off, which, recs, 1, tile, CO.IMAGE), recs)])
            d = np.abs(got - want)
            print(f"shot {tile} {source}: pixels {want.size}, restatement differs on {int((rest != want).sum())}, kernel on {int((d > 0).sum())}, "
                  f"largest count difference {d.max():.0f}, largest count {want.max():.0f}")
            total, rest_diff, got_diff, worst = total + want.size, rest_diff + int((rest != want).sum()), got_diff + int((d > 0).sum()), max(worst, float(d.max()))
    cap = MARGIN * rest_diff / total
    print(f"shot pooled: {total} pixels, restatement share {rest_diff / total:.3e}, kernel share {got_diff / total:.3e}, cap {cap:.3e}")
    assert worst <= 1
    assert got_diff / total <= cap


def test_noise_is_that_of_the_tile_kernel_bit_for_bit():
    """An identity crop of the 64 x 64 item through ``biu_augment_f32_crop`` and the same tile, record index, seed, epoch and field through
    ``biu_augment_f32``: the stages and the counter are one header, so the bytes are the same."""
    from bio_image_unet_amd._lib import check
    arena, off, items = _arena(1, "f32", CO.IMAGE, seed=8, lo=0.05, hi=0.9)
    for kw in (dict(shot_s=0.004), dict(gauss_sigma=0.07), dict(blur_k=3, shot_s=0.01, gauss_sigma=0.03, bc=(1.05, -0.02))):
        got = _run(arena, off, [2], np.stack([A.record_crop(41, ITEMS[2], **kw)]), 1, (64, 64), CO.IMAGE)
        rec = np.stack([A.record_f32(41, 64, 64, **kw)])
        src = torch.from_numpy(items[2][None]).cuda()
        dst = torch.empty_like(src)
        par = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        check(lib.biu_augment_f32(C.c_void_p(src.data_ptr()), 0, C.c_void_p(dst.data_ptr()), 1, 1, 64, 64, CO.IMAGE, C.c_void_p(par.data_ptr()),
                                  int(kw.get("blur_k", 0)), SEED, EPOCH, FID, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "augment_f32")
        torch.cuda.synchronize()
        assert _same(got, dst.cpu().numpy()), kw


def _law_records(h, w):
    """Every record kind of the law once; the first nine do not blur.  ``record_f32`` turns square tiles only, so the quarter turns are
    ``record_crop``'s: to either entry point a record is a map, a pair rotation and stages."""
    return np.stack([A.record_crop(0, (h, w), rot_k=1, origin=(2, 1)), A.record_f32(1, h, w, angle=33.7), A.record_f32(2, h, w, scale=1.21),
                     A.record_f32(3, h, w, shift=(w + 5, -(2 * h + 3))), A.record_f32(4, h, w, shot_s=0.004), A.record_f32(5, h, w, gauss_sigma=0.07),
                     A.record_f32(6, h, w, bc=(1.1, -0.05)), A.record_f32(7, h, w, angle=151.0, scale=0.93, shot_s=0.01, gauss_sigma=0.03, bc=(1.05, -0.02)),
                     A.record_f32(8, h, w), A.record_f32(9, h, w, angle=17.3, blur_k=3),
                     A.record_crop(10, (h, w), rot_k=3, origin=(1, 3), blur_k=A.MAX_BLUR, shot_s=0.01, gauss_sigma=0.03, bc=(0.95, 0.03))])


# (h, w), dst one float behind a 16-byte boundary: 2 x 2 blocks with partial edges on the 16-byte row path; the same on the unaligned path; the
# per-pixel path (w % 4 != 0)
LAW_CASES = [((72, 68), False), ((72, 68), True), ((40, 38), False)]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("case", LAW_CASES, ids=["rows", "rows-offset-dst", "pixels"])
@pytest.mark.parametrize("kind", [CO.IMAGE, CO.MASK, CO.VECTOR], ids=["image", "mask", "vector"])
def test_equivalence_law(kind, case, source):
    """include/biu.h: items whose extent is the tile's, the same record bytes, NaN-free data -> the bytes of ``biu_augment_f32``.

    One restriction, found when the two sources still had a kernel file each and kept since: ``biu_augment_f32`` rotates a VECTOR pair with
    the ``cos_t`` product fused into the sum where a lane stores four pixels of a row (``w % 4 == 0`` and an aligned ``dst``), and with both
    products rounded everywhere else, as ``biu_augment_f32_crop`` does on every path.  So on the row path the records with an arbitrary angle
    (``cos_t``, ``sin_t`` not in {0, 1, -1}) are held to ``2 VECTOR_BOUND`` (each side is within ``VECTOR_BOUND`` of the exact pair) instead
    of to equality; every other record, kind and path is bit for bit."""
    from bio_image_unet_amd._lib import check
    (h, w), offset_dst = case
    recs = _law_records(h, w)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for these in (recs[:9], recs):                                  # without a blurring sample: the point kernels; with: the tile kernels
        n = len(these)
        rng = np.random.default_rng(8)
        batch = rng.integers(13, 230, size=(n, 2, h, w), dtype=np.uint8) if source == "u8" else (0.05 + 0.85 * rng.random((n, 2, h, w))).astype(np.float32)
        blur = int(these["blur_k"].max()) if kind == CO.IMAGE else 0
        par = torch.from_numpy(these.view(np.uint8).copy()).cuda()
        src = torch.from_numpy(batch).cuda()
        arena = torch.cat([src.new_zeros(8), src.reshape(-1)])      # the items behind 8 elements, so that no offset is 0
        sources = np.empty(n, dtype=A.SOURCE_DTYPE)
        for j in range(n):
            sources[j] = (8 + j * 2 * h * w, h, w)
        sources = torch.from_numpy(sources.view(np.uint8).copy()).cuda()
        outs = []
        for crop in (False, True):
            whole = torch.full((n * 2 * h * w + 4,), 7.0, dtype=torch.float32, device="cuda")
            dst = whole[1:1 + n * 2 * h * w] if offset_dst else whole[:n * 2 * h * w]
            assert (dst.data_ptr() % 16 == 4) == offset_dst
            if crop:
                check(lib.biu_augment_f32_crop(C.c_void_p(arena.data_ptr()), int(source == "u8"), arena.numel(), C.c_void_p(dst.data_ptr()), n, 2, h, w, kind,
                                               C.c_void_p(par.data_ptr()), C.c_void_p(sources.data_ptr()), 0.0, blur, SEED, EPOCH, FID, stream()), "augment_f32_crop")
            else:
                check(lib.biu_augment_f32(C.c_void_p(src.data_ptr()), int(source == "u8"), C.c_void_p(dst.data_ptr()), n, 2, h, w, kind,
                                          C.c_void_p(par.data_ptr()), blur, SEED, EPOCH, FID, stream()), "augment_f32")
            torch.cuda.synchronize()
            outs.append(dst.view(n, 2, h, w).cpu().numpy())
            assert bool((whole[1 + n * 2 * h * w:] == 7.0).all())
        want, got = outs
        fused = kind == CO.VECTOR and w % 4 == 0 and not offset_dst
        ok = []
        for j, r in enumerate(these):
            if fused and r["flags"] & A.ROT_F:
                d = float(np.abs(got[j].astype(np.float64) - want[j]).max())
                print(f"equivalence kind {kind} {h} x {w} {source} record {j}: fused against rounded rotation, max |diff| {d:.3e}, bound {2 * VECTOR_BOUND:.3e}")
                ok.append(d <= 2 * VECTOR_BOUND)
            else:
                ok.append(_same(got[j], want[j]))
        print(f"equivalence kind {kind} {h} x {w} offset dst {offset_dst} {source} max blur {blur}: {sum(ok)} of {len(ok)} records hold")
        assert all(ok)
        assert not _same(got[0], got[8]) and not np.isnan(got).any()            # the records really do different things


def test_argument_errors_launch_nothing():
    arena, off, items = _arena(2, "f32", CO.IMAGE)
    a = torch.from_numpy(arena).cuda()
    whole = torch.full((2 * 2 * 64 * 64 + 1,), 7.0, dtype=torch.float32, device="cuda")
    dst = whole[:2 * 2 * 64 * 64]
    par = torch.from_numpy(np.stack([A.record_crop(0, ITEMS[1]), A.record_crop(1, ITEMS[2])]).view(np.uint8).copy()).cuda()
    src = torch.from_numpy(_sources(off, [1, 2]).view(np.uint8).copy()).cuda()
    t = (64, 64)
    bad = [("null arena", _call(None, dst, 2, 2, t, 0, par, src, u8=0, elems=10)), ("null dst", _call(a, None, 2, 2, t, 0, par, src)),
           ("null records", _call(a, dst, 2, 2, t, 0, None, src)), ("null sources", _call(a, dst, 2, 2, t, 0, par, None)),
           ("dst inside the arena", _call(a, a[8:], 2, 2, t, 0, par, src)), ("dst over the records", _call(a, par.view(torch.float32), 2, 2, (1, 1), 0, par, src)),
           ("unaligned dst", _call(a, whole.view(torch.uint8)[2:], 2, 2, t, 0, par, src)),
           ("unaligned arena", _call(a.view(torch.uint8)[1:], dst, 2, 2, t, 0, par, src, u8=0, elems=100)),
           ("n = 0", _call(a, dst, 0, 2, t, 0, par, src)), ("planes = 0", _call(a, dst, 2, 0, t, 0, par, src)), ("th = 0", _call(a, dst, 2, 2, (0, 64), 0, par, src)),
           ("tw < 0", _call(a, dst, 2, 2, (64, -1), 0, par, src)), ("empty arena", _call(a, dst, 2, 2, t, 0, par, src, elems=0)),
           ("unknown kind", _call(a, dst, 2, 2, t, 3, par, src)), ("odd vector planes", _call(a, dst, 2, 1, t, 2, par, src)),
           ("blur 17", _call(a, dst, 2, 2, t, 0, par, src, blur=17)), ("field_id 2^28", _call(a, dst, 2, 2, t, 0, par, src, fid=1 << 28)),
           ("2^31 elements", _call(a, dst, 2, 2, (32768, 16384), 0, par, src)), ("NaN nan_to_val", _call(a, dst, 2, 2, t, 1, par, src, nan_to_val=float("nan")))]
    torch.cuda.synchronize()
    for what, rc in bad:
        print(f"{what}: status {rc}")
    assert all(rc != 0 for _, rc in bad)
    assert bool((whole == 7.0).all())                                               # the canary: nothing was launched
    # a source that does not lie inside the arena is rendered as nan_to_val and nothing outside the arena is read
    out = torch.from_numpy(np.array([(a.numel() - 10, 64, 64), (off[2], 64, 64)], dtype=A.SOURCE_DTYPE).view(np.uint8).copy()).cuda()
    assert _call(a, dst, 2, 2, t, 0, par, out, nan_to_val=-3.0) == 0
    torch.cuda.synchronize()
    got = dst.view(2, 2, 64, 64).cpu().numpy()
    assert (got[0] == -3.0).all() and _same(got[1], items[2]) and float(whole[-1]) == 7.0


# ---- feeder, prepare, Trainer -----------------------------------------------------------------------------------------------------------
HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "distance": {"channels": 1, "activation": "relu", "loss": "WeightedDistanceGradientLoss", "weight": 0.25},
         "orientation": {"channels": 2, "activation": None, "loss": "WeightedVectorFieldLoss", "weight": 0.5}}


def _raw(seed=0, sizes=((70, 90), (64, 64), (50, 130))):
    rng = np.random.default_rng(seed)
    images = [rng.integers(100, 4000, hw).astype(np.uint16) for hw in sizes]
    mask = [_nan_holes((rng.random(hw) > 0.5).astype(np.float32), rng) for hw in sizes]
    distance = [(rng.random(hw) * 5).astype(np.float64) for hw in sizes]
    orientation = [_nan_holes(rng.uniform(0, 2 * np.pi, hw), rng) for hw in sizes]
    return images, {"mask": mask, "distance": distance, "orientation": orientation}


def _epoch(fd):
    return [{k: v.cpu().clone() for k, v in b.items()} for b in fd]


def test_crop_feeder_and_prepare(tmp_path):
    from bio_image_unet_amd import multi_output_unet as M
    from bio_image_unet_amd.preprocess import DeviceFrontEnd
    images, targets = _raw()
    st = M.prepare(images, targets, str(tmp_path / "s"), dim_out=(64, 64), nan_to_val=-1, scale_limit=(-0.2, 0.3), clip_threshold=(0., 99.98), device="cuda")
    assert isinstance(st, feed.ImageStore) and st.fields == {"image": (64, 64), "mask": (64, 64), "distance": (64, 64), "orientation": (2, 64, 64)}
    assert len(st) == sum(max(int(h * w / 4096 * 2), 2) for h, w in st.sizes) and st.nan_to_val == -1.0
    # the image is what PredictMo2d(preprocess="device") feeds its network for the same array and keywords: the same front-end calls
    for i, img in enumerate(images):
        fe = DeviceFrontEnd(img[None], "cuda")
        fe.normalise("single", (0., 99.98))
        want = fe.tiles([(0, 0, 0, 0)], (1,) + img.shape, out="float32").batch(0, 1)[0].cpu().numpy()
        assert _same(np.asarray(st.item(i, "image")), want) and 0.0 <= want.min() and want.max() == 1.0
        phi = targets["orientation"][i].astype(np.float32)
        assert np.asarray(st.item(i, "orientation")).tobytes() == np.stack([np.cos(phi), np.sin(phi)]).tobytes()
        assert np.isnan(st.item(i, "mask")).any() and np.array_equal(np.isnan(st.item(i, "orientation")[0]), np.isnan(st.item(i, "orientation")[1]))
    mk = lambda: A.AugmenterF32.from_store(st, seed=5)
    idx = list(np.random.default_rng(0).permutation(len(st)))
    fa, fb = feed.CropFeeder(st, idx, 2, "cuda", mk(), depth=2), feed.CropFeeder(st, idx, 2, "cuda", mk(), epoch_key=0)
    a0, b0, a1 = _epoch(fa), _epoch(fb), _epoch(fa)
    assert len(a0) == len(idx) // 2 and all(v.dtype == torch.float32 and not torch.isnan(v).any() for b in a0 for v in b.values())
    assert a0[0]["image"].shape == (2, 64, 64) and a0[0]["orientation"].shape == (2, 2, 64, 64)
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a0, b0) for k in x)             # the same key: the same bits
    assert any(not torch.equal(x["image"], y["image"]) for x, y in zip(a0, a1))        # another key: other crops
    assert all(torch.equal(x[k], y[k]) for x, y in zip(b0, _epoch(fb)) for k in x)     # a fixed key: the same every epoch
    assert any(bool((b["mask"] == -1.0).any()) for b in a0)
    # a batch equals the oracle's rendering of the same records
    recs, _ = mk().draw_crops(0, idx[:2], st)
    for j, r in enumerate(recs):
        item = np.asarray(st.item(st.locate(int(idx[j])), "mask"))
        want, safe = CO.apply(item, r, CO.MASK, (64, 64), -1.0, 5, 0, A.field_id("mask"))
        if not int(r["flags"]) & A.ROT_F:
            assert np.array_equal(a0[0]["mask"][j].numpy().astype(np.float64)[safe], want[0][safe])
    with pytest.raises(NotImplementedError, match="cubic"):
        feed.CropFeeder(st, idx, 2, "cuda", A.AugmenterF32.from_store(st, target_interp="cubic"))
    with pytest.raises(ValueError):
        feed.CropFeeder(st, idx, 2, "cuda", None)
    u8 = M.prepare(images, targets, str(tmp_path / "u"), dim_out=(64, 64), clip_threshold=(0., 99.98), image_dtype="u8", device="cuda")
    assert u8.dtypes["image"] == "u8" and np.abs(np.asarray(u8.item(0, "image")) / 255.0 - np.asarray(st.item(0, "image"))).max() <= 1 / 255.0
    assert next(iter(feed.CropFeeder(u8, idx, 2, "cuda", A.AugmenterF32.from_store(u8, seed=5))))["image"].dtype == torch.float32


def test_trainer_mo2d_on_an_image_store(tmp_path):
    from bio_image_unet_amd import multi_output_unet as M
    images, targets = _raw(1)
    st = M.prepare(images, targets, str(tmp_path / "s"), dim_out=(64, 64), nan_to_val=0, aug_factor=6, scale_limit=(-0.1, 0.1), device="cuda")
    assert len(st) == 24                                                            # 9 + 6 + 9 patches: 20 to train on, 4 to validate on
    torch.manual_seed(3)
    tr = M.Trainer(st, 1, batch_size=2, output_heads=HEADS, n_filter=8, save_dir=str(tmp_path / "o"), device="cuda")
    assert isinstance(tr.augmenter, A.AugmenterF32) and tr.augmenter.scale_limit == (-0.1, 0.1)
    assert isinstance(tr.train_loader, feed.CropFeeder) and isinstance(tr.val_loader, feed.CropFeeder)
    assert tr.val_loader.epoch_key == A.VALIDATION_EPOCH and tr.train_loader.epoch_key is None and tr.params["augmentation"] == 6
    assert len(tr.train_loader.indices) + len(tr.val_loader.indices) == len(st) and len(tr.val_loader) >= 1
    v0, v1 = _epoch(tr.val_loader), _epoch(tr.val_loader)
    assert all(torch.equal(x[k], y[k]) for x, y in zip(v0, v1) for k in x)             # validation patches: augmented, but fixed
    tr.start()
    ck = torch.load(str(tmp_path / "o" / "model.pt"), weights_only=False)
    print(f"TrainerMo2d on an ImageStore: validation loss after one epoch {float(ck['best_loss']):.6f}")
    assert torch.isfinite(torch.as_tensor(ck["best_loss"])) and ck["online_augmentation"]["recipe"] == "mo2d" and tr.train_loader.epoch == 1
    with pytest.raises(ValueError):
        M.Trainer(st, 1, batch_size=2, output_heads=HEADS, n_filter=8, save_dir=str(tmp_path / "q"), device="cuda", augment=False)
