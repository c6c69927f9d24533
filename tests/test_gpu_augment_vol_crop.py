"""Whole-volume crop augmentation on the GPU: ``biu_augment_vol_f32_crop`` through the C ABI against the float64 oracle
(``tests/augment_vol_crop_oracle.py``: transform the whole plane, slice, then the stages on the slice), against ``biu_augment_vol_f32`` where the
contract says the two agree bit for bit, then ``multi_output_unet3d.prepare``, the feeder and ``TrainerMo3d`` on a ``feed.VolumeStore``.
Every test prints its figures before it asserts.

Items ``[D, H, W]``: ``(3, 20, 24)`` (only moves the others off offset 0), ``(7, 70, 90)``, ``(6, 64, 64)``, ``(9, 80, 130)``, in ONE arena.  Tiles:
``(4, 64, 64)`` (16-byte stores, one 64-tile), ``(3, 50, 61)`` (odd rows, a partial tile), ``(2, 70, 84)`` (crosses the 64-tile edge in both axes
with a halo of 7).  Each tile is rendered only from the items that hold it, at the origin ``(0, 0)``, the far corner and an interior place, with
``z0`` 0, ``D - td`` and one between.

Bounds are ``tests/test_gpu_augment_vol.py``'s; none comes from the kernel under test:

* exact cases (pure crops, brightness/contrast alone, NaN -> ``nan_to_val``) and the equivalence law: bit for bit.
* nearest gathers: equal to the oracle on every voxel whose float64 source coordinate is farther than 1e-3 from a rounding tie, at most 1 % left
  out (asserted first, on the CPU); VECTOR under an angle within ``3 sqrt(2) 2^-24`` (three fp32 roundings on ``|c cos| + |s sin| <= sqrt 2``).
* bilinear gather and continuous stages, on all voxels: six times the largest deviation of the fp32 numpy restatement from the float64 oracle on
  the same inputs (which must be above 0).
* shot noise: counts within one of the oracle's; the differing share at most six times the restatement's share, pooled.
* chunks of planes: the chunk the library reports is asserted; noise-free output equals the same planes rendered alone, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd import feed  # noqa: E402
from bio_image_unet_amd._lib import check, lib  # noqa: E402
from tests import augment_vol_crop_oracle as CO  # noqa: E402

ITEMS = [(3, 20, 24), (7, 70, 90), (6, 64, 64), (9, 80, 130)]
TILES = [(4, 64, 64), (3, 50, 61), (2, 70, 84)]
SOURCES = ["f32", "u8"]
BORDERS = [CO.REFLECT, CO.CONSTANT]
GEOMETRY = [(17.3, 1), (151, 0.7313), (203.7, 0.4137), (359, 0.2913), (77.7, 0.5519), (0, 0.6137), (0, 0.9137), (0, 0.3371)]   # test_gpu_augment_vol.py's
SEED, EPOCH, FID = 0x1234567890ABCDEF, 3, A.field_id("volume")
VECTOR_BOUND = 3 * np.sqrt(2.0) * 2.0 ** -24
MARGIN = 6.0
ids = lambda s: s if isinstance(s, str) else ("reflect", "constant")[s] if isinstance(s, int) else "x".join(map(str, s))


def everything(fn):
    """All tiles x both borders x both source types."""
    fn = pytest.mark.parametrize("source", SOURCES)(fn)
    fn = pytest.mark.parametrize("border", BORDERS, ids=ids)(fn)
    return pytest.mark.parametrize("tile", TILES, ids=ids)(fn)


def holders(tile):
    """The items that hold the tile."""
    return [i for i, it in enumerate(ITEMS) if i and all(e >= t for e, t in zip(it, tile))]


def placements(item, tile):
    """(z0, oy, ox): the origin, the far corner, an interior place."""
    (d, h, w), (td, th, tw) = item, tile
    return [(0, 0, 0), (d - td, h - th, w - tw), ((d - td + 1) // 2, (h - th) // 2, (w - tw) // 3)]


def cases(tile):
    """Every (item, z0, oy, ox) the tile is rendered at."""
    return [(i,) + p for i in holders(tile) for p in placements(ITEMS[i], tile)]


def _nan_holes(x, rng):
    """A blob, isolated voxels, and a whole last row and first column, in every plane of ``x [..., H, W]``."""
    h, w = x.shape[-2:]
    yy, xx = np.mgrid[:h, :w]
    x[..., (yy - h // 3) ** 2 + (xx - w // 2) ** 2 < 64] = np.nan
    x[..., rng.integers(0, h, 30), rng.integers(0, w, 30)] = np.nan
    x[..., h - 1, :] = np.nan
    x[..., :, 0] = np.nan
    return x


def _arena(channels, source, kind, seed=0, nan=False, lo=0.0, hi=1.0):
    """-> (arena 1-D, element offsets per item, the items ``[channels, D, H, W]``); ``nan``: float MASK / VECTOR items get NaN holes (a VECTOR item
    in ONE plane of the pair at a place: the cos plane's holes and the sin plane's are elsewhere)."""
    rng = np.random.default_rng(seed)
    items = []
    for d, h, w in ITEMS:
        if kind == CO.VECTOR:
            phi = rng.uniform(0, 2 * np.pi, (channels // 2, d, h, w))
            f = np.stack([np.cos(phi), np.sin(phi)], axis=1).reshape(channels, d, h, w)
            f = f.astype(np.float32) if source == "f32" else np.rint((f + 1) * 127.5).astype(np.uint8)
            if nan and source == "f32":
                f[0::2, :, h // 4:h // 4 + 5, :] = np.nan
                f[1::2, :, :, w // 2:w // 2 + 3] = np.nan
        elif source == "u8":
            f = rng.integers(int(lo * 255), max(int(hi * 255), 1) + 1, size=(channels, d, h, w), dtype=np.uint8)
        else:
            f = (lo + (hi - lo) * rng.random((channels, d, h, w))).astype(np.float32)
            if nan:
                f = _nan_holes(f, rng)
        items.append(f)
    sizes = [f.size for f in items]
    return np.concatenate([f.reshape(-1) for f in items]), np.concatenate([[0], np.cumsum(sizes)[:-1]]), items


def _sources(offsets, which, z0s):
    src = np.empty(len(which), dtype=A.SOURCE_VOL_DTYPE)
    for j, (i, z0) in enumerate(zip(which, z0s)):
        src[j] = (offsets[i],) + ITEMS[i] + (z0,)
    return src


def _call(arena_t, dst, n, channels, tile, kind, border, par, src, nan_to_val=0.0, blur=0, seed=SEED, epoch=EPOCH, fid=FID, u8=None, elems=None):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return lib.biu_augment_vol_f32_crop(p(arena_t), int(arena_t.dtype == torch.uint8) if u8 is None else u8, arena_t.numel() if elems is None else elems,
                                        p(dst), n, channels, tile[0], tile[1], tile[2], kind, border, p(par), p(src), nan_to_val, blur, seed, epoch, fid,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _max_blur(recs, kind):
    blurs = recs["blur_k"][(recs["flags"] & A.BLUR_F) != 0]
    return int(blurs.max()) if kind == CO.IMAGE and len(blurs) else 0


def _run(arena, off, which, z0s, recs, channels, tile, kind, border, nan_to_val=0.0):
    recs = np.ascontiguousarray(recs, dtype=A.PARAMS_F32_DTYPE)
    a = torch.from_numpy(arena).cuda()
    dst = torch.full((len(which), channels) + tuple(tile), 7.0, dtype=torch.float32, device="cuda")
    check(_call(a, dst, len(which), channels, tile, kind, border, _bytes(recs), _bytes(_sources(off, which, z0s)), nan_to_val, _max_blur(recs, kind)),
          "augment_vol_f32_crop")
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _oracle(items, which, z0s, recs, tile, kind, border, nan_to_val=0.0, dtype=np.float64, **kw):
    outs, safes = zip(*[CO.apply(items[i], r, z0, tile, kind, border, nan_to_val, SEED, EPOCH, FID, dtype=dtype, **kw) for i, z0, r in zip(which, z0s, recs)])
    return np.stack(outs), np.stack(safes)


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _crop(f, z0, oy, ox, tile):
    return f[:, z0:z0 + tile[0], oy:oy + tile[1], ox:ox + tile[2]]


def _rec(j, i, g=(0, 1), origin=(0, 0), **kw):
    """Record ``j`` for a crop out of item ``i`` under geometry ``g = (angle, scale)``."""
    return A.record_vol_crop(j, ITEMS[i][1:], angle=g[0] if g[0] else None, scale=g[1] if g[1] != 1 else None, origin=origin, **kw)


# ---- 1. exact cases ------------------------------------------------------------------------------------------------------------------------
@everything
def test_exact_cases(tile, source, border):
    """The empty record at every origin and z0 is a pure crop; brightness/contrast alone is the fp32 formula; NaN gives ``nan_to_val``; the VECTOR
    pair rule; ``dst`` holds no NaN; a second run gives the same bits.  One- and two-channel fields, point and tile kernel."""
    cs = cases(tile)
    which, z0s = [c[0] for c in cs], [c[1] for c in cs]
    recs = np.stack([_rec(j, i, origin=(ox, oy)) for j, (i, _, oy, ox) in enumerate(cs)])
    for kind, channels in ((CO.IMAGE, 1), (CO.IMAGE, 2), (CO.MASK, 2), (CO.VECTOR, 2)):
        arena, off, items = _arena(channels, source, kind, seed=1)
        got = _run(arena, off, which, z0s, recs, channels, tile, kind, border)
        ok = [_same(got[j], _crop(CO.widen(items[i]), z0, oy, ox, tile)) for j, (i, z0, oy, ox) in enumerate(cs)]
        print(f"pure crop {tile} {source} border {border} kind {kind} channels {channels}: {sum(ok)} of {len(ok)} placements equal")
        assert all(ok)
        assert _same(_run(arena, off, which, z0s, recs, channels, tile, kind, border), got)
    # brightness/contrast alone, through the point kernel and, with a blurring neighbour in the batch, through the tile kernel
    bcs = [(1.1, 0.1), (0.9, -0.1), (1.0337, 0.0421), (1.3, 0.2)]
    arena, off, items = _arena(2, source, CO.IMAGE, seed=20)
    sel = [cs[j % len(cs)] for j in range(len(bcs))]
    brecs = np.stack([_rec(j, c[0], origin=(c[3], c[2]), bc=bc) for j, (c, bc) in enumerate(zip(sel, bcs))])
    want = [np.clip(_crop(CO.widen(items[c[0]]), c[1], c[2], c[3], tile) * np.float32(a) + np.float32(b), np.float32(0), np.float32(1)) for c, (a, b) in zip(sel, bcs)]
    got = _run(arena, off, [c[0] for c in sel], [c[1] for c in sel], brecs, 2, tile, CO.IMAGE, border)
    blurring = np.stack([_rec(99, sel[0][0], blur_k=5, gauss_sigma=0.05, bc=(1.1, 0.02))])
    tiled = _run(arena, off, [sel[0][0]] + [c[0] for c in sel], [0] + [c[1] for c in sel], np.concatenate([blurring, brecs]), 2, tile, CO.IMAGE, border)
    for j in range(len(bcs)):
        a, b = _same(got[j], want[j]), _same(tiled[j + 1], want[j])
        print(f"bc alone {tile} {source} border {border} record {j}: point kernel {'equal' if a else 'DIFFERENT'}, tile kernel {'equal' if b else 'DIFFERENT'}")
        assert a and b
    if source == "u8":
        return                                                      # bytes hold no NaN
    for ntv in (0.0, -1.0):
        arena, off, items = _arena(2, source, CO.MASK, seed=2, nan=True)
        got = _run(arena, off, which, z0s, recs, 2, tile, CO.MASK, border, ntv)
        crops = [_crop(items[i], z0, oy, ox, tile) for i, z0, oy, ox in cs]
        ok = [_same(got[j], np.where(np.isnan(c), np.float32(ntv), c)) for j, c in enumerate(crops)]
        holes = sum(int(np.isnan(c).sum()) for c in crops)
        print(f"NaN mask {tile} border {border} nan_to_val {ntv}: {sum(ok)} of {len(ok)} equal, {holes} NaN voxels, NaN in dst {int(np.isnan(got).sum())}")
        assert all(ok) and holes > 0 and not np.isnan(got).any()
        arena, off, items = _arena(2, source, CO.VECTOR, seed=3, nan=True)
        got = _run(arena, off, which, z0s, recs, 2, tile, CO.VECTOR, border, ntv)
        one_only = 0
        for j, (i, z0, oy, ox) in enumerate(cs):
            c = _crop(items[i], z0, oy, ox, tile)
            none = np.isnan(c[0]) | np.isnan(c[1])
            one_only += int((np.isnan(c[0]) != np.isnan(c[1])).sum())
            assert _same(got[j], np.where(none[None], np.float32(ntv), c)), (j, ntv)
        print(f"NaN pair {tile} border {border} nan_to_val {ntv}: voxels with NaN in one plane only {one_only}, NaN in dst {int(np.isnan(got).sum())}")
        assert one_only > 0 and not np.isnan(got).any()


# ---- 2. the equivalence law ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("border", BORDERS, ids=ids)
@pytest.mark.parametrize("kind", [CO.IMAGE, CO.MASK, CO.VECTOR], ids=["image", "mask", "vector"])
def test_equivalence_law(kind, border, source):
    """Item ``(6, 64, 64)``, tile ``(6, 64, 64)``, ``z0 = 0``, origin 0: the bytes of ``biu_augment_vol_f32`` for the same records."""
    tile, i = ITEMS[2], 2
    recs = np.stack([_rec(0, i, GEOMETRY[1]), _rec(1, i, GEOMETRY[2], bc=(1.1, -0.05)), _rec(2, i, GEOMETRY[0], shot_s=0.004), _rec(3, i, gauss_sigma=0.07),
                     _rec(4, i, GEOMETRY[4], blur_k=7), _rec(5, i, GEOMETRY[3], blur_k=3, shot_s=0.01, gauss_sigma=0.03, bc=(1.05, -0.02)), _rec(6, i)])
    for these in (recs[[0, 1, 2, 3, 6]], recs):                     # without a blurring sample: the point kernels; with: the tile kernels
        arena, off, items = _arena(2, source, kind, seed=8, lo=0.05, hi=0.9)
        got = _run(arena, off, [i] * len(these), [0] * len(these), these, 2, tile, kind, border)
        src = torch.from_numpy(np.stack([items[i]] * len(these))).cuda()
        dst = torch.empty(src.shape, dtype=torch.float32, device="cuda")
        check(lib.biu_augment_vol_f32(C.c_void_p(src.data_ptr()), int(source == "u8"), C.c_void_p(dst.data_ptr()), len(these), 2, *tile, kind, border,
                                      C.c_void_p(_bytes(these).data_ptr()), _max_blur(these, kind), SEED, EPOCH, FID,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "augment_vol_f32")
        torch.cuda.synchronize()
        want = dst.cpu().numpy()
        ok = [_same(got[j], want[j]) for j in range(len(these))]
        print(f"equivalence kind {kind} border {border} {source} max blur {_max_blur(these, kind)}: {sum(ok)} of {len(ok)} records equal")
        assert all(ok)
        assert not _same(got[0], got[-1])                           # the records really do different things


# ---- 3. nearest gathers --------------------------------------------------------------------------------------------------------------------
def _geo_cases(tile, **kw):
    """Every geometry at a placement of its own, cycling through the items and placements of the tile."""
    cs = cases(tile)
    sel = [cs[(2 * j + j // len(cs)) % len(cs)] for j in range(len(GEOMETRY))]
    recs = np.stack([_rec(j, c[0], g, origin=(c[3], c[2]), **{k: v(j) for k, v in kw.items()}) for j, (c, g) in enumerate(zip(sel, GEOMETRY))])
    return [c[0] for c in sel], [c[1] for c in sel], recs


@everything
def test_nearest_gathers(tile, source, border):
    which, z0s, recs = _geo_cases(tile)
    for kind, channels in ((CO.MASK, 1), (CO.MASK, 2), (CO.VECTOR, 2)):
        arena, off, items = _arena(channels, source, kind, seed=7, nan=True)
        want, safe = _oracle(items, which, z0s, recs, tile, kind, border, -1.0)
        left_out = [1.0 - s.mean() for s in safe]
        print(f"nearest {tile} {source} border {border} kind {kind}: left out at most {100 * max(left_out):.3f} %")
        assert max(left_out) <= 0.01                                # on the CPU, before the kernel runs
        got = _run(arena, off, which, z0s, recs, channels, tile, kind, border, -1.0)
        tol = VECTOR_BOUND if kind == CO.VECTOR else 0.0
        for j, g in enumerate(GEOMETRY):
            d = np.abs(got[j].astype(np.float64) - want[j])
            bad = int((d > tol)[..., safe[j]].sum())
            print(f"nearest {tile} {source} border {border} kind {kind} channels {channels} {g} item {which[j]} z0 {z0s[j]} origin {CO.origin(recs[j])}: "
                  f"beyond {tol:.3g} on safe voxels {bad}, on all {int((d > tol).sum())}")
            assert bad == 0
        assert not np.isnan(got).any()


# ---- 4. the bilinear image and the continuous stages ---------------------------------------------------------------------------------------
def continuous_cases(tile):
    """(stage, item per record, z0 per record, records), all IMAGE.  The blur cases include crops at the far corner."""
    cs = cases(tile)
    far = [c for c in cs if c[1:] == placements(ITEMS[c[0]], tile)[1]]
    at = lambda c, j, g=(0, 1), **kw: _rec(j, c[0], g, origin=(c[3], c[2]), **kw)
    rot = [g for g in GEOMETRY if g[0]]
    pick = lambda j: cs[(2 * j + 1) % len(cs)]
    out = [("gather",) + _geo_cases(tile)]
    for what, sel, recs in (
            ("brightness_contrast", [pick(0), pick(1), pick(2)], lambda s: [at(s[0], 0, bc=(1.1, 0.1)), at(s[1], 1, bc=(0.9, -0.1)), at(s[2], 2, GEOMETRY[1], bc=(1.0337, 0.0421))]),
            ("blur", [far[0], far[-1], pick(0), pick(1), far[0], far[-1]],
             lambda s: [at(s[j], j, blur_k=k) for j, k in enumerate((3, 5, 7, 15))] + [at(s[4], 5, GEOMETRY[6], blur_k=7), at(s[5], 6, GEOMETRY[3], blur_k=3)]),
            ("bc_blur_rotated", [pick(j) for j in range(len(rot))],
             lambda s: [at(s[j], j, g, blur_k=(3, 5, 7, 15, 5)[j], bc=(1.0 + 0.1 * (j - 2), 0.04 * (2 - j))) for j, g in enumerate(rot)]),
            ("gauss_noise", [pick(0), far[0], pick(2)], lambda s: [at(s[0], 5, gauss_sigma=0.01), at(s[1], 6, gauss_sigma=0.1), at(s[2], 7, GEOMETRY[4], gauss_sigma=0.2)]),
            ("chain", [far[-1], pick(1), pick(2)],
             lambda s: [at(s[j], j, GEOMETRY[(1, 6, 2)[j]], blur_k=(3, 0, 7)[j], gauss_sigma=0.05, bc=(1.0 + 0.1 * (j - 1), 0.05 * (1 - j))) for j in range(3)])):
        out.append((what, [c[0] for c in sel], [c[1] for c in sel], np.stack(recs(sel))))
    return out


@everything
def test_bilinear_and_continuous_stages(tile, source, border):
    rows = []
    arena, off, items = _arena(2, source, CO.IMAGE, seed=100, lo=0.02, hi=0.98)
    for what, which, z0s, recs in continuous_cases(tile):
        want, _ = _oracle(items, which, z0s, recs, tile, CO.IMAGE, border)
        rest, _ = _oracle(items, which, z0s, recs, tile, CO.IMAGE, border, dtype=np.float32)
        measured = float(np.abs(rest.astype(np.float64) - want).max())
        if what == "blur":
            # halo = reflect-101 of the OUTPUT tile, not more gathered volume: on these far-corner crops the two differ by far more than the bound
            for j in (0, 1):
                whole, _ = CO.transform_whole(items[which[j]][:, z0s[j]:z0s[j] + tile[0]], recs[j], CO.IMAGE, border)
                ox, oy = CO.origin(recs[j])
                other = CO.VO.box_blur_reflect(whole, int(recs[j]["blur_k"]))[..., oy:oy + tile[1], ox:ox + tile[2]]
                gap = float(np.abs(other - want[j]).max())
                print(f"blur halo {tile} {source} border {border} record {j}: tile reflection vs more gathered volume differ by {gap:.3e}")
                assert gap > 100 * MARGIN * measured
        got = _run(arena, off, which, z0s, recs, 2, tile, CO.IMAGE, border)
        err = float(np.abs(got.astype(np.float64) - want).max())
        rows.append((what, err, measured))
        print(f"continuous {what} {tile} {source} border {border}: kernel max |diff| {err:.3e}, fp32 restatement {measured:.3e}, bound {MARGIN * measured:.3e}")
    for what, err, measured in rows:
        assert measured > 0 and err <= MARGIN * measured, (what, err, measured)


# ---- 5. shot noise -------------------------------------------------------------------------------------------------------------------------
SHOT_SCALES = (0.001, 0.002, 0.005, 0.01, 0.015, 0.02)      # lambda = v^2.2 / s with v <= 0.7: up to 456 ... 23 -- both samplers


def _counts(v, s):
    return np.rint(v.astype(np.float64) ** float(np.float32(2.2)) / float(np.float32(s)))


def test_shot_noise_counts():
    total = rest_diff = got_diff = 0
    worst = 0.0
    for tile in TILES:
        cs = cases(tile)
        for source in SOURCES:
            for border in BORDERS:
                sel = [cs[(j + border) % len(cs)] for j in range(len(SHOT_SCALES))]
                which, z0s = [c[0] for c in sel], [c[1] for c in sel]
                recs = np.stack([_rec(20 + j, c[0], origin=(c[3], c[2]), shot_s=s) for j, (c, s) in enumerate(zip(sel, SHOT_SCALES))])
                arena, off, items = _arena(1, source, CO.IMAGE, seed=300 + 50 * border, lo=0.05, hi=0.7)
                want, _ = _oracle(items, which, z0s, recs, tile, CO.IMAGE, border, shot_counts=True)
                rest, _ = _oracle(items, which, z0s, recs, tile, CO.IMAGE, border, dtype=np.float32, shot_counts=True)
                assert (want * recs["shot_s"][:, None, None, None, None].astype(np.float64)).max() < 1.0          # the clip stays out of it
                got = np.stack([_counts(g, r["shot_s"]) for g, r in zip(_run(arena, off, which, z0s, recs, 1, tile, CO.IMAGE, border), recs)])
                d = np.abs(got - want)
                print(f"shot {tile} {source} border {border}: voxels {want.size}, restatement differs on {int((rest != want).sum())}, kernel on {int((d > 0).sum())}, "
                      f"largest count difference {d.max():.0f}, largest count {want.max():.0f}")
                total, rest_diff, got_diff, worst = total + want.size, rest_diff + int((rest != want).sum()), got_diff + int((d > 0).sum()), max(worst, float(d.max()))
    cap = MARGIN * rest_diff / total
    print(f"shot pooled: {total} voxels, restatement share {rest_diff / total:.3e}, kernel share {got_diff / total:.3e}, cap {cap:.3e}")
    assert worst <= 1
    assert got_diff / total <= cap


# ---- 6. a lane, or a block, that walks more than one plane -------------------------------------------------------------------------------------
def _device_item(shape, source, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if source == "u8":
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    return torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)


def _render(arena, n, channels, tile, kind, border, recs, src, max_blur=0):
    dst = torch.full((n, channels) + tuple(tile), 7.0, dtype=torch.float32, device="cuda")
    assert dst.data_ptr() % 16 == 0
    check(_call(arena, dst, n, channels, tile, kind, border, _bytes(recs), _bytes(src), 0.0, max_blur), "augment_vol_f32_crop")
    return dst


def _alone(whole_src, recs, td):
    """Every z-plane of every sample as a sample of its own: ``td = 1`` at ``z0 + z``."""
    src = np.repeat(whole_src, td)
    src["z0"] += np.tile(np.arange(td, dtype=np.int32), len(whole_src))
    return src, np.repeat(recs, td)


@pytest.mark.parametrize("source,border", [("f32", CO.REFLECT), ("u8", CO.CONSTANT)], ids=["f32-reflect", "u8-constant"])
@pytest.mark.parametrize("kind", [CO.IMAGE, CO.MASK, CO.VECTOR], ids=["image", "mask", "vector"])
def test_a_lane_walks_a_chunk_of_planes(kind, source, border):
    """``[1, C, 130, 256, 256]`` out of an item ``(134, 260, 264)`` at ``z0 = 3``: 16 384 lanes a plane, 2048 blocks need 33 chunks: 4 planes a lane, the
    last chunk 2.  Every plane equals that plane rendered alone (``td = 1``, ``z0 + z``), bit for bit: this also pins ``z0``."""
    item, tile, z0, channels = (134, 260, 264), (130, 256, 256), 3, 2 if kind == CO.VECTOR else 1
    took = lib.biu_augment_vol_chunk(1, channels, *tile, kind, 0, 1)
    print(f"walk {tile} kind {kind} {source} border {border}: chunk {took}, last chunk {tile[0] % took}")
    assert took == 4 and tile[0] % took == 2
    assert lib.biu_augment_vol_chunk(tile[0], channels, 1, *tile[1:], kind, 0, 1) == 1
    g = GEOMETRY[1] if kind == CO.IMAGE else GEOMETRY[2]
    rec = A.record_vol_crop(0, item[1:], angle=g[0], scale=g[1], origin=(3, 2), bc=(1.1, -0.05) if kind == CO.IMAGE else None)
    arena = _device_item((channels,) + item, source, 11).reshape(-1)
    src = np.array([(0,) + item + (z0,)], dtype=A.SOURCE_VOL_DTYPE)
    whole = _render(arena, 1, channels, tile, kind, border, np.stack([rec]), src)
    asrc, arecs = _alone(src, np.stack([rec]), tile[0])
    alone = _render(arena, tile[0], channels, (1,) + tile[1:], kind, border, arecs, asrc)           # [td, C, 1, th, tw]
    alone = alone[:, :, 0].permute(1, 0, 2, 3)[None]
    differing = int((whole != alone).sum())
    print(f"walk {tile} kind {kind} {source} border {border}: differing elements {differing} of {whole.numel()}")
    assert differing == 0 and torch.equal(whole, alone)
    assert not bool((whole[0, :, 1] == whole[0, :, 0]).all())                  # the planes really are different data


@pytest.mark.parametrize("source,border", [("f32", CO.REFLECT), ("u8", CO.CONSTANT)], ids=["f32-reflect", "u8-constant"])
def test_a_block_walks_a_chunk_of_planes(source, border):
    """The blurring launch with two planes per block and a last chunk of one: 32 samples x 65 planes of 70 x 40 (two tiles) out of an item
    ``(67, 75, 52)`` make 2112 blocks at two planes each and 1088 at four.  Every plane equals that plane rendered alone."""
    item, tile, n = (67, 75, 52), (65, 70, 40), 32
    took = lib.biu_augment_vol_chunk(n, 1, *tile, CO.IMAGE, 15, 1)
    print(f"tile walk {(n, 1) + tile} {source} border {border}: chunk {took}, last chunk {tile[0] % took}")
    assert took == 2 and tile[0] % took == 1
    assert lib.biu_augment_vol_chunk(n * tile[0], 1, 1, *tile[1:], CO.IMAGE, 15, 1) == 1
    # every fourth sample does not blur (the blurring launch walks its planes as the point kernel does); the others blur with 3 .. 15
    recs = np.stack([A.record_vol_crop(j, item[1:], angle=GEOMETRY[j % 8][0] or None, scale=GEOMETRY[j % 8][1], origin=(j % 13, j % 6),
                                       bc=(0.9 + 0.05 * (j % 5), 0.03 * (j % 3 - 1)), blur_k=0 if j % 4 == 3 else (3, 5, 7, 15)[j // 4 % 4]) for j in range(n)])
    arena = _device_item((1,) + item, source, 12).reshape(-1)
    src = np.array([(0,) + item + (j % 3,) for j in range(n)], dtype=A.SOURCE_VOL_DTYPE)
    whole = _render(arena, n, 1, tile, CO.IMAGE, border, recs, src, 15)
    asrc, arecs = _alone(src, recs, tile[0])
    alone = _render(arena, n * tile[0], 1, (1,) + tile[1:], CO.IMAGE, border, arecs, asrc, 15).reshape(whole.shape)
    per_sample = (whole != alone).flatten(1).sum(1).cpu().tolist()
    print(f"tile walk {(n, 1) + tile} {source} border {border}: differing elements per sample {per_sample}")
    assert sum(per_sample) == 0 and torch.equal(whole, alone)


# ---- 7. arguments --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    arena, off, items = _arena(2, "f32", CO.IMAGE)
    a = torch.from_numpy(arena).cuda()
    t, r = (4, 64, 64), CO.REFLECT
    count = 2 * 2 * 4 * 64 * 64
    whole = torch.full((count + 1,), 7.0, dtype=torch.float32, device="cuda")
    dst = whole[:count]
    par = _bytes(np.stack([_rec(0, 1), _rec(1, 2)]))
    src = _bytes(_sources(off, [1, 2], [0, 2]))
    bad = [("null arena", _call(None, dst, 2, 2, t, 0, r, par, src, u8=0, elems=10)), ("null dst", _call(a, None, 2, 2, t, 0, r, par, src)),
           ("null records", _call(a, dst, 2, 2, t, 0, r, None, src)), ("null sources", _call(a, dst, 2, 2, t, 0, r, par, None)),
           ("dst inside the arena", _call(a, a[8:], 2, 2, t, 0, r, par, src)),
           ("dst over the records", _call(a, par.view(torch.float32), 2, 2, (1, 1, 1), 0, r, par, src)),
           ("dst over the sources", _call(a, src.view(torch.float32), 2, 2, (1, 1, 1), 0, r, par, src)),
           ("unaligned dst", _call(a, whole.view(torch.uint8)[2:], 2, 2, t, 0, r, par, src)),
           ("unaligned arena", _call(a.view(torch.uint8)[1:], dst, 2, 2, t, 0, r, par, src, u8=0, elems=100)),
           ("unaligned records", _call(a, dst, 2, 2, t, 0, r, par[4:], src)), ("unaligned sources", _call(a, dst, 1, 2, t, 0, r, par, src[4:])),
           ("n = 0", _call(a, dst, 0, 2, t, 0, r, par, src)), ("channels = 0", _call(a, dst, 2, 0, t, 0, r, par, src)),
           ("td = 0", _call(a, dst, 2, 2, (0, 64, 64), 0, r, par, src)), ("th = 0", _call(a, dst, 2, 2, (4, 0, 64), 0, r, par, src)),
           ("tw < 0", _call(a, dst, 2, 2, (4, 64, -1), 0, r, par, src)), ("empty arena", _call(a, dst, 2, 2, t, 0, r, par, src, elems=0)),
           ("unknown kind", _call(a, dst, 2, 2, t, 3, r, par, src)), ("unknown border", _call(a, dst, 2, 2, t, 0, 2, par, src)),
           ("odd vector channels", _call(a, dst, 2, 1, t, 2, r, par, src)), ("blur 17", _call(a, dst, 2, 2, t, 0, r, par, src, blur=17)),
           ("field_id 2^28", _call(a, dst, 2, 2, t, 0, r, par, src, fid=1 << 28)),
           ("2^31 elements", _call(a, dst, 2, 2, (1 << 9, 1 << 10, 1 << 10), 0, r, par, src)),
           ("NaN nan_to_val", _call(a, dst, 2, 2, t, 1, r, par, src, nan_to_val=float("nan")))]
    torch.cuda.synchronize()
    for what, rc in bad:
        print(f"{what}: status {rc}")
    assert all(rc != 0 for _, rc in bad)
    assert bool((whole == 7.0).all())                                               # the canary: nothing was launched
    # sources the kernel refuses per sample are rendered as nan_to_val, their neighbours in the batch normally; nothing outside the arena is read
    par3 = _bytes(np.stack([_rec(0, 2), _rec(1, 2), _rec(2, 2)]))
    want = _crop(items[2], 2, 0, 0, t)
    for what, refused in (("z0 + td > d", (off[2],) + ITEMS[2] + (3,)), ("z0 < 0", (off[2],) + ITEMS[2] + (-1,)),
                          ("offset beyond the arena", (a.numel() - 10,) + ITEMS[2] + (0,)), ("h = 0", (off[2], 6, 0, 64, 0)),
                          ("2^31 - 4 elements or more", (off[2], 1 << 10, 1 << 10, 1 << 10, 0))):
        out = _bytes(np.array([(off[2],) + ITEMS[2] + (2,), refused, (off[2],) + ITEMS[2] + (2,)], dtype=A.SOURCE_VOL_DTYPE))
        for kind, blur in ((CO.IMAGE, 0), (CO.IMAGE, 5), (CO.MASK, 0), (CO.VECTOR, 0)):
            whole.fill_(7.0)
            big = torch.full((3 * 2 * 4 * 64 * 64 + 1,), 7.0, dtype=torch.float32, device="cuda")
            assert _call(a, big[:-1], 3, 2, t, kind, r, par3, out, nan_to_val=-3.0, blur=blur) == 0
            torch.cuda.synchronize()
            got = big[:-1].view(3, 2, 4, 64, 64).cpu().numpy()
            ok = (got[1] == -3.0).all() and _same(got[0], want) and _same(got[2], want) and float(big[-1]) == 7.0
            print(f"refused source ({what}) kind {kind} blur {blur}: {'nan_to_val, neighbours intact' if ok else 'WRONG'}")
            assert ok


# ---- 8. prepare, feeder, Trainer -----------------------------------------------------------------------------------------------------------
HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "orientation": {"channels": 2, "activation": None, "loss": "TverskyLoss", "weight": 0.5}}
RAW_SIZES = ((7, 70, 90), (6, 64, 64), (9, 80, 130))


def _raw(seed=0, sizes=RAW_SIZES):
    rng = np.random.default_rng(seed)
    volumes = [rng.integers(100, 4000, s).astype(np.uint16) for s in sizes]
    mask = [_nan_holes((rng.random(s) > 0.5).astype(np.float32), rng) for s in sizes]
    distance = [(rng.random(s) * 5).astype(np.float64) for s in sizes]
    orientation = [_nan_holes(rng.uniform(0, 2 * np.pi, s), rng) for s in sizes]
    return volumes, {"mask": mask, "distance": distance, "orientation": orientation}


def _epoch(fd):
    return [{k: v.cpu().clone() for k, v in b.items()} for b in fd]


DIM = (4, 48, 48)


def test_crop_feeder_and_prepare(tmp_path):
    from bio_image_unet_amd import multi_output_unet3d as M
    from bio_image_unet_amd.preprocess import DeviceFrontEnd
    volumes, targets = _raw()
    kw = dict(dim_out=DIM, aug_factor=3, clip_threshold=(0., 99.98), device="cuda")
    st = M.prepare(volumes, targets, str(tmp_path / "s"), nan_to_val=-1, scale_limit=(-0.5, 0), **kw)
    assert isinstance(st, feed.VolumeStore) and st.fields == {"volume": DIM, "mask": DIM, "distance": DIM, "orientation": (2,) + DIM}
    assert len(st) == 9 and st.nan_to_val == -1.0 and st.aug_factor == 3 and [tuple(s) for s in st.sizes] == list(RAW_SIZES)
    for i, vol in enumerate(volumes):
        fe = DeviceFrontEnd(vol, "cuda", depth=vol.shape[0])
        fe.normalise("single", (0., 99.98))
        want = fe.tiles([(0, 0, 0, 0)], vol.shape, out="float32").batch(0, 1)[0].cpu().numpy()
        got = np.asarray(st.item(i, "volume"))[0]
        print(f"prepare item {i}: volume equal to the front end's {_same(got, want)}, range {want.min():.4f} .. {want.max():.4f}")
        assert _same(got, want) and 0.0 <= want.min() and want.max() == 1.0
        phi = targets["orientation"][i].astype(np.float32)
        assert np.asarray(st.item(i, "orientation")).tobytes() == np.stack([np.cos(phi), np.sin(phi)]).tobytes()
        assert np.asarray(st.item(i, "mask")).tobytes() == targets["mask"][i].tobytes() and np.isnan(st.item(i, "mask")).any()
        assert np.asarray(st.item(i, "distance")).tobytes() == targets["distance"][i].astype(np.float32).tobytes()
        assert np.array_equal(np.isnan(st.item(i, "orientation")[0]), np.isnan(st.item(i, "orientation")[1]))
    mk = lambda s=st: A.AugmenterVol.from_store(s, seed=5)
    assert mk().scale_limit == (-0.5, 0.0)
    idx = [int(i) for i in np.random.default_rng(0).permutation(len(st))][:8]
    fa, fb = feed.CropFeeder(st, idx, 2, "cuda", mk(), depth=2), feed.CropFeeder(st, idx, 2, "cuda", mk(), epoch_key=0)
    a0, b0, a1 = _epoch(fa), _epoch(fb), _epoch(fa)
    assert len(a0) == 4 and all(v.dtype == torch.float32 and not torch.isnan(v).any() for b in a0 for v in b.values())
    assert a0[0]["volume"].shape == (2,) + DIM and a0[0]["orientation"].shape == (2, 2) + DIM
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a0, b0) for k in x)             # the same key: the same bits
    assert any(not torch.equal(x["volume"], y["volume"]) for x, y in zip(a0, a1))      # another epoch: other crops
    assert all(torch.equal(x[k], y[k]) for x, y in zip(b0, _epoch(fb)) for k in x)     # a fixed key: the same every time
    assert any(bool((b["mask"] == -1.0).any()) for b in a0)
    # a batch equals the oracle's rendering of draw_crops' records on safe voxels
    recs, sources = mk().draw_crops(0, idx, st)
    for j, r in enumerate(recs):
        i, z0 = st.locate(idx[j]), int(sources["mask"]["z0"][j])
        got = {k: a0[j // 2][k][j % 2].numpy().astype(np.float64) for k in ("mask", "distance", "orientation", "volume")}
        for k, kind in (("mask", CO.MASK), ("distance", CO.MASK), ("orientation", CO.VECTOR)):
            want, safe = CO.apply(np.asarray(st.item(i, k)), r, z0, DIM, kind, CO.REFLECT, -1.0, 5, 0, A.field_id(k))
            d = np.abs(got[k].reshape(want.shape) - want)[..., safe]
            print(f"feeder patch {idx[j]} item {i} z0 {z0} origin {CO.origin(r)} {k}: max |diff| on safe voxels {d.max():.3g}, left out {100 * (1 - safe.mean()):.3f} %")
            assert d.max() <= (VECTOR_BOUND if kind == CO.VECTOR else 0.0)
        if not int(r["flags"]) & A.SHOT_F:                                             # counts have a test of their own
            args = (np.asarray(st.item(i, "volume")), r, z0, DIM, CO.IMAGE, CO.REFLECT, -1.0, 5, 0, A.field_id("volume"))
            want, rest = CO.apply(*args)[0], CO.apply(*args, dtype=np.float32)[0]
            err, measured = np.abs(got["volume"] - want[0]).max(), np.abs(rest.astype(np.float64) - want).max()
            print(f"feeder patch {idx[j]} volume: kernel max |diff| {err:.3e}, fp32 restatement {measured:.3e}")
            assert err <= MARGIN * measured
    with pytest.raises(ValueError):
        feed.CropFeeder(st, idx, 2, "cuda", None)
    with pytest.raises(ValueError):
        feed.CropFeeder(st, idx, 2, "cuda", A.AugmenterF32())
    u8 = M.prepare(volumes, targets, str(tmp_path / "u"), volume_dtype="u8", **kw)
    assert u8.dtypes["volume"] == "u8" and np.abs(np.asarray(u8.item(0, "volume")) / 255.0 - np.asarray(st.item(0, "volume"))).max() <= 1 / 255.0
    assert next(iter(feed.CropFeeder(u8, idx, 2, "cuda", mk(u8))))["volume"].dtype == torch.float32


@pytest.mark.timeout(300)
def test_trainer_mo3d_on_a_volume_store(tmp_path):
    """One epoch of ``multi_output_unet3d.Trainer`` on a prepared ``VolumeStore``.  ``MultiOutputUnet3D`` pools three times and refuses a
    depth that is no multiple of 8 (``models.py``, as the reference's ``torch.cat`` does), so this store cannot have the ``dim_out = (4, 48, 48)``
    of the feeder test above: its patches are ``(8, 48, 48)`` and its volumes two to three planes deeper, ``(9, 70, 90)``, ``(8, 64, 64)`` (a
    volume exactly as deep as the patch: ``z0`` is always 0 there) and ``(11, 80, 130)``; everything else is the same."""
    from bio_image_unet_amd import multi_output_unet3d as M
    volumes, targets = _raw(1, ((9, 70, 90), (8, 64, 64), (11, 80, 130)))
    st = M.prepare(volumes, targets, str(tmp_path / "s"), dim_out=(8, 48, 48), nan_to_val=0, aug_factor=3, scale_limit=(-0.5, 0), device="cuda")
    assert len(st) == 9                                                             # val_split 0.25: 7 patches to train on, 2 (one batch) to validate on
    torch.manual_seed(3)
    kw = dict(n_filter=8, batch_size=2, val_split=0.25, device="cuda")
    tr = M.Trainer(st, HEADS, 1, save_dir=str(tmp_path / "o"), **kw)
    assert isinstance(tr.augmenter, A.AugmenterVol) and tr.augmenter.scale_limit == (-0.5, 0.0)
    assert isinstance(tr.train_loader, feed.CropFeeder) and isinstance(tr.val_loader, feed.CropFeeder)
    assert tr.val_loader.epoch_key == A.VALIDATION_EPOCH and tr.train_loader.epoch_key is None and tr.params["augmentation"] == 3
    assert len(tr.train_loader.indices) == 7 and len(tr.val_loader.indices) == 2 and len(tr.val_loader) == 1 and len(tr.train_loader) == 3
    v0, v1 = _epoch(tr.val_loader), _epoch(tr.val_loader)
    assert len(v0) == 1 and all(torch.equal(x[k], y[k]) for x, y in zip(v0, v1) for k in x)      # validation patches: augmented, but fixed
    tr.start()
    ck = torch.load(str(tmp_path / "o" / "model.pt"), weights_only=False)
    print(f"TrainerMo3d on a VolumeStore: validation loss after one epoch {float(ck['best_loss']):.6f}")
    assert torch.isfinite(torch.as_tensor(ck["best_loss"])) and ck["online_augmentation"]["recipe"] == "mo3d" and tr.train_loader.epoch == 1
    own = A.AugmenterVol.from_store(st, seed=77, border="constant")
    assert M.Trainer(st, HEADS, 1, save_dir=str(tmp_path / "p"), augment=own, **kw).augmenter is own
    with pytest.raises(ValueError):
        M.Trainer(st, HEADS, 1, save_dir=str(tmp_path / "q"), augment=False, **kw)
