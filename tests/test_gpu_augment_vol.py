"""Volume augmentation on the GPU: ``biu_augment_vol_f32`` through the C ABI against the float64 oracle (``tests/augment_vol_oracle.py``), then
the feeder and ``TrainerMo3d`` that carry it.  Every test prints its figures before it asserts, and runs on both source types (float32, uint8)
and both borders (reflect-101, constant 0) unless it says why not.

The shapes are small on purpose: ``(3, 19, 37)`` has odd rows (no 16-byte stores), ``(2, 70, 130)`` crosses the 64-tile edge on both axes with
a halo of 7, ``(5, 48, 80)`` and ``(4, 96, 96)`` take the 16-byte path (the square one also the odd quarter turns); the vector fields are
``[2, D, H, W]`` with the (cos, sin) planes a volume apart.

Bounds (none of them comes from what the kernel gives):

* exact cases (the empty record, quarter turns, brightness/contrast alone -- the kernel rounds product and sum one after the other, as the fp32
  formula does): bit for bit.
* nearest gathers: MASK equals the oracle on every pixel whose float64 source coordinate is farther than 1e-3 from a rounding tie; at most 1 %
  of the pixels may be left out (asserted first; these geometries leave out at most 0.853 %, ``tests/test_augment_vol_host.py``).  A VECTOR
  field is gathered exactly but its pair is rotated in fp32: three roundings of 2^-24 on ``|c cos_t| + |s sin_t| <= sqrt(2)``:
  ``3 sqrt(2) 2^-24 = 2.53e-7``, the bound of ``tests/test_gpu_augment_f32.py``.
* the bilinear IMAGE gather and the continuous stages, on ALL pixels (a bilinear gather has no ties): six times the largest deviation of the
  fp32 numpy restatement (``augment_vol_oracle`` with ``dtype=np.float32``) from the float64 oracle ON THE SAME INPUTS, computed by the test on
  the CPU; the restatement's deviation must be above 0.  The margin is ``tests/test_gpu_augment.py``'s, for fused multiply-adds and another
  operation order.
* shot noise: no count may differ from the oracle's by more than one, and the share of differing pixels is capped at six times the share on
  which the fp32 restatement differs, pooled over all shapes, sources, borders and six noise scales.
* chunks of planes: the launch gives a lane (a block of the blurring path) more than one plane only once it has 2048 blocks without, which
  none of the small shapes reaches.  Three tests use fields large enough for chunks of 2, 4 and 16 planes with a shorter last chunk, ask the
  library which chunk it takes (``biu_augment_vol_chunk``) and assert it: noise-free fields equal the same planes run alone bit for bit
  (compared on the device; no oracle, so the size costs little), and a noisy chain, whose Philox counter holds the element's place in the
  whole field, is within the continuous stages' bound of the oracle.
* a radial field stays radial: a nearest gather displaces the source by at most ``sqrt(0.5)`` pixels, i.e. the angle by at most
  ``atan(sqrt(0.5) / r_src)`` at the source radius ``r_src = r / scale``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd._lib import check, lib  # noqa: E402
from bio_image_unet_amd.feed import DeviceFeeder, TileStore  # noqa: E402
from tests import augment_vol_oracle as VO  # noqa: E402

VOL_SHAPES = [(3, 19, 37), (2, 70, 130), (5, 48, 80), (4, 96, 96)]             # [D, H, W]
VEC_SHAPES = [(2, 3, 19, 37), (2, 2, 70, 130)]                                # [C, D, H, W]
SOURCES = ["f32", "u8"]
BORDERS = [VO.REFLECT, VO.CONSTANT]
# angle in degrees, scale
GEOMETRY = [(17.3, 1), (151, 0.7313), (203.7, 0.4137), (359, 0.2913), (77.7, 0.5519), (0, 0.6137), (0, 0.9137), (0, 0.3371)]
SEED, EPOCH, FID = 0x1234567890ABCDEF, 3, A.field_id("volume")
VECTOR_BOUND = 3 * np.sqrt(2.0) * 2.0 ** -24
MARGIN = 6.0
ids = lambda s: s if isinstance(s, str) else ("reflect", "constant")[s] if isinstance(s, int) else "x".join(map(str, s))
cdhw = lambda shape: tuple(shape) if len(shape) == 4 else (1,) + tuple(shape)


def everything(fn):
    """Both borders x both source types."""
    return pytest.mark.parametrize("border", BORDERS, ids=ids)(pytest.mark.parametrize("source", SOURCES)(fn))


def _field(shape, source, seed, lo=0.0, hi=1.0, vector=False):
    """A noise field ``[C, D, H, W]`` of one sample: float32 in [lo, hi) or uint8; ``vector``: unit (cos, sin) channel pairs (as bytes: any numbers)."""
    rng = np.random.default_rng(seed)
    shape = cdhw(shape)
    if vector:
        phi = rng.uniform(0, 2 * np.pi, (shape[0] // 2,) + shape[1:])
        f = np.stack([np.cos(phi), np.sin(phi)], axis=1).reshape(shape)
        return f.astype(np.float32) if source == "f32" else np.rint((f + 1) * 127.5).astype(np.uint8)
    if source == "u8":
        return rng.integers(int(lo * 255), max(int(hi * 255), 1) + 1, size=shape, dtype=np.uint8)
    return (lo + (hi - lo) * rng.random(shape)).astype(np.float32)


def _batch(shape, source, n, kind=VO.IMAGE, seed0=0, **kw):
    return np.stack([_field(shape, source, seed0 + i, vector=kind == VO.VECTOR, **kw) for i in range(n)])


def _geo(index, h, w, g, **kw):
    return A.record_f32(index, h, w, angle=g[0] if g[0] else None, scale=g[1] if g[1] != 1 else None, **kw)


def _call(src, dst, par, dims, kind, border, max_blur, seed=SEED, epoch=EPOCH, fid=FID, u8=0):
    n, c, d, h, w = dims
    return lib.biu_augment_vol_f32(C.c_void_p(src.data_ptr()), u8, C.c_void_p(dst.data_ptr()), n, c, d, h, w, kind, border, C.c_void_p(par.data_ptr()),
                                   max_blur, seed, epoch, fid, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _run(batch, recs, kind, border, seed=SEED, epoch=EPOCH, fid=FID):
    """``batch`` [N, C, D, H, W] float32 or uint8, one record per sample -> the kernel's output as a numpy array."""
    recs = np.ascontiguousarray(recs, dtype=A.PARAMS_F32_DTYPE)
    assert batch.ndim == 5 and len(recs) == len(batch)
    src = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
    dst = torch.full(batch.shape, 7.0, dtype=torch.float32, device="cuda")
    par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    blurs = recs["blur_k"][(recs["flags"] & A.BLUR_F) != 0]
    check(_call(src, dst, par, batch.shape, kind, border, int(blurs.max()) if kind == VO.IMAGE and len(blurs) else 0, seed, epoch, fid,
                int(batch.dtype == np.uint8)), "augment_vol_f32")
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _oracle(batch, recs, kind, border, dtype=np.float64, seed=SEED, epoch=EPOCH, fid=FID, **kw):
    outs, safes = zip(*[VO.apply(batch[i], recs[i], kind, border, seed, epoch, fid, dtype=dtype, **kw) for i in range(len(batch))])
    return np.stack(outs), np.stack(safes)


def _rots(h, w):
    return (0, 1, 2, 3) if h == w else (0, 2)


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _kinds(shape):
    return (VO.VECTOR,) if len(shape) == 4 else (VO.IMAGE, VO.MASK)


# ---- 1. exact cases ------------------------------------------------------------------------------------------------------------------------
@everything
@pytest.mark.parametrize("shape", VOL_SHAPES + VEC_SHAPES, ids=ids)
def test_exact_cases(shape, source, border):
    """The empty record returns the widened source, quarter turns equal ``np.rot90`` per plane (sign-and-swap of the pair for VECTOR), a
    brightness/contrast-only record equals the fp32 formula: bit for bit, and the same with a blurring neighbour in the batch (the tile kernel)."""
    h, w = shape[-2:]
    rk = _rots(h, w)
    recs = np.stack([A.record_f32(i, h, w, rot_k=k) for i, k in enumerate(rk)])
    for kind in _kinds(shape):
        batch = _batch(shape, source, len(recs), kind)
        wide = VO.widen(batch)
        got = _run(batch, recs, kind, border)
        for i, k in enumerate(rk):
            turned = np.rot90(wide[i], k, axes=(2, 3))
            if kind == VO.VECTOR:
                c, s = turned[0::2], turned[1::2]
                wc, ws = [(c, s), (s, -c), (-c, -s), (-s, c)][k]
                ok = _same(got[i][0::2], wc) and _same(got[i][1::2], ws)
            else:
                ok = _same(got[i], turned)
            print(f"exact {shape} {source} border {border} kind {kind} rot_k {k}: {'equal' if ok else 'DIFFERENT'}")
            assert ok, (kind, k)
        assert _same(_run(batch, recs, kind, border), got)                          # two launches give the same bytes
    if len(shape) == 4:
        return
    bcs = [(1.1, 0.1), (0.9, -0.1), (1.0337, 0.0421), (1.3, 0.2)]
    img = _batch(shape, source, len(bcs) + 2, seed0=20)
    brecs = np.stack([A.record_f32(i, h, w, bc=bc) for i, bc in enumerate(bcs)] + [A.record_f32(7, h, w), A.record_f32(8, h, w, rot_k=2)])
    wide = VO.widen(img)
    want = [np.clip(wide[i] * np.float32(a) + np.float32(b), np.float32(0), np.float32(1)) for i, (a, b) in enumerate(bcs)]
    want += [wide[len(bcs)], np.rot90(wide[len(bcs) + 1], 2, axes=(2, 3))]
    assert all(x.dtype == np.float32 for x in want)
    got = _run(img, brecs, VO.IMAGE, border)
    # the same through the tile kernel: a blurring neighbour in the batch sends the whole launch there
    tile = _run(np.concatenate([img[:1], img]), np.concatenate([np.stack([A.record_f32(99, h, w, blur_k=5, gauss_sigma=0.05, bc=(1.1, 0.02))]), brecs]),
                VO.IMAGE, border)
    for i in range(len(brecs)):
        a, b = _same(got[i], want[i]), _same(tile[i + 1], want[i])
        print(f"exact {shape} {source} border {border} image record {i}: point kernel {'equal' if a else 'DIFFERENT'}, tile kernel {'equal' if b else 'DIFFERENT'}")
        assert a and b, i


# ---- 2. nearest gathers --------------------------------------------------------------------------------------------------------------------
@everything
@pytest.mark.parametrize("shape", VOL_SHAPES + VEC_SHAPES, ids=ids)
def test_nearest_gathers(shape, source, border):
    """MASK equals the oracle on every safe pixel, VECTOR is within the fp32 rotation's bound there; at most 1 % is left out."""
    h, w = shape[-2:]
    kind = VO.VECTOR if len(shape) == 4 else VO.MASK
    recs = np.stack([_geo(i, h, w, g) for i, g in enumerate(GEOMETRY)])
    batch = _batch(shape, source, len(recs), kind, seed0=7)
    got = _run(batch, recs, kind, border)
    want, safe = _oracle(batch, recs, kind, border)
    for i, g in enumerate(GEOMETRY):
        left_out = 1.0 - safe[i].mean()
        d = np.abs(got[i].astype(np.float64) - want[i])
        tol = VECTOR_BOUND if kind == VO.VECTOR else 0.0
        bad = int((d > tol)[..., safe[i]].sum())
        print(f"nearest {shape} {source} border {border} kind {kind} {g}: left out {100 * left_out:.3f} %, beyond {tol:.3g} on safe pixels {bad}, "
              f"on all pixels {int((d > tol).sum())}, max on safe {d[..., safe[i]].max():.3g}")
        assert left_out <= 0.01
        assert bad == 0


# ---- 3. the bilinear image and the continuous stages ----------------------------------------------------------------------------------------
def continuous_cases(shape):
    """(stage, records) of the continuous checks, all IMAGE."""
    d, h, w = shape
    rot = [g for g in GEOMETRY if g[0]]
    return [("gather", [_geo(i, h, w, g) for i, g in enumerate(GEOMETRY)]),
            ("brightness_contrast", [A.record_f32(0, h, w, bc=(1.1, 0.1)), A.record_f32(1, h, w, bc=(0.9, -0.1)), _geo(2, h, w, GEOMETRY[1], bc=(1.0337, 0.0421))]),
            ("blur", [A.record_f32(i, h, w, blur_k=k) for i, k in enumerate((3, 5, 7, 15))] + [_geo(5, h, w, GEOMETRY[6], blur_k=7), _geo(6, h, w, GEOMETRY[3], blur_k=3)]),
            ("bc_blur_rotated", [_geo(i, h, w, g, blur_k=(3, 5, 7, 15, 5)[i], bc=(1.0 + 0.1 * (i - 2), 0.04 * (2 - i))) for i, g in enumerate(rot)]),
            ("gauss_noise", [A.record_f32(5, h, w, gauss_sigma=0.01), A.record_f32(6, h, w, gauss_sigma=0.1), _geo(7, h, w, GEOMETRY[4], gauss_sigma=0.2)]),
            ("chain", [_geo(i, h, w, GEOMETRY[(1, 6, 2)[i]], blur_k=(3, 0, 7)[i], gauss_sigma=0.05, bc=(1.0 + 0.1 * (i - 1), 0.05 * (1 - i))) for i in range(3)])]


@everything
@pytest.mark.parametrize("shape", VOL_SHAPES, ids=ids)
def test_bilinear_and_continuous_stages(shape, source, border):
    """The bilinear gather, brightness/contrast, blur, brightness/contrast -> blur under a rotation, Gauss noise and a whole chain, on all pixels,
    within six times the deviation of the fp32 numpy restatement from the float64 oracle on the same inputs (module docstring)."""
    rows = []
    for what, recs in continuous_cases(shape):
        recs = np.stack(recs)
        batch = _batch(shape, source, len(recs), seed0=100, lo=0.02, hi=0.98)
        want, _ = _oracle(batch, recs, VO.IMAGE, border)
        rest, _ = _oracle(batch, recs, VO.IMAGE, border, dtype=np.float32)
        measured = float(np.abs(rest.astype(np.float64) - want).max())
        got = _run(batch, recs, VO.IMAGE, border)
        err = float(np.abs(got.astype(np.float64) - want).max())
        rows.append((what, err, measured))
        print(f"continuous {what} {shape} {source} border {border}: kernel max |diff| {err:.3e}, fp32 restatement {measured:.3e}, bound {MARGIN * measured:.3e}")
    for what, err, measured in rows:
        assert measured > 0 and err <= MARGIN * measured, (what, err, measured)


# ---- 4. shot noise -------------------------------------------------------------------------------------------------------------------------
SHOT_SCALES = (0.001, 0.002, 0.005, 0.01, 0.015, 0.02)      # lambda = v^2.2 / s with v <= 0.7: up to 456 ... 23 -- both samplers


def shot_cases():
    for shape in VOL_SHAPES:
        for source in SOURCES:
            for border in BORDERS:
                d, h, w = shape
                recs = np.stack([A.record_f32(20 + i, h, w, shot_s=s) for i, s in enumerate(SHOT_SCALES)])
                yield shape, source, border, recs, _batch(shape, source, len(recs), seed0=300 + 50 * border, lo=0.05, hi=0.7)


def _counts(v, s):
    """The Poisson counts behind a shot-noise output (``n s < 1`` on these inputs, so the clip never bites)."""
    return np.rint(v.astype(np.float64) ** float(np.float32(2.2)) / float(np.float32(s)))


@pytest.mark.timeout(900)
def test_shot_noise_counts():
    """Counts differ from the oracle's by at most one, on at most six times the share of pixels on which the fp32 restatement differs (pooled)."""
    total = rest_diff = got_diff = 0
    worst = 0.0
    for shape, source, border, recs, batch in shot_cases():
        want, _ = _oracle(batch, recs, VO.IMAGE, border, shot_counts=True)
        rest, _ = _oracle(batch, recs, VO.IMAGE, border, dtype=np.float32, shot_counts=True)
        assert (want * recs["shot_s"][:, None, None, None, None].astype(np.float64)).max() < 1.0                  # the clip stays out of it
        got = np.stack([_counts(g, r["shot_s"]) for g, r in zip(_run(batch, recs, VO.IMAGE, border), recs)])
        d = np.abs(got - want)
        print(f"shot {shape} {source} border {border}: pixels {want.size}, restatement differs on {int((rest != want).sum())}, kernel on {int((d > 0).sum())}, "
              f"largest count difference {d.max():.0f}, largest count {want.max():.0f}")
        total, rest_diff, got_diff, worst = total + want.size, rest_diff + int((rest != want).sum()), got_diff + int((d > 0).sum()), max(worst, float(d.max()))
    cap = MARGIN * rest_diff / total
    print(f"shot pooled: {total} pixels, restatement share {rest_diff / total:.3e}, kernel share {got_diff / total:.3e}, cap {cap:.3e}")
    assert worst <= 1
    assert got_diff / total <= cap


# ---- 5. depth and channel independence -----------------------------------------------------------------------------------------------------
@everything
@pytest.mark.parametrize("shape", [(2, 3, 19, 37), (2, 2, 70, 130), (4, 5, 48, 80)], ids=ids)
def test_planes_are_independent(shape, source, border):
    """Plane ``z`` of channel ``c`` of a ``[C, D, H, W]`` run equals, bit for bit, a run on that plane alone (VECTOR: on that pair of planes alone),
    for MASK, VECTOR and noise-free IMAGE records, through the point kernel and the tile kernel."""
    c, d, h, w = shape
    cases = [(VO.MASK, _geo(0, h, w, GEOMETRY[1])), (VO.VECTOR, _geo(0, h, w, GEOMETRY[2])), (VO.IMAGE, _geo(0, h, w, GEOMETRY[4], bc=(1.1, -0.05))),
             (VO.IMAGE, _geo(0, h, w, GEOMETRY[1], bc=(0.9, 0.05), blur_k=7))]
    for kind, rec in cases:
        batch = _batch(shape, source, 1, kind, seed0=60)
        whole = _run(batch, np.stack([rec]), kind, border)[0]
        if kind == VO.VECTOR:               # the pair (2 j, 2 j + 1) at depth z, as a [2, 1, H, W] sample of its own
            alone_in = batch[0].reshape(c // 2, 2, d, h, w).transpose(0, 2, 1, 3, 4).reshape(c // 2 * d, 2, 1, h, w)
            alone = _run(np.ascontiguousarray(alone_in), np.stack([rec] * len(alone_in)), kind, border)
            alone = alone.reshape(c // 2, d, 2, h, w).transpose(0, 2, 1, 3, 4).reshape(c, d, h, w)
        else:
            alone = _run(np.ascontiguousarray(batch[0].reshape(c * d, 1, 1, h, w)), np.stack([rec] * (c * d)), kind, border).reshape(c, d, h, w)
        differing = int((whole != alone).sum())
        distinct = len({whole[i, j].tobytes() for i in range(c) for j in range(d)})
        print(f"planes {shape} {source} border {border} kind {kind} blur {int(rec['blur_k'])}: differing elements {differing}, distinct planes {distinct} of {c * d}")
        assert differing == 0 and _same(whole, alone)
        assert distinct == c * d                                    # the planes really are different data


# ---- 5b. a lane, or a block, that walks more than one plane -----------------------------------------------------------------------------------
def _chunk(dims, kind, max_blur=0):
    """The planes per lane (per block of the blurring path) the library takes for this launch, with a 16-byte aligned destination."""
    return lib.biu_augment_vol_chunk(*dims, kind, max_blur, 1)


def _run_on_device(src, recs, kind, border, max_blur=0):
    recs = np.ascontiguousarray(recs, dtype=A.PARAMS_F32_DTYPE)
    assert src.dim() == 5 and src.is_contiguous() and len(recs) == len(src)
    dst = torch.full(src.shape, 7.0, dtype=torch.float32, device="cuda")
    assert dst.data_ptr() % 16 == 0
    par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    check(_call(src, dst, par, tuple(src.shape), kind, border, max_blur, u8=int(src.dtype == torch.uint8)), "augment_vol_f32")
    return dst


def _device_field(shape, source, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if source == "u8":
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    return torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)


def _alone(src, kind):
    """``[N, C, D, H, W]`` -> every plane (VECTOR: every pair of planes) as a sample of its own, and how to put the outputs back."""
    n, c, d, h, w = src.shape
    if kind != VO.VECTOR:
        return src.reshape(n * c * d, 1, 1, h, w), lambda out: out.reshape(n, c, d, h, w)
    split = src.reshape(n, c // 2, 2, d, h, w).permute(0, 1, 3, 2, 4, 5).reshape(n * (c // 2) * d, 2, 1, h, w).contiguous()
    return split, lambda out: out.reshape(n, c // 2, d, 2, h, w).permute(0, 1, 3, 2, 4, 5).reshape(n, c, d, h, w)


# 130 planes of 256 x 256: 16 384 lanes a plane (4 pixels each), 2048 blocks need 33 chunks: 4 planes a lane, the last chunk 2.
# 130 planes of 254 x 254: no 16-byte stores, 64 516 lanes a plane, 9 chunks fill 2048 blocks: 16 planes a lane, the last chunk 2.
WALKS = [((130, 256, 256), 4), ((130, 254, 254), 16)]


@everything
@pytest.mark.parametrize("kind", [VO.IMAGE, VO.MASK, VO.VECTOR], ids=["image", "mask", "vector"])
@pytest.mark.parametrize("dhw,chunk", WALKS, ids=["rows4", "single"])
def test_a_lane_walks_a_chunk_of_planes(dhw, chunk, kind, source, border):
    """The point kernels with more than one plane per lane and a shorter last chunk: every plane equals, bit for bit, that plane run alone
    (one plane per lane).  The chunk the library takes is asserted, so the shape cannot fall back to one plane per lane unnoticed."""
    d, h, w = dhw
    dims = (1, 2 if kind == VO.VECTOR else 1, d, h, w)
    units = d
    took = _chunk(dims, kind)
    print(f"walk {dims} kind {kind} {source} border {border}: chunk {took}, last chunk {units % took}")
    assert took == chunk and units % took == 2
    rec = _geo(0, h, w, GEOMETRY[1], bc=(1.1, -0.05)) if kind == VO.IMAGE else _geo(0, h, w, GEOMETRY[2])
    src = _device_field(dims, source, 11)
    whole = _run_on_device(src, np.stack([rec]), kind, border)
    alone_src, back = _alone(src, kind)
    assert _chunk(tuple(alone_src.shape), kind) == 1
    alone = back(_run_on_device(alone_src, np.stack([rec] * len(alone_src)), kind, border))
    differing = int((whole != alone).sum())
    print(f"walk {dims} kind {kind} {source} border {border}: differing elements {differing} of {whole.numel()}")
    assert differing == 0 and torch.equal(whole, alone)
    assert not bool((whole[0, :, 1] == whole[0, :, 0]).all())                  # the planes really are different data


def _tile_records(n, h, w, **kw):
    """Every fourth sample does not blur (the blurring launch walks its planes as the point kernel does); the others blur with 3 .. 15."""
    return np.stack([_geo(i, h, w, GEOMETRY[i % len(GEOMETRY)], bc=(0.9 + 0.05 * (i % 5), 0.03 * (i % 3 - 1)), blur_k=0 if i % 4 == 3 else (3, 5, 7, 15)[i // 4 % 4],
                          **{k: v(i) for k, v in kw.items()}) for i in range(n)])


@everything
def test_a_block_walks_a_chunk_of_planes(source, border):
    """The blurring launch with two planes per block and a last chunk of one: 32 samples x 65 planes of 70 x 40 (two tiles) make 2112 blocks at
    two planes each and 1088 at four.  The LDS tiles are reused from plane to plane; every plane equals that plane run alone."""
    n, d, h, w = 32, 65, 70, 40
    dims = (n, 1, d, h, w)
    took = _chunk(dims, VO.IMAGE, 15)
    print(f"tile walk {dims} {source} border {border}: chunk {took}, last chunk {d % took}")
    assert took == 2 and d % took == 1
    recs = _tile_records(n, h, w)
    src = _device_field(dims, source, 12)
    whole = _run_on_device(src, recs, VO.IMAGE, border, 15)
    alone_src, back = _alone(src, VO.IMAGE)
    assert _chunk(tuple(alone_src.shape), VO.IMAGE, 15) == 1
    alone = back(_run_on_device(alone_src, np.repeat(recs, d), VO.IMAGE, border, 15))
    per_sample = (whole != alone).flatten(1).sum(1).cpu().tolist()
    print(f"tile walk {dims} {source} border {border}: differing elements per sample {per_sample}")
    assert sum(per_sample) == 0 and torch.equal(whole, alone)


@everything
@pytest.mark.parametrize("which", ["point", "tile"])
def test_noise_over_a_chunk_of_planes(which, source, border):
    """Gauss noise behind the gather, brightness/contrast and (tile) the blur, where a lane or block walks two planes and the last chunk is
    one: the counter holds the voxel's place in the whole field, so no plane can be run alone; the oracle is the reference, under the bound of
    the continuous stages (six times the fp32 restatement's deviation, on all voxels).
    point: 8 x 65 planes of 45 x 45, 2025 lanes a plane: 534 600 lanes at two planes each (2048 blocks are 524 288), 275 400 at four.
    tile : 64 x 65 planes of 10 x 12, one tile: 2112 blocks at two planes each, 1088 at four."""
    n, d, h, w = (8, 65, 45, 45) if which == "point" else (64, 65, 10, 12)
    dims = (n, 1, d, h, w)
    sigma = lambda i: 0.02 * (1 + i % 4)
    if which == "point":
        recs = np.stack([_geo(i, h, w, GEOMETRY[i], bc=(0.9 + 0.05 * (i % 5), 0.03 * (i % 3 - 1)), gauss_sigma=sigma(i)) for i in range(n)])
    else:
        recs = _tile_records(n, h, w, gauss_sigma=sigma)
    max_blur = 0 if which == "point" else 15
    took = _chunk(dims, VO.IMAGE, max_blur)
    print(f"noise walk {which} {dims} {source} border {border}: chunk {took}, last chunk {d % took}")
    assert took == 2 and d % took == 1
    batch = _batch((d, h, w), source, n, seed0=500, lo=0.02, hi=0.98)
    want, _ = _oracle(batch, recs, VO.IMAGE, border)
    rest, _ = _oracle(batch, recs, VO.IMAGE, border, dtype=np.float32)
    measured = float(np.abs(rest.astype(np.float64) - want).max())
    got = _run_on_device(torch.from_numpy(batch).cuda(), recs, VO.IMAGE, border, max_blur).cpu().numpy()
    per_plane = np.abs(got.astype(np.float64) - want).max(axis=(0, 1, 3, 4))
    err = float(per_plane.max())
    print(f"noise walk {which} {dims} {source} border {border}: kernel max |diff| {err:.3e} (first planes of the chunks {per_plane[0::2].max():.3e}, "
          f"second {per_plane[1::2].max():.3e}), fp32 restatement {measured:.3e}, bound {MARGIN * measured:.3e}")
    assert measured > 0 and err <= MARGIN * measured


# ---- 6. a radial field stays radial --------------------------------------------------------------------------------------------------------
@everything
def test_a_radial_field_stays_radial(source, border):
    """``phi = atan2(y - cy, x - cx)`` stored as (cos, sin), rotated and scaled by every rotating geometry, is the radial field of the output
    grid within the nearest gather's displacement, ``atan(sqrt(0.5) / r_src)``, on ``8 <= r_src <= 30``.  A uint8 field holds no negative
    number: there the pair is stored as ``rint(255 max(c, 0))``, which is the field where the SOURCE direction lies in the first quadrant, and
    the comparison runs on those pixels (0.1 rad away from the axes), under the same bound."""
    n = 65
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64) - (n - 1) / 2.0
    phi, r = np.arctan2(yy, xx), np.hypot(xx, yy)
    pair = np.stack([np.cos(phi), np.sin(phi)])[:, None].repeat(2, axis=1)                            # [2, D = 2, 65, 65]
    pair = pair.astype(np.float32) if source == "f32" else np.rint(np.clip(pair, 0, 1) * 255).astype(np.uint8)
    geos = [g for g in GEOMETRY if g[0]]
    recs = np.stack([_geo(i, n, n, g) for i, g in enumerate(geos)])
    got = _run(np.stack([pair] * len(geos)), recs, VO.VECTOR, border).astype(np.float64)
    for i, g in enumerate(geos):
        r_src = r / float(np.float32(g[1]))
        where = (r_src >= 8) & (r_src <= 30)
        if source == "u8":
            phi_src = np.angle(np.exp(1j * (phi + np.deg2rad(float(np.float32(g[0]))))))                # the direction stored at the source voxel
            where &= (phi_src > 0.1) & (phi_src < np.pi / 2 - 0.1)
        bound = np.arctan(np.sqrt(0.5) / r_src[where])
        for z in range(2):
            dev = np.angle(np.exp(1j * (np.arctan2(got[i, 1, z], got[i, 0, z]) - phi)))[where]
            opposite = np.angle(np.exp(1j * (np.arctan2(-got[i, 1, z], got[i, 0, z]) - phi)))[where]
            bad = int((np.abs(dev) > bound).sum())
            print(f"radial {source} border {border} {g} plane {z}: {int(where.sum())} pixels, beyond the bound {bad}, largest deviation / bound "
                  f"{np.abs(dev / bound).max():.3f}; with the opposite sign {int((np.abs(opposite) > bound).sum())} beyond")
            assert where.sum() >= (200 if source == "f32" else 40) and bad == 0


# ---- 7. arguments --------------------------------------------------------------------------------------------------------------------------
def test_arguments_are_validated():
    dims = (2, 2, 3, 32, 32)
    t = torch.zeros(dims, dtype=torch.float32, device="cuda")
    marker = torch.full(dims, 7.0, dtype=torch.float32, device="cuda")
    par = torch.from_numpy(np.stack([A.record_f32(0, 32, 32)] * 2).view(np.uint8).copy()).cuda()
    call = lambda src, dst, dims, kind, border, blur, fid=1: _call(src, dst, par, dims, kind, border, blur, 0, 0, fid)
    assert call(t, marker, (2, 1, 6, 32, 32), VO.VECTOR, VO.REFLECT, 0) != 0 and b"pairs" in lib.biu_last_error()      # an odd number of channels
    assert call(t, t, dims, VO.IMAGE, VO.REFLECT, 0) != 0                                                             # in place
    assert call(t, marker, dims, 3, VO.REFLECT, 0) != 0 and b"kind" in lib.biu_last_error()
    assert call(t, marker, dims, VO.IMAGE, 2, 0) != 0 and b"border" in lib.biu_last_error()
    assert call(t, marker, dims, VO.IMAGE, VO.REFLECT, 17) != 0 and b"blur" in lib.biu_last_error()
    assert call(t, marker, (2, 2, 1 << 9, 1 << 10, 1 << 10), VO.MASK, VO.REFLECT, 0) != 0 and b"2^31" in lib.biu_last_error()   # dimensions only
    assert call(t, marker, (1 << 16, 1, 1 << 5, 1 << 5, 1 << 5), VO.MASK, VO.REFLECT, 0) != 0                          # exactly 2^31
    assert call(t, marker, dims, VO.MASK, VO.REFLECT, 0, fid=1 << 28) != 0 and b"field_id" in lib.biu_last_error()
    torch.cuda.synchronize()
    assert bool((marker == 7.0).all())                                                                                # nothing was launched
    assert call(t, marker, dims, VO.VECTOR, VO.CONSTANT, 0, fid=(1 << 28) - 1) == 0
    torch.cuda.synchronize()
    assert bool((marker == 0.0).all())
    aug = A.AugmenterVol(shape=(3, 32, 32))
    recs = aug.draw(0, [0, 1])
    with pytest.raises(ValueError):
        aug({"volume": t}, recs, 0, out={"volume": t})
    with pytest.raises(ValueError):
        aug({"volume": t.half()}, recs, 0)
    with pytest.raises(ValueError):
        aug({"volume": t[:, 0, 0]}, recs, 0)                    # [B, H, W]: not a volume
    with pytest.raises(ValueError):
        aug({"orientation": t[:, 0].contiguous()}, recs, 0)     # [B, D, H, W]: one channel, no pair
    assert aug({"orientation": t, "volume": t[:, 0].contiguous()}, recs, 0)["orientation"].shape == dims
    torch.cuda.synchronize()


# ---- 8. feeder -----------------------------------------------------------------------------------------------------------------------------
def _store(tmp_path, name, n, dhw=(4, 24, 40), seed=0, attrs=None):
    """A mixed store: the volume as bytes, a copy of it, a mask and an orientation pair as float32."""
    fields = {"volume": dhw, "copy": dhw, "mask": dhw, "orientation": (2,) + dhw}
    st = TileStore.create(str(tmp_path / name), n, fields, {"dim_out": list(dhw), **(attrs or {})}, dtypes={"copy": "f32", "mask": "f32", "orientation": "f32"})
    rng = np.random.default_rng(seed)
    st.maps["volume"][:] = rng.integers(0, 256, (n,) + dhw)
    st.maps["copy"][:] = st.maps["volume"][:].astype(np.float32) / np.float32(255)
    st.maps["mask"][:] = rng.random((n,) + dhw) > 0.5
    phi = rng.uniform(0, 2 * np.pi, (n,) + dhw)
    st.maps["orientation"][:] = np.stack([np.cos(phi), np.sin(phi)], axis=1)
    st.flush()
    return st


def _epoch(fd):
    return [{k: v.cpu().clone() for k, v in b.items()} for b in fd]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("border", ["reflect", "constant"])
def test_feeder_with_volume_augmenter(tmp_path, border):
    st = _store(tmp_path, "t", 16, attrs={"scale_limit": [-0.5, 0.0], "rotate_limit": [0, 180]})
    mk = lambda: A.AugmenterVol.from_store(st, seed=5, border=border, kinds={"copy": "mask"})
    assert mk().scale_limit == (-0.5, 0.0) and mk().rotate_limit == (0.0, 180.0) and mk().shape == (4, 24, 40)
    idx = [3, 1, 4, 11, 5, 9, 2, 6, 0, 8, 7, 10, 12, 13, 14, 15]
    fa, fb = DeviceFeeder(st, idx, 4, "cuda", depth=2, augmenter=mk()), DeviceFeeder(st, idx, 4, "cuda", depth=3, augmenter=mk())
    a0, b0 = _epoch(fa), _epoch(fb)
    assert len(a0) == 4 and fa.epoch == 1 and all(v.dtype == torch.float32 for v in a0[0].values())
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a0, b0) for k in x)               # same seed, same epoch: bit for bit
    on_main = _epoch(DeviceFeeder(st, idx, 4, "cuda", augmenter=mk(), augment_stream="main"))
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a0, on_main) for k in x)
    a1, b1 = _epoch(fa), _epoch(fb)
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a1, b1) for k in x)
    assert any(not torch.equal(x["volume"], y["volume"]) for x, y in zip(a0, a1))        # a fresh draw every epoch
    aug, moved, still, changed = mk(), 0, 0, 0
    for b, got in enumerate(a0):
        ids_b = idx[4 * b:4 * b + 4]
        recs = aug.draw(0, ids_b)
        raw = {k: v.cuda() for k, v in st.batch_u8(ids_b).items()}
        want = aug(raw, recs, 0)                                                        # == AugmenterVol.__call__ on the raw batch
        assert all(torch.equal(want[k].cpu(), got[k]) for k in got)
        for j, r in enumerate(recs):
            if int(r["flags"]) & A.ROT_F:
                moved += 1
            else:                                                                       # every field of a sample shares the geometry
                still += 1
                assert torch.equal(got["copy"][j], raw["copy"][j].cpu()) and torch.equal(got["mask"][j], raw["mask"][j].cpu())
                assert torch.equal(got["orientation"][j], raw["orientation"][j].cpu())
                if not int(r["flags"]) & (A.BC_F | A.BLUR_F | A.SHOT_F | A.GAUSS_F):
                    assert torch.equal(got["volume"][j], got["copy"][j])
        changed += int(not torch.equal(raw["mask"].cpu(), got["mask"]))
        norm = (got["orientation"].double() ** 2).sum(1)
        assert float(torch.minimum((norm - 1).abs(), norm.abs()).max()) < 1e-6           # a rotated unit pair stays a unit pair (constant border: or 0)
        assert set(np.unique(got["mask"].numpy())) <= {0.0, 1.0}
    print(f"feeder border {border}: {moved} samples moved, {still} not, {changed} of {len(a0)} batches changed")
    assert moved > 0 and still > 0 and changed > 0
    # validation batches (a feeder without an augmenter) equal the store, in the fields' own dtypes
    for b, got in enumerate(_epoch(DeviceFeeder(st, idx, 4, "cuda"))):
        raw = st.batch_u8(idx[4 * b:4 * b + 4])
        assert all(torch.equal(raw[k], got[k]) and raw[k].dtype == got[k].dtype for k in got)
    with pytest.raises(ValueError):
        DeviceFeeder(st, idx, 4, "cuda", augmenter=A.Augmenter("unet3d"))               # the uint8 augmenter cannot take float fields


# ---- 9. TrainerMo3d ------------------------------------------------------------------------------------------------------------------------
HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "orientation": {"channels": 2, "activation": None, "loss": "TverskyLoss", "weight": 0.5}}


class _Volumes(torch.utils.data.Dataset):
    """The 3-D multi-output item contract: 'volume' (D, H, W) a multiple of 1/255, one float target per head."""
    aug_factor, clip_threshold, scale_limit, rotate_limit, gauss_noise_lims, shot_noise_lims = 1, (0., 99.99), (-0.5, 0), (0, 360), (0.01, 0.1), (0.005, 0.01)
    brightness_contrast, blur_limit, random_rotate, dim_out = (0.1, 0.1), (3, 7), True, (8, 32, 32)

    def __init__(self, n):
        g = torch.Generator().manual_seed(0)
        self.items = []
        for _ in range(n):
            phi = torch.rand((8, 32, 32), generator=g) * 6.2831853
            self.items.append({"volume": torch.round(torch.rand((8, 32, 32), generator=g) * 255) / 255,
                               "mask": (torch.rand((8, 32, 32), generator=g) > 0.5).float(),
                               "orientation": torch.stack([torch.cos(phi), torch.sin(phi)])})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.mark.timeout(600)
def test_trainer_mo3d_with_online_augmentation(tmp_path):
    from bio_image_unet_amd.workflow import TrainerMo3d
    ds = _Volumes(8)
    st = TileStore.from_dataset(str(tmp_path / "mixed"), ds, dtypes={"mask": "f32", "orientation": "f32"})
    assert st.dtypes["volume"] == "u8" and st.fields["orientation"] == (2, 8, 32, 32)
    kw = dict(batch_size=1, n_filter=8, device="cuda")            # 8 volumes, val_split 0.2: one validation volume, so batches of one
    torch.manual_seed(3)
    tr = TrainerMo3d(st, HEADS, 2, save_dir=str(tmp_path / "o"), augment=True, **kw)
    assert isinstance(tr.augmenter, A.AugmenterVol) and tr.augmenter.scale_limit == (-0.5, 0.0) and tr.augmenter.rotate_limit == (0.0, 360.0)
    assert tr.train_loader.augmenter is tr.augmenter and tr.val_loader.augmenter is None
    for b, batch in enumerate(tr.val_loader):                                          # validation sees the raw tiles
        raw = st.batch_u8(tr.val_loader.indices[b:b + 1])
        assert all(torch.equal(batch[k].cpu(), raw[k]) for k in batch)
    assert len(tr.val_loader) == 1 and len(tr.train_loader) == 7
    batch = next(iter(tr.train_loader))
    assert all(v.dtype == torch.float32 for v in batch.values()) and batch["orientation"].shape == (1, 2, 8, 32, 32)
    loss = tr._total_loss(batch, validating=False)
    print(f"TrainerMo3d(augment=True): first loss {float(loss):.6f}")
    assert torch.isfinite(loss)
    tr.start()
    ck = torch.load(str(tmp_path / "o" / "model.pt"), weights_only=False)
    print(f"TrainerMo3d(augment=True): best validation loss after two epochs {float(ck['best_loss']):.6f}")
    assert ck["online_augmentation"] == tr.augmenter.describe() and ck["online_augmentation"]["recipe"] == "mo3d"
    assert torch.isfinite(torch.as_tensor(ck["best_loss"])) and tr.train_loader.epoch == 3
    own = A.AugmenterVol.from_store(st, seed=77, border="constant")
    assert TrainerMo3d(st, HEADS, 1, save_dir=str(tmp_path / "p"), augment=own, **kw).augmenter is own
    with pytest.raises(ValueError):
        TrainerMo3d(st, HEADS, 1, save_dir=str(tmp_path / "q"), augment=A.AugmenterF32(), **kw)
    # without the keyword the checkpoint's key set is exactly what it was before the keyword existed
    plain = TrainerMo3d(st, HEADS, 1, save_dir=str(tmp_path / "r"), **kw)
    assert plain.augmenter is None and plain.train_loader.augmenter is None
    plain.start()
    keys = set(torch.load(str(tmp_path / "r" / "model.pt"), weights_only=False))
    assert keys == {"epoch", "epoch_start", "best_loss", "state_dict", "optimizer", "lr", "loss_function", "loss_params", "time_loss_weight", "n_filter",
                    "use_interpolation", "dilation", "batch_size", "augmentation", "clip_threshold", "scale_limit", "rotate_limit", "gauss_noise_lims",
                    "shot_noise_lims", "blur_limit", "random_rotate", "brightness_contrast", "in_channels", "output_heads"}
    assert keys == set(ck) - {"online_augmentation"}
