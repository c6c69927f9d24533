"""The byte kernels of ``csrc/biu_io.hip`` through the C ABI, value for value: the uint8 widening (``biu_from_nchw_u8``, ``biu_u8_to_f32``)
against the correctly rounded quotient bit for bit, ``biu_quantize_u8`` against numpy's truncating cast, and ``biu_stitch_add`` /
``biu_stitch_finish`` in uint8 mode (exact integer means) and in float mode (inputs chosen so that every product and sum is exact in fp32
and only the final division rounds).  References are numpy float32 / integer / float64 on the host."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bio_image_unet_amd._lib import BIU_BF16, BIU_F32  # noqa: E402
from tests.gpu_util import Dev, check, lib, ptr, stream  # noqa: E402

CODES = np.arange(256, dtype=np.uint8)
QUOT = CODES.astype(np.float32) / np.float32(255)             # the reference's `tile.astype('float32') / 255`


def bf16_bits(x):
    """Round-to-nearest-even bf16 of finite float32 values, as int16 bit patterns."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# uint8 -> float: one value for one byte, whatever its route
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_io_from_nchw_u8_is_the_rounded_quotient(dtype):
    n, c, d, h, w = 2, 3, 4, 5, 6
    i = np.arange(n * c * d * h * w)
    src = ((7 * i + 3 * (i // (c * d * h * w))) % 256).astype(np.uint8).reshape(n, c, d, h, w)      # 7 is odd: a run of 256 holds every code once
    assert len(np.unique(src)) == 256
    for a in range(n):                                           # no two channels, and no two positions a layout slip could swap, hold equal data
        flat = src[a].reshape(c, -1)
        assert all(not np.array_equal(flat[p], flat[q]) for p in range(c) for q in range(p))
    dst = Dev(shape=(n, c, d, h, w), dtype=dtype, pitch=c + 5, c0=2)
    check(lib.biu_from_nchw_u8(ptr(torch.from_numpy(src).cuda()), 255.0, dst.a(), BIU_F32 if dtype == "f32" else BIU_BF16, stream()), "from_nchw_u8")
    torch.cuda.synchronize()
    want = np.ascontiguousarray(QUOT[src].transpose(0, 2, 3, 4, 1))             # [N, D, H, W, C]: the NCDHW value at its channels-last place
    if dtype == "f32":
        got = dst.buf[..., 2:2 + c].cpu().numpy()
        differ = np.unique(src.transpose(0, 2, 3, 4, 1)[bits(got) != bits(want)])
        assert len(differ) == 0, f"{len(differ)} codes differ from float32(k) / 255: {differ[:12].tolist()} ..."
    else:
        got = dst.buf[..., 2:2 + c].contiguous().view(torch.int16).cpu().numpy()
        assert np.array_equal(got, bf16_bits(want))
    outside = torch.cat([dst.buf[..., :2], dst.buf[..., 2 + c:]], dim=-1)
    assert bool(torch.isnan(outside).all())


def test_io_u8_to_f32_is_the_rounded_quotient():
    from bio_image_unet_amd.feed import u8_to_float
    src = (np.arange(1000) % 256).astype(np.uint8)
    dev = torch.from_numpy(src).cuda()
    out = torch.full((1000 + 8,), float("nan"), device="cuda")
    check(lib.biu_u8_to_f32(ptr(dev), 255.0, ptr(out), 1000, stream()), "u8_to_f32")
    got = out.cpu().numpy()
    differ = np.unique(src[bits(got[:1000]) != bits(QUOT[src])])
    assert len(differ) == 0, f"{len(differ)} codes differ from float32(k) / 255: {differ[:12].tolist()} ..."
    assert np.isnan(got[1000:]).all()
    assert got[255] == np.float32(1.0) and got[0] == 0.0                           # binary targets (0 / 255) are exactly 0 and 1
    assert np.array_equal(bits(u8_to_float(dev).cpu().numpy()), bits(QUOT[src]))


def test_io_one_value_for_one_pixel(tmp_path):
    """The host item, the target path, the network-input path and an identity pass of either float augmenter give equal floats."""
    from bio_image_unet_amd import augment as A
    from bio_image_unet_amd.feed import TileStore, u8_to_float
    st = TileStore.create(str(tmp_path / "s"), 2, {"image": (16, 16)})
    st.maps["image"][0] = CODES.reshape(16, 16)
    st.maps["image"][1] = CODES[::-1].reshape(16, 16)
    st.flush()
    host = torch.stack([st[0]["image"], st[1]["image"]]).numpy()
    assert np.array_equal(bits(host), bits(QUOT[np.asarray(st.maps["image"])]))
    batch = st.batch_u8([0, 1])["image"].cuda()
    assert np.array_equal(bits(u8_to_float(batch).cpu().numpy()), bits(host))
    dst = Dev(shape=(2, 1, 1, 16, 16), dtype="f32")
    check(lib.biu_from_nchw_u8(ptr(batch), 255.0, dst.a(), BIU_F32, stream()), "from_nchw_u8")
    assert np.array_equal(bits(dst.get().numpy().reshape(2, 16, 16)), bits(host))
    recs = np.stack([A.record_f32(i, 16, 16) for i in range(2)])
    flat = A.AugmenterF32(shape=(16, 16))({"image": batch, "mask": batch.clone()}, recs, 0)
    assert np.array_equal(bits(flat["image"].cpu().numpy()), bits(host)) and np.array_equal(bits(flat["mask"].cpu().numpy()), bits(host))
    vol = A.AugmenterVol(shape=(1, 16, 16))({"volume": batch.view(2, 1, 16, 16).contiguous()}, recs, 0)
    assert np.array_equal(bits(vol["volume"].cpu().numpy().reshape(2, 16, 16)), bits(host))


# ---------------------------------------------------------------------------------------------------------------------------------
# float -> uint8
# ---------------------------------------------------------------------------------------------------------------------------------
def _quantize(p):
    src = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).cuda()
    out = torch.full((src.numel() + 16,), 7, dtype=torch.uint8, device="cuda")
    check(lib.biu_quantize_u8(ptr(src), 255.0, ptr(out), src.numel(), stream()), "quantize_u8")
    got = out.cpu().numpy()
    assert (got[src.numel():] == 7).all()
    return got[:src.numel()]


def test_io_quantize_u8_truncates_like_numpy():
    """``(p * 255).astype('uint8')`` bit for bit: at every code's own float, its neighbours one and two ulp away, and across [0, 1]."""
    f32 = np.float32
    centre = (CODES.astype(np.float64) / 255).astype(f32)
    up1, dn1 = np.nextafter(centre, f32(2)), np.nextafter(centre, f32(-1))
    near = np.concatenate([centre, up1, np.nextafter(up1, f32(2)), dn1, np.nextafter(dn1, f32(-1))])
    near = near[(near >= 0) & (near <= 1)]                                   # the numpy cast is defined inside [0, 255] only
    assert len(near) == 5 * 256 - 4
    uniform = np.random.default_rng(5).random(100_000, dtype=f32)
    p = np.concatenate([near, uniform, np.array([1.0, 0.0], dtype=f32)])
    want = (p * f32(255)).astype(np.uint8)
    got = _quantize(p)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} of {len(p)} differ, first p = {p[bad[:4]].tolist()} got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}"
    assert got[len(near) + len(uniform)] == 255
    # truncation is not rounding: these inputs tell them apart
    assert int((np.rint(p * f32(255)).astype(np.uint8) != want).sum()) > 40_000
    # the kernel's own clamp
    low = np.array([-1e-45, -1e-3, -0.5, -1.0, -300.0, -3e38], dtype=f32)
    high = np.array([np.nextafter(f32(1), f32(2)), 1.001, 1.5, 2.0, 300.0, 3e38], dtype=f32)
    assert (_quantize(low) == 0).all() and (_quantize(high) == 255).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# stitching
# ---------------------------------------------------------------------------------------------------------------------------------
VOL, PATCH = (5, 11, 13), (4, 6, 7)
# overlaps 2, 3 and 4 deep; (3, 8, 9) and (2, 6, 8) stick out of the volume on the high side of every axis; some voxels stay untouched
ORIGINS = [(0, 0, 0), (1, 2, 3), (0, 3, 2), (1, 1, 1), (3, 8, 9), (2, 6, 8), (2, 7, 9)]


def _place(origin):
    """(volume slices, patch slices) of the part of a patch at ``origin`` that lies inside the volume."""
    ext = [min(o + p, v) - o for o, p, v in zip(origin, PATCH, VOL)]
    return tuple(slice(o, o + e) for o, e in zip(origin, ext)), tuple(slice(0, e) for e in ext)


def _coverage():
    cnt = np.zeros(VOL, dtype=np.int64)
    for o in ORIGINS:
        cnt[_place(o)[0]] += 1
    return cnt


def test_io_stitch_geometry_is_what_the_cases_need():
    cnt = _coverage()
    assert {0, 1, 2, 3, 4} <= set(np.unique(cnt).tolist())
    for ax in range(3):
        assert any(o[ax] + PATCH[ax] > VOL[ax] for o in ORIGINS)


def _stitch(patches, weights, channels, layers, set_, out_u8, dtype):
    d, h, w = VOL
    acc = torch.zeros((layers, channels, d, h, w), dtype=torch.float32, device="cuda")
    wsum = torch.zeros((layers, d, h, w), dtype=torch.float32, device="cuda")
    keep = []
    for i, (o, p) in enumerate(zip(ORIGINS, patches)):
        pt = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        wt = torch.from_numpy(np.ascontiguousarray(weights[i])).cuda() if weights is not None else None
        keep += [pt, wt]
        layer = i % layers
        check(lib.biu_stitch_add(ptr(pt), int(dtype == np.uint8), ptr(wt), channels, *PATCH, ptr(acc[layer]), ptr(wsum[layer]), d, h, w,
                                 o[0], o[1], o[2], set_, stream()), "stitch_add")
    out = torch.full((channels * d * h * w + 32,), 9, dtype=torch.uint8 if out_u8 else torch.float32, device="cuda")
    check(lib.biu_stitch_finish(ptr(acc), ptr(wsum), layers, channels, d * h * w, ptr(out), int(out_u8), stream()), "stitch_finish")
    res = out.cpu().numpy()
    assert (res[channels * d * h * w:] == 9).all()
    return res[:channels * d * h * w].reshape((channels,) + VOL), wsum.cpu().numpy()


@pytest.mark.parametrize("channels", [1, 2])
def test_io_stitch_u8_sum_over_count(channels):
    """One layer, ``set = 0``, no weight plane: the integer mean ``sum // count`` of the overlapping uint8 patches, 0 where none lies."""
    rng = np.random.default_rng(10 + channels)
    patches = [rng.integers(0, 256, size=(channels,) + PATCH, dtype=np.uint8) for _ in ORIGINS]
    patches[0][:] = 255                                              # 255 + 255 + ... : the largest sums
    total, cnt = np.zeros((channels,) + VOL, dtype=np.int64), _coverage()
    for o, p in zip(ORIGINS, patches):
        vs, ps = _place(o)
        total[(slice(None),) + vs] += p[(slice(None),) + ps]
    want = np.where(cnt > 0, total // np.maximum(cnt, 1), 0).astype(np.uint8)
    got, wsum = _stitch(patches, None, channels, 1, 0, True, np.uint8)
    assert np.array_equal(wsum[0], cnt.astype(np.float32))
    assert np.array_equal(got, want)
    assert (got[:, cnt == 0] == 0).all() and (cnt == 0).any()


@pytest.mark.parametrize("channels", [1, 2])
def test_io_stitch_u8_three_layers_nanmean(channels):
    """``set = 1`` into layer ``i % 3`` (the three-layer buffer of unet3d/predict.py:173-195), then the mean over the layers that hold a value."""
    rng = np.random.default_rng(20 + channels)
    patches = [rng.integers(0, 256, size=(channels,) + PATCH, dtype=np.uint8) for _ in ORIGINS]
    buf = np.full((3, channels) + VOL, np.nan)
    for i, (o, p) in enumerate(zip(ORIGINS, patches)):
        vs, ps = _place(o)
        buf[(i % 3, slice(None)) + vs] = p[(slice(None),) + ps]
    held = ~np.isnan(buf[:, 0])
    assert {0, 1, 2, 3} <= set(np.unique(held.sum(0)).tolist())
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # mean of an all-NaN column: the untouched voxels
            mean = np.nanmean(buf, axis=0)
    want = np.where(np.isnan(mean), 0, mean).astype(np.uint8)        # (the numpy cast of NaN is undefined; the kernel writes 0 there)
    got, wsum = _stitch(patches, None, channels, 3, 1, True, np.uint8)
    assert np.array_equal(wsum, held.astype(np.float32))
    assert np.array_equal(got, want)
    assert (got[:, held.sum(0) == 0] == 0).all()


@pytest.mark.parametrize("channels", [1, 2])
def test_io_stitch_float_weighted_blend(channels):
    """Patches on the 2^-10 grid and weights on the 1/16 grid: every product (a multiple of 2^-14 below 1) and every sum (below 8) is exact
    in fp32, so the only rounding is the final division: within 1 fp32 ulp of the float64 quotient, exactly 0 where the weights sum to 0."""
    rng = np.random.default_rng(30 + channels)
    patches = [(rng.integers(0, 1024, size=(channels,) + PATCH) / 1024).astype(np.float32) for _ in ORIGINS]
    weights = [(rng.integers(0, 17, size=PATCH) / 16).astype(np.float32) for _ in ORIGINS]
    for wt in weights:
        wt[:, 2, :] = 0                                              # a zero row inside every plane
    acc, ws = np.zeros((channels,) + VOL), np.zeros(VOL)
    acc32, ws32 = acc.astype(np.float32), ws.astype(np.float32)
    for o, p, wt in zip(ORIGINS, patches, weights):
        vs, ps = _place(o)
        prod = p.astype(np.float64)[(slice(None),) + ps] * wt.astype(np.float64)[ps]
        assert np.array_equal(prod, prod.astype(np.float32).astype(np.float64))                    # exact products ...
        acc[(slice(None),) + vs] += prod
        ws[vs] += wt[ps]
        acc32[(slice(None),) + vs] += p[(slice(None),) + ps] * wt[ps]
        ws32[vs] += wt[ps]
    assert np.array_equal(acc, acc32.astype(np.float64)) and np.array_equal(ws, ws32.astype(np.float64))    # ... and exact sums, in fp32
    cnt = _coverage()
    dead = (cnt > 0) & (ws == 0)
    interior = dead[1:-1, 1:-1, 1:-1]
    assert interior.any(), "a covered voxel inside the volume must have weight 0"
    q = np.where(ws > 0, acc / np.where(ws > 0, ws, 1), 0)
    got, wsum = _stitch(patches, weights, channels, 1, 0, False, np.float32)
    assert np.array_equal(wsum[0], ws32)
    ulp = np.spacing(np.abs(q).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - q) / ulp
    print(f"stitch float blend, {channels} channel(s): worst deviation {err.max():.3f} ulp")
    assert err.max() <= 1.0
    assert (got[:, ws == 0] == 0).all() and not np.signbit(got[:, ws == 0]).any()
