"""One SHA-256 per case of the output of the four float augmentation entry points (biu_augment_f32, biu_augment_f32_crop, biu_augment_vol_f32,
biu_augment_vol_f32_crop), to hold two builds of the library to each other byte for byte:

    BIU_LIB_PATH=tools/variants/libbiu_<name>.so python tools/digest_augment.py > a.txt;  python tools/digest_augment.py > b.txt;  diff a.txt b.txt

Small fields throughout, but for the three `chunk` cases of each 3-D entry point: a lane (a block) walks more than one plane only in a launch
of 2048 blocks and more, so these are the smallest fields with two planes per chunk and a short last chunk."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd._lib import check, lib  # noqa: E402

IMAGE, MASK, VECTOR = 0, 1, 2
SEED, EPOCH, FID = 0x1234567890ABCDEF, 3, 5
PLANES = [((72, 68), False), ((72, 68), True), ((70, 61), False)]      # (h, w), dst one float off a 16-byte boundary; partial 64-tiles in all
p = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
bytes_of = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def field(shape, source, rng, nan=False):
    if source == "u8":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    f = rng.random(shape).astype(np.float32)
    if nan:
        f[rng.random(shape) < 0.05] = np.nan
        f[..., -1, :] = np.nan
    return f


def run(name, shape, off, call):
    """``call(dst)`` on a canary-filled ``dst`` of ``shape``, ``off``: one float off a 16-byte boundary -> prints the digest."""
    n = int(np.prod(shape))
    whole = torch.full((n + 4,), 7.0, dtype=torch.float32, device="cuda")
    dst = whole[1:1 + n] if off else whole[:n]
    check(call(dst), name)
    torch.cuda.synchronize()
    print(name, "x".join(map(str, shape)), "off" if off else "", hashlib.sha256(dst.cpu().numpy().tobytes()).hexdigest(), flush=True)


def records(make, kind, blur, **first):
    """Geometry and stages, singly and together; ``blur``: three of the samples blur, with 3 and the maximum, the others stay plain."""
    b = (lambda k: dict(blur_k=k)) if blur and kind == IMAGE else (lambda k: {})
    return np.stack([make(0, **first), make(1, angle=33.7, **b(3)), make(2, scale=0.83), make(3, angle=151.0, scale=1.17, shot_s=0.01, gauss_sigma=0.03,
                     bc=(1.05, -0.02), **b(A.MAX_BLUR)), make(4, shot_s=0.004), make(5, gauss_sigma=0.07, **b(A.MAX_BLUR)), make(6, bc=(1.1, -0.05)), make(7)])


def two_d(source, kind, hw, off, blur):
    (h, w), rng = hw, np.random.default_rng(1)
    tag = f"{source} kind {kind} blur {blur}"
    recs = records(lambda j, **kw: A.record_f32(j, h, w, **kw), kind, blur, rot_k=2, shift=(w + 5, -(2 * h + 3)))
    n, mb = len(recs), A.MAX_BLUR if blur and kind == IMAGE else 0
    src, par = torch.from_numpy(field((n, 2, h, w), source, rng)).cuda(), bytes_of(recs)
    run(f"augment_f32 {tag}", (n, 2, h, w), off,
        lambda dst: lib.biu_augment_f32(p(src), int(source == "u8"), p(dst), n, 2, h, w, kind, p(par), mb, SEED, EPOCH, FID, stream()))
    # items of differing size, the first smaller than the tile (it wraps more than once); NaN in float targets; sample 6 names no part of the arena
    items = [(33, 27), (70, 90), (50, 130), (72, 68)]
    arena = np.concatenate([field((2,) + it, source, rng, nan=kind != IMAGE).reshape(-1) for it in items])
    offs = np.concatenate([[0], np.cumsum([2 * a * b for a, b in items])])
    recs = records(lambda j, **kw: A.record_crop(j, items[j % 4], **kw), kind, blur, rot_k=3, origin=(140, 77))
    srcs = np.array([(offs[j % 4], *items[j % 4]) for j in range(n)], dtype=A.SOURCE_DTYPE)
    srcs[6]["offset"] = arena.size - 10
    a, par, srcs = torch.from_numpy(arena).cuda(), bytes_of(recs), bytes_of(srcs)
    run(f"augment_f32_crop {tag}", (n, 2, h, w), off, lambda dst: lib.biu_augment_f32_crop(
        p(a), int(source == "u8"), a.numel(), p(dst), n, 2, h, w, kind, p(par), p(srcs), -2.0, mb, SEED, EPOCH, FID, stream()))


def three_d(source, kind, border, tile, off, blur, n=None, channels=2, chunked=False):
    (d, h, w), rng = tile, np.random.default_rng(2)
    tag = f"{source} kind {kind} border {border} blur {blur}" + (" chunk" if chunked else "")
    recs = records(lambda j, **kw: A.record_f32(j, h, w, **kw), kind, blur, shift=(3, -2))
    n = n or len(recs)
    recs, mb = np.resize(np.roll(recs, -3 * chunked), n), A.MAX_BLUR if blur and kind == IMAGE else 0       # chunked: the full chain first
    if chunked:
        took = lib.biu_augment_vol_chunk(n, channels, d, h, w, kind, mb, 1)
        units = channels * d // (2 if kind == VECTOR else 1)
        assert took > 1 and units % took, (took, units)
    src, par = torch.from_numpy(field((n, channels, d, h, w), source, rng)).cuda(), bytes_of(recs)
    run(f"augment_vol_f32 {tag}", (n, channels, d, h, w), off, lambda dst: lib.biu_augment_vol_f32(
        p(src), int(source == "u8"), p(dst), n, channels, d, h, w, kind, border, p(par), mb, SEED, EPOCH, FID, stream()))
    # items of differing size, the first smaller than the tile in the plane (it reflects); z0 > 0; NaN; sample 6 names no part of the arena
    items = [(d + 4, h + 3, w + 8)] if chunked else [(d + 2, 33, 27), (d + 1, 70, 90), (d + 3, 50, 130), (d, h, w)]
    m = len(items)
    arena = np.concatenate([field((channels,) + it, source, rng, nan=kind != IMAGE and not chunked).reshape(-1) for it in items])
    offs = np.concatenate([[0], np.cumsum([channels * a * b * c for a, b, c in items])])
    recs = records(lambda j, **kw: A.record_vol_crop(j, items[j % m][1:], **kw), kind, blur, origin=(5, 3))
    recs = np.resize(np.roll(recs, -3 * chunked), n)
    srcs = np.array([(offs[j % m], *items[j % m], items[j % m][0] - d) for j in range(n)], dtype=A.SOURCE_VOL_DTYPE)
    if not chunked:
        srcs[6]["z0"] += 1                                                      # the crop's last plane lies behind the item
    a, par, srcs = torch.from_numpy(arena).cuda(), bytes_of(recs), bytes_of(srcs)
    run(f"augment_vol_f32_crop {tag}", (n, channels, d, h, w), off, lambda dst: lib.biu_augment_vol_f32_crop(
        p(a), int(source == "u8"), a.numel(), p(dst), n, channels, d, h, w, kind, border, p(par), p(srcs), -2.0, mb, SEED, EPOCH, FID, stream()))


if __name__ == "__main__":
    for source in ("f32", "u8"):
        for kind in (IMAGE, MASK, VECTOR):
            for hw, off in PLANES:
                for blur in ((False, True) if kind == IMAGE else (False,)):
                    two_d(source, kind, hw, off, blur)
                    for border in (A.BORDER_REFLECT, A.BORDER_CONSTANT):
                        three_d(source, kind, border, (3,) + hw, off, blur, channels=4 if kind == VECTOR else 2)     # VECTOR: two pairs
    # more than one plane per lane (IMAGE, VECTOR: 255 planes, two per lane, the last alone) and per block (16 samples x 255 planes of 8 x 8)
    three_d("f32", IMAGE, A.BORDER_REFLECT, (255, 128, 128), False, False, n=1, channels=1, chunked=True)
    three_d("u8", VECTOR, A.BORDER_CONSTANT, (255, 128, 128), False, False, n=1, channels=2, chunked=True)
    three_d("f32", IMAGE, A.BORDER_REFLECT, (255, 8, 8), False, True, n=16, channels=1, chunked=True)
