"""What rendering training patches out of whole volumes costs (bio_image_unet_amd/augment.py: AugmenterVol.draw_crops / launch_crop,
biu_augment_vol_f32_crop; bio_image_unet_amd/feed.py: VolumeStore, CropFeeder).

    python tools/bench_augment_vol_crop.py [--iters 50] [--rounds 3] [--only kernels|steps] [--out profiles/r11_augment_vol_crop.txt]

kernels : per kind and source, the crop launch out of an arena of larger items next to biu_augment_vol_f32 on stored tiles AT THE SAME OUTPUT
          SHAPE AND RECORD, interleaved in one process (tile, crop, tile, crop ... --rounds times, the median of the rounds): both write the same
          bytes, so the tile launch is the yardstick, and the ratio crop / tile is what the per-sample item costs.  Device events around --iters
          back-to-back launches (launch gaps included), at [1, 1, 128, 256, 256] out of items (136, 288, 320) and at [4, 1, 32, 128, 128] out of
          items (40, 160, 176) (the vector kind: two channels).
steps   : what the user pays.  Synchronised step time of TrainerMo3d (MultiOutputUnet3D(n_filter=64, interpolation) in bf16, batch 1,
          128 x 256 x 256: the cfg5 workload of bench.py with a mask, a distance and an orientation head), A / A / B / C interleaved in one
          process: two DeviceFeeders over a TileStore without augmenter (the spread between two runs of the same thing), one with
          AugmenterVol (augment=True), and a CropFeeder over a VolumeStore of whole volumes (136, 288, 320).  One model and optimizer serve all.

Everything printed is also written to --out.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd._lib import check, lib  # noqa: E402
from bio_image_unet_amd.feed import CropFeeder, DeviceFeeder, TileStore, VolumeStore  # noqa: E402

SIZES = (((1, 128, 256, 256), (136, 288, 320)), ((4, 32, 128, 128), (40, 160, 176)))          # (batch, td, th, tw), the items' (D, H, W)
GEO = dict(angle=17.3, scale=0.7313)
CASES = {            # name: (kind, channels, record keywords)
    "image, gather only": (A.KIND_IMAGE, 1, dict(**GEO)),
    "image, bc + shot + gauss": (A.KIND_IMAGE, 1, dict(shot_s=0.0075, gauss_sigma=0.05, bc=(1.1, 0.05), **GEO)),
    "image, all stages, blur 7": (A.KIND_IMAGE, 1, dict(blur_k=7, shot_s=0.0075, gauss_sigma=0.05, bc=(1.1, 0.05), **GEO)),
    "mask": (A.KIND_MASK, 1, dict(**GEO)),
    "vector": (A.KIND_VECTOR, 2, dict(**GEO)),
}
HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "distance": {"channels": 1, "activation": "sigmoid", "loss": "TverskyLoss", "weight": 0.25},
         "orientation": {"channels": 2, "activation": None, "loss": "TverskyLoss", "weight": 0.5}}


class _Tee:
    def __init__(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.f, self.out = open(path, "w"), sys.stdout

    def write(self, s):
        self.out.write(s)
        self.f.write(s)

    def flush(self):
        self.out.flush()
        self.f.flush()


def _timed(fn, iters, warm=3):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernels(a):
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    print("planes: the planes a lane (a block, where the case blurs) walks in both launches (biu_augment_vol_chunk on the output shape)")
    print(f"{'case':28s} {'output':>20s} {'source':>6s} {'planes':>6s} {'MiB r+w':>8s} {'tile us':>9s} {'crop us':>9s} {'crop/tile':>9s} {'crop GB/s':>9s}")
    for (n, td, th, tw), item in SIZES:
        for name, (kind, c, kw) in CASES.items():
            blur = int(kw.get("blur_k", 0))
            for u8 in (False, True):
                shape, ishape = (n, c, td, th, tw), (n, c) + item          # one item per sample, so no sample finds its neighbour's item in cache
                mk = lambda s: torch.randint(0, 256, s, dtype=torch.uint8, device="cuda") if u8 else torch.rand(s, dtype=torch.float32, device="cuda")
                tiles, arena = mk(shape), mk(ishape).reshape(-1)
                dst = torch.empty(shape, dtype=torch.float32, device="cuda")
                trecs = np.stack([A.record_f32(i, th, tw, **kw) for i in range(n)])
                crecs = np.stack([A.record_vol_crop(i, item[1:], origin=((item[2] - tw) // 2, (item[1] - th) // 2), **kw) for i in range(n)])
                src = np.array([(i * c * item[0] * item[1] * item[2],) + item + ((item[0] - td) // 2,) for i in range(n)], dtype=A.SOURCE_VOL_DTYPE)
                tpar, cpar, csrc = (torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in (trecs, crecs, src))
                tile = lambda i: check(lib.biu_augment_vol_f32(p(tiles), int(u8), p(dst), n, c, td, th, tw, kind, A.BORDER_REFLECT, p(tpar), blur if kind == A.KIND_IMAGE else 0,
                                                               1, i, A.field_id("f"), stream()), "augment_vol_f32")
                crop = lambda i: check(lib.biu_augment_vol_f32_crop(p(arena), int(u8), arena.numel(), p(dst), n, c, td, th, tw, kind, A.BORDER_REFLECT, p(cpar), p(csrc),
                                                                    0.0, blur if kind == A.KIND_IMAGE else 0, 1, i, A.field_id("f"), stream()), "augment_vol_f32_crop")
                t_us, c_us = [], []
                for _ in range(a.rounds):
                    t_us.append(_timed(tile, a.iters))
                    c_us.append(_timed(crop, a.iters))
                t_med, c_med = statistics.median(t_us), statistics.median(c_us)
                nbytes = dst.numel() * (tiles.element_size() + 4)
                planes = lib.biu_augment_vol_chunk(*shape, kind, blur, int(dst.data_ptr() % 16 == 0))
                print(f"{name:28s} {str(list(shape)):>20s} {'u8' if u8 else 'f32':>6s} {planes:6d} {nbytes / 2 ** 20:8.2f} {t_med:9.2f} {c_med:9.2f} "
                      f"{c_med / t_med:9.3f} {nbytes / c_med / 1e3:9.1f}", flush=True)


def _fill(rng, shape):
    phi = rng.random(shape, dtype=np.float32) * np.float32(2 * np.pi)
    return {"volume": rng.integers(0, 256, shape, dtype=np.uint8), "mask": (rng.random(shape, dtype=np.float32) > 0.5).astype(np.float32),
            "distance": rng.random(shape, dtype=np.float32), "orientation": np.stack([np.cos(phi), np.sin(phi)])}


def _stores(tmp, dhw, item, n_tiles=6, n_items=2, aug_factor=3):
    rng = np.random.default_rng(0)
    f32 = {"mask": "f32", "distance": "f32", "orientation": "f32"}
    tiles = TileStore.create(os.path.join(tmp, "tiles"), n_tiles, {"volume": dhw, "mask": dhw, "distance": dhw, "orientation": (2,) + dhw},
                             {"dim_out": list(dhw)}, dtypes=f32)
    for i in range(n_tiles):
        for k, v in _fill(rng, dhw).items():
            tiles.maps[k][i] = v
    tiles.flush()
    vols = VolumeStore.create(os.path.join(tmp, "volumes"), [item] * n_items, {"volume": 1, "mask": 1, "distance": 1, "orientation": 2},
                              {"dim_out": list(dhw), "aug_factor": aug_factor, "nan_to_val": 0.0}, dtypes={"volume": "u8", **f32},
                              squeeze={"volume": True, "mask": True, "distance": True})
    for i in range(n_items):
        for k, v in _fill(rng, item).items():
            vols.put(i, k, v)
    vols.flush()
    return tiles, vols


def steps(a):
    from bio_image_unet_amd import MultiOutputUnet3D
    from bio_image_unet_amd.workflow import TrainerMo3d
    dhw, item = SIZES[0][0][1:], SIZES[0][1]
    with tempfile.TemporaryDirectory() as tmp:
        st, vs = _stores(tmp, dhw, item)
        torch.manual_seed(0)
        tr = TrainerMo3d(st, HEADS, 1, network=MultiOutputUnet3D, use_interpolation=True, batch_size=1, n_filter=64, val_split=0.0,
                         save_dir=os.path.join(tmp, "out"), device="cuda")
        tr.model.set_compute_dtype(torch.bfloat16)
        idx = tr.train_loader.indices
        feeders = {"A1 (TileStore, no augmenter)": DeviceFeeder(st, idx, 1, "cuda"), "A2 (TileStore, no augmenter)": DeviceFeeder(st, idx, 1, "cuda"),
                   "B  (TileStore, augment=True)": DeviceFeeder(st, idx, 1, "cuda", augmenter=A.AugmenterVol.from_store(st, seed=1)),
                   "C  (VolumeStore, CropFeeder)": CropFeeder(vs, range(len(vs)), 1, "cuda", A.AugmenterVol.from_store(vs, seed=1))}
        times = {k: [] for k in feeders}
        for rnd in range(a.rounds + 1):                          # round 0 warms every shape up and is dropped
            for k, fd in feeders.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for batch in fd:
                    loss = tr._total_loss(batch, validating=False)
                    tr.optimizer.zero_grad()
                    loss.backward()
                    tr.optimizer.clip_grad_norm_(1.0)
                    tr.optimizer.step()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if rnd:
                        times[k].append((t1 - t0) * 1e3)
                    t0 = t1
        print(f"TrainerMo3d MultiOutputUnet3D n_filter=64 interpolation bf16 batch 1 {dhw}, whole volumes {item}: synchronised step time, ms, "
              f"{len(times[k])} steps per variant")
        for k, v in times.items():
            v = sorted(v)
            print(f"  {k:30s} median {statistics.median(v):8.3f}   min {v[0]:8.3f}   max {v[-1]:8.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["kernels", "steps"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_augment_vol_crop.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    sys.stdout = _Tee(a.out)
    shown = [v for i, v in enumerate(sys.argv[1:], 1) if v != "--out" and sys.argv[i - 1] != "--out"]      # where the copy goes is no part of the measurement
    print("python tools/bench_augment_vol_crop.py " + " ".join(shown))
    for mode, fn in (("kernels", kernels), ("steps", steps)):
        if a.only in (None, mode):
            print(f"\n== {mode} ==", flush=True)
            fn(a)


if __name__ == "__main__":
    main()
