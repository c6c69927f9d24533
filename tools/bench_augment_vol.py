"""What on-device augmentation of volumes costs (bio_image_unet_amd/augment.py: AugmenterVol, biu_augment_vol_f32).

    python tools/bench_augment_vol.py [--iters 50] [--rounds 3] [--only hbm|kernels|steps] [--out profiles/r10_augment_vol.txt]

hbm     : what tools/hbm_probe.py reports on this box (fill, copy, read-reduce with plain torch kernels): the yardstick for the rates below.
kernels : one launch per field per batch, timed with device events around --iters back-to-back launches (launch gaps included), per kind
          (IMAGE gather only, with the per-voxel stages, and with the blur; MASK; VECTOR), float32 and uint8 sources, both borders for the image,
          at [4, 1, 32, 128, 128] and [1, 1, 128, 256, 256] (the vector kind: two channels).  Printed with the bytes the algorithm needs (field
          read once + written once), the rate that makes, and the planes a lane or block walks in that launch.
steps   : what the user pays.  Synchronised step time of TrainerMo3d (MultiOutputUnet3D(n_filter=64, interpolation) in bf16, batch 1,
          128 x 256 x 256: the cfg5 workload of bench.py with a mask, a distance and an orientation head) fed from a mixed u8 / f32 TileStore,
          A / A / B interleaved in one process: two feeders without augmenter (the spread between two runs of the same thing) and one with.
          One model and optimizer serve all three.

Everything printed is also written to --out.
"""
import argparse
import ctypes as C
import os
import runpy
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
from bio_image_unet_amd.feed import DeviceFeeder, TileStore  # noqa: E402

SIZES = ((4, 32, 128, 128), (1, 128, 256, 256))          # batch, D, H, W
GEO = dict(angle=17.3, scale=0.7313)
CASES = {            # name: (kind, channels, record keywords, borders)
    "image, gather only": (A.KIND_IMAGE, 1, dict(**GEO), ("reflect", "constant")),
    "image, bc + shot + gauss": (A.KIND_IMAGE, 1, dict(shot_s=0.0075, gauss_sigma=0.05, bc=(1.1, 0.05), **GEO), ("reflect",)),
    "image, bc + blur 5": (A.KIND_IMAGE, 1, dict(blur_k=5, bc=(1.1, 0.05), **GEO), ("reflect",)),
    "image, all stages, blur 7": (A.KIND_IMAGE, 1, dict(blur_k=7, shot_s=0.0075, gauss_sigma=0.05, bc=(1.1, 0.05), **GEO), ("reflect",)),
    "mask": (A.KIND_MASK, 1, dict(**GEO), ("reflect",)),
    "vector": (A.KIND_VECTOR, 2, dict(**GEO), ("reflect",)),
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


def _launch(src, dst, par, recs, kind, border, epoch):
    n, c, d, h, w = src.shape
    blurs = recs["blur_k"][(recs["flags"] & A.BLUR_F) != 0]
    check(lib.biu_augment_vol_f32(C.c_void_p(src.data_ptr()), int(src.dtype == torch.uint8), C.c_void_p(dst.data_ptr()), n, c, d, h, w, kind,
                                  A.BORDERS_VOL[border], C.c_void_p(par.data_ptr()), int(blurs.max()) if kind == A.KIND_IMAGE and len(blurs) else 0,
                                  1, epoch, A.field_id("f"), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "augment_vol_f32")


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
    print("planes: the planes a lane (a block, where the case blurs) walks with one set of taps in this launch (biu_augment_vol_chunk)")
    print(f"{'case':28s} {'field':>20s} {'border':>8s} {'source':>6s} {'planes':>6s} {'MiB r+w':>8s} {'us/launch':>10s} {'GB/s':>8s}")
    for n, d, h, w in SIZES:
        for name, (kind, c, kw, borders) in CASES.items():
            recs = np.stack([A.record_f32(i, h, w, **kw) for i in range(n)])
            par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
            for border in borders:
                for u8 in (False, True):
                    shape = (n, c, d, h, w)
                    src = (torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda") if u8 else torch.rand(shape, dtype=torch.float32, device="cuda"))
                    dst = torch.empty(shape, dtype=torch.float32, device="cuda")
                    us = _timed(lambda i: _launch(src, dst, par, recs, kind, border, i), a.iters)
                    nbytes = src.numel() * (src.element_size() + 4)
                    planes = lib.biu_augment_vol_chunk(*shape, kind, int(kw.get("blur_k", 0)), int(dst.data_ptr() % 16 == 0))
                    print(f"{name:28s} {str(list(shape)):>20s} {border:>8s} {'u8' if u8 else 'f32':>6s} {planes:6d} {nbytes / 2 ** 20:8.2f} {us:10.2f} "
                          f"{nbytes / us / 1e3:8.1f}", flush=True)


def _make_store(tmp, n, dhw):
    fields = {"volume": dhw, "mask": dhw, "distance": dhw, "orientation": (2,) + dhw}
    st = TileStore.create(os.path.join(tmp, "mo3d"), n, fields, {"dim_out": list(dhw)}, dtypes={"mask": "f32", "distance": "f32", "orientation": "f32"})
    rng = np.random.default_rng(0)
    for i in range(n):
        phi = rng.random(dhw, dtype=np.float32) * np.float32(2 * np.pi)
        st.maps["volume"][i] = rng.integers(0, 256, dhw, dtype=np.uint8)
        st.maps["mask"][i] = rng.random(dhw, dtype=np.float32) > 0.5
        st.maps["distance"][i] = rng.random(dhw, dtype=np.float32)
        st.maps["orientation"][i] = np.stack([np.cos(phi), np.sin(phi)])
    st.flush()
    return st


def steps(a):
    from bio_image_unet_amd import MultiOutputUnet3D
    from bio_image_unet_amd.workflow import TrainerMo3d
    dhw = (128, 256, 256)
    with tempfile.TemporaryDirectory() as tmp:
        st = _make_store(tmp, 6, dhw)
        torch.manual_seed(0)
        tr = TrainerMo3d(st, HEADS, 1, network=MultiOutputUnet3D, use_interpolation=True, batch_size=1, n_filter=64, val_split=0.0,
                         save_dir=os.path.join(tmp, "out"), device="cuda")
        tr.model.set_compute_dtype(torch.bfloat16)
        idx = tr.train_loader.indices
        feeders = {"A1 (no augmenter)": DeviceFeeder(st, idx, 1, "cuda"), "A2 (no augmenter)": DeviceFeeder(st, idx, 1, "cuda"),
                   "B  (augmenter)": DeviceFeeder(st, idx, 1, "cuda", augmenter=A.AugmenterVol.from_store(st, seed=1))}
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
        print(f"TrainerMo3d MultiOutputUnet3D n_filter=64 interpolation bf16 batch 1 {dhw}: synchronised step time, ms, {len(times[k])} steps per variant")
        for k, v in times.items():
            v = sorted(v)
            print(f"  {k:20s} median {statistics.median(v):8.3f}   min {v[0]:8.3f}   max {v[-1]:8.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["hbm", "kernels", "steps"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_augment_vol.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    sys.stdout = _Tee(a.out)
    shown = [v for i, v in enumerate(sys.argv[1:], 1) if v != "--out" and sys.argv[i - 1] != "--out"]      # where the copy goes is no part of the measurement
    print("python tools/bench_augment_vol.py " + " ".join(shown))
    for mode, fn in (("hbm", lambda a: runpy.run_path(os.path.join(ROOT, "tools", "hbm_probe.py"))), ("kernels", kernels), ("steps", steps)):
        if a.only in (None, mode):
            print(f"\n== {mode} ==", flush=True)
            fn(a)


if __name__ == "__main__":
    main()
