"""What on-device augmentation costs (bio_image_unet_amd/augment.py, biu_augment_u8).

    python tools/bench_augment.py kernels [--config NAME] [--iters 200]
    python tools/bench_augment.py steps   [--rounds 6] [--family 2d|3d]
    python tools/bench_augment.py torch   [--iters 50]

kernels : one launch per field per batch, timed with device events around --iters back-to-back launches (launch gaps included), for
          "unet" on 4 x 1 x 256^2 and 16 x 1 x 512^2 with the blur gate of every sample forced on and off, and "unet3d" on 4 x 128^3.
          Every other stage of the recipe is on.  Printed with the bytes the algorithm needs (field read once + written once) and
          their share of the HBM peak.  ``--config NAME`` runs one configuration only: the kernel time proper comes from
          ``rocprofv3 --kernel-trace --stats -- python tools/bench_augment.py kernels --config NAME``, a run of its own per configuration
          (the two kernels serve every shape, so their names do not tell the configurations apart).
steps   : what the user pays.  Median synchronised step time of Trainer2D (Unet(1,1,32), batch 4, 256^2) and Trainer3D (UNet3D(1,1,32),
          batch 4, 128^3) fed from a TileStore, A / A / B interleaved in one process: two feeders without augmenter (the spread between
          two runs of the same thing), one with (B), and B with its launches on the
          main stream at hand-over instead of the copy stream (C).  One model and optimizer serve all four.
torch   : the same augmentation written as the eager torch composition a user would otherwise write (affine_grid / grid_sample /
          avg_pool2d / rand_like and the casts around them, fp32), event-timed per batch, with its launches per batch.
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
from bio_image_unet_amd.feed import DeviceFeeder, TileStore  # noqa: E402

HBM_PEAK = 8.0e12            # bytes/s, MI355X HBM3E specification (6.29e12 measured with a float4 copy)
GEO = (17.3, 1.07, 0.03, -0.05)
CONFIGS = {                 # name: (recipe, n, planes, h, w, blur_k)
    "unet_4x256_noblur": ("unet", 4, 1, 256, 256, 0), "unet_4x256_blur7": ("unet", 4, 1, 256, 256, 7),
    "unet_16x512_noblur": ("unet", 16, 1, 512, 512, 0), "unet_16x512_blur7": ("unet", 16, 1, 512, 512, 7),
    "unet3d_4x128": ("unet3d", 4, 128, 128, 128, 0),
}


def _records(recipe, n, h, w, blur_k):
    kw = {"mult": (0.5, 1.2), "blur_k": blur_k} if recipe == "unet" else {"gauss_sigma": 10.0 ** 0.5}
    return np.stack([A.record(i, h, w, rot_k=i % 4 if h == w else 0, ssr=GEO, bc=(1.1, 0.05), **kw) for i in range(n)])


def _launch(src, dst, par, recs, recipe, is_mask, epoch, name):
    n, p, h, w = src.shape
    blurs = recs["blur_k"][(recs["flags"] & A.BLUR) != 0]
    check(lib.biu_augment_u8(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, p, h, w, int(is_mask), C.c_void_p(par.data_ptr()),
                             A.RECIPES[recipe], 0 if is_mask or not len(blurs) else int(blurs.max()), 1, epoch, A.field_id(name),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), "augment_u8")


def kernels(a):
    print(f"{'configuration':22s} {'field':>6s} {'MiB r+w':>8s} {'us/launch':>10s} {'GB/s':>8s} {'% HBM peak':>10s}")
    for name, (recipe, n, p, h, w, blur_k) in CONFIGS.items():
        if a.config and a.config != name:
            continue
        recs = _records(recipe, n, h, w, blur_k)
        par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
        src = torch.randint(0, 256, (n, p, h, w), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for field, is_mask in (("image", False), ("mask", True)):
            for i in range(5):
                _launch(src, dst, par, recs, recipe, is_mask, i, field)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.iters):
                _launch(src, dst, par, recs, recipe, is_mask, i, field)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.iters
            nbytes = 2 * src.numel()
            print(f"{name:22s} {field:>6s} {nbytes / 2 ** 20:8.2f} {us:10.2f} {nbytes / us / 1e3:8.1f} {100 * nbytes / (us * 1e-6) / HBM_PEAK:10.2f}")


def _make_store(tmp, name, n, fields):
    st = TileStore.create(os.path.join(tmp, name), n, fields, {"dim_out": list(next(iter(fields.values()))), "shiftscalerotate": [0.1, 0.2, 30]})
    rng = np.random.default_rng(0)
    for k, shp in fields.items():
        for i in range(n):
            st.maps[k][i] = (rng.random(shp) > 0.5) * 255 if k == "mask" else rng.integers(0, 256, shp)
    st.flush()
    return st


def steps(a):
    from bio_image_unet_amd.workflow import Trainer2D, Trainer3D
    with tempfile.TemporaryDirectory() as tmp:
        for fam, T, fields, n, recipe in (("2d", Trainer2D, {"image": (256, 256), "mask": (256, 256)}, 80, "unet"),
                                          ("3d", Trainer3D, {"volume": (128, 128, 128), "mask": (128, 128, 128)}, 20, "unet3d")):
            if a.family and a.family != fam:
                continue
            st = _make_store(tmp, fam, n, fields)
            torch.manual_seed(0)
            tr = T(st, 1, batch_size=4, n_filter=32, val_split=0.2, save_dir=os.path.join(tmp, "out" + fam), device="cuda")
            idx = tr.train_loader.indices
            feeders = {"A1 (no augmenter)": DeviceFeeder(st, idx, 4, "cuda"), "A2 (no augmenter)": DeviceFeeder(st, idx, 4, "cuda"),
                       "B  (augmenter)": DeviceFeeder(st, idx, 4, "cuda", augmenter=A.Augmenter.from_store(st, recipe, seed=1)),
                       "C  (B, main stream)": DeviceFeeder(st, idx, 4, "cuda", augmenter=A.Augmenter.from_store(st, recipe, seed=1),
                                                           augment_stream="main")}
            times = {k: [] for k in feeders}
            for rnd in range(a.rounds + 1):                      # round 0 warms every shape up and is dropped
                for k, fd in feeders.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for batch in fd:
                        loss = tr._forward_loss(batch, validating=False)
                        tr.optimizer.zero_grad()
                        loss.backward()
                        tr.optimizer.step()
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        if rnd:
                            times[k].append((t1 - t0) * 1e3)
                        t0 = t1
            print(f"{T.__name__} n_filter=32 batch 4 {next(iter(fields.values()))}: synchronised step time, ms, {len(times[k])} steps per variant")
            for k, v in times.items():
                v = sorted(v)
                print(f"  {k:20s} median {statistics.median(v):8.3f}   p10 {v[len(v) // 10]:8.3f}   p90 {v[(9 * len(v)) // 10]:8.3f}")


def _torch_compose(x, recs, recipe, is_mask):
    """[N, P, H, W] uint8 -> uint8: the eager composition (one affine resampling per batch; per-sample blur sizes would need a loop on top)."""
    import torch.nn.functional as F
    n, p, h, w = x.shape
    m = torch.from_numpy(recs["m"].reshape(n, 2, 3).astype(np.float32)).cuda()
    # pixel-space inverse map -> the normalised [-1, 1] grid of affine_grid(align_corners=True)
    sx, sy = (w - 1) / 2.0, (h - 1) / 2.0
    theta = torch.stack([torch.stack([m[:, 0, 0], m[:, 0, 1] * sy / sx, (m[:, 0, 0] * sx + m[:, 0, 1] * sy + m[:, 0, 2]) / sx - 1], 1),
                         torch.stack([m[:, 1, 0] * sx / sy, m[:, 1, 1], (m[:, 1, 0] * sx + m[:, 1, 1] * sy + m[:, 1, 2]) / sy - 1], 1)], 1)
    grid = F.affine_grid(theta, (n, p, h, w), align_corners=True)
    q = lambda v: v.clamp(0, 255).round()
    v = q(F.grid_sample(x.float(), grid, mode="nearest" if is_mask else "bilinear", padding_mode="reflection", align_corners=True))
    if is_mask:
        return v.to(torch.uint8)
    alpha = torch.from_numpy(recs["alpha"].copy()).cuda().view(n, 1, 1, 1)
    beta = torch.from_numpy(recs["beta"].copy()).cuda().view(n, 1, 1, 1)
    if recipe == "unet":
        v = q(v * alpha + beta)
        k = int(recs["blur_k"].max())
        if k:
            v = q(F.avg_pool2d(F.pad(v, (k // 2,) * 4, mode="reflect"), k, stride=1))
        v = q(v * (0.5 + 0.7 * torch.rand_like(v)))
    else:
        v = q(v + float(recs["noise_a"][0]) * torch.randn_like(v))
        v = q(v * alpha + beta)
    return v.to(torch.uint8)


def torch_compose(a):
    print(f"{'configuration':22s} {'field':>6s} {'us/batch, eager torch':>22s} {'launches/batch':>15s}   (biu_augment_u8: 1 launch per field)")
    for name, (recipe, n, p, h, w, blur_k) in CONFIGS.items():
        if a.config and a.config != name:
            continue
        recs = _records(recipe, n, h, w, blur_k)
        src = torch.randint(0, 256, (n, p, h, w), dtype=torch.uint8, device="cuda")
        for field, is_mask in (("image", False), ("mask", True)):
            for _ in range(3):
                _torch_compose(src, recs, recipe, is_mask)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                _torch_compose(src, recs, recipe, is_mask)
            e1.record()
            torch.cuda.synchronize()
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    _torch_compose(src, recs, recipe, is_mask)
                    torch.cuda.synchronize()
                launches = str(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))
            except Exception as ex:                              # the count is a convenience; the time above does not depend on it
                launches = f"not measured ({type(ex).__name__})"
            print(f"{name:22s} {field:>6s} {e0.elapsed_time(e1) * 1e3 / a.iters:22.1f} {launches:>15s}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "steps", "torch"])
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--family", default=None, choices=["2d", "3d"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    print("python tools/bench_augment.py " + " ".join(sys.argv[1:]))
    {"kernels": kernels, "steps": steps, "torch": torch_compose}[a.mode](a)


if __name__ == "__main__":
    main()
