"""What on-device float augmentation costs (bio_image_unet_amd/augment.py: AugmenterF32, biu_augment_f32).

    python tools/bench_augment_f32.py kernels [--iters 200]
    python tools/bench_augment_f32.py torch   [--iters 50]
    python tools/bench_augment_f32.py steps   [--rounds 6]
    python tools/bench_augment_f32.py cubic   [--iters 200] [--rounds 6]

kernels : one launch per field per batch, timed with device events around --iters back-to-back launches (launch gaps included), per kind
          (IMAGE with every intensity stage on, with and without the blur; MASK nearest and bilinear; VECTOR), float32 and uint8 sources, at
          4 x 256^2 and 4 x 512^2.  Printed with the bytes the algorithm needs (field read once + written once).
torch   : the same pipeline written as the eager torch composition a user would otherwise write (index gather with wrap-around, avg_pool2d
          on a wrap-padded tile, torch.poisson / randn_like, clamp), event-timed per batch.
steps   : what the user pays.  Median synchronised step time of TrainerMo2d (MultiOutputNestedUNet(n_filter=32), batch 4, 256^2, a mask, a
          distance and an orientation head) fed from a mixed u8 / f32 TileStore, A / A / B interleaved in one process: two feeders without
          augmenter (the spread between two runs of the same thing), one with the default augmenter and one with
          AugmenterF32(target_interp="cubic").  One model and optimizer serve all four.
cubic   : what the cubic-spline resampling of rotated targets costs over the bilinear gather.  The MASK launch of biu_augment_f32 against
          biu_spline_prefilter_f32 + biu_augment_f32_cubic (three launches), alternating in one process, --rounds rounds of --iters back-to-back
          calls each, at 4 x 1 x 256^2 and 4 x 2 x 256^2 with all four samples under an arbitrary angle and with one of four; median and
          (min .. max) over the rounds.  Then a DeviceFeeder epoch (no training, consumer synchronises per batch) with either augmenter,
          alternating, ms per batch of 4.
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

SIZES = ((4, 256), (4, 512))
CASES = {            # name: (kind, planes, record keywords)
    "image, all stages, blur 5": (A.KIND_IMAGE, 1, dict(angle=17.3, scale=1.07, shift=(5, -3), blur_k=5, shot_s=0.005, gauss_sigma=0.05, bc=(1.1, 0.05))),
    "image, all stages, no blur": (A.KIND_IMAGE, 1, dict(angle=17.3, scale=1.07, shift=(5, -3), shot_s=0.005, gauss_sigma=0.05, bc=(1.1, 0.05))),
    "image, gather only": (A.KIND_IMAGE, 1, dict(angle=17.3, scale=1.07, shift=(5, -3))),
    "mask, bilinear": (A.KIND_MASK, 1, dict(angle=17.3, scale=1.07, shift=(5, -3))),
    "mask, nearest": (A.KIND_MASK, 1, dict(rot_k=1, scale=1.07, shift=(5, -3))),
    "vector": (A.KIND_VECTOR, 2, dict(angle=17.3, scale=1.07, shift=(5, -3))),
}
HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "distance": {"channels": 1, "activation": "relu", "loss": "WeightedDistanceGradientLoss", "weight": 0.25},
         "orientation": {"channels": 2, "activation": None, "loss": "WeightedVectorFieldLoss", "weight": 0.5}}


def _launch(src, dst, par, recs, kind, epoch):
    n, p, h, w = src.shape
    blurs = recs["blur_k"][(recs["flags"] & A.BLUR_F) != 0]
    check(lib.biu_augment_f32(C.c_void_p(src.data_ptr()), int(src.dtype == torch.uint8), C.c_void_p(dst.data_ptr()), n, p, h, w, kind,
                              C.c_void_p(par.data_ptr()), int(blurs.max()) if kind == A.KIND_IMAGE and len(blurs) else 0, 1, epoch, A.field_id("f"),
                              C.c_void_p(torch.cuda.current_stream().cuda_stream)), "augment_f32")


def _timed(fn, iters, warm=5):
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


def _source(n, p, hw, u8):
    return (torch.randint(0, 256, (n, p, hw, hw), dtype=torch.uint8, device="cuda") if u8
            else torch.rand((n, p, hw, hw), dtype=torch.float32, device="cuda"))


def kernels(a):
    print(f"{'case':28s} {'batch':>10s} {'source':>6s} {'MiB r+w':>8s} {'us/launch':>10s} {'GB/s':>8s}")
    for n, hw in SIZES:
        for name, (kind, p, kw) in CASES.items():
            recs = np.stack([A.record_f32(i, hw, hw, **kw) for i in range(n)])
            par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
            for u8 in (False, True):
                src = _source(n, p, hw, u8)
                dst = torch.empty(src.shape, dtype=torch.float32, device="cuda")
                us = _timed(lambda i: _launch(src, dst, par, recs, kind, i), a.iters)
                nbytes = src.numel() * (src.element_size() + 4)
                print(f"{name:28s} {f'{n} x {hw}^2':>10s} {'u8' if u8 else 'f32':>6s} {nbytes / 2 ** 20:8.2f} {us:10.2f} {nbytes / us / 1e3:8.1f}")


def _torch_compose(x, recs, kind):
    """[N, P, H, W] float32 -> float32: the eager composition of the same pipeline (one blur size and one noise scale per batch; per-sample
    values would need a loop on top)."""
    import torch.nn.functional as F
    n, p, h, w = x.shape
    m = torch.from_numpy(recs["m"].copy()).cuda()
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float64), torch.arange(w, device="cuda", dtype=torch.float64), indexing="ij")
    sx = m[:, 0, None, None] * xx + m[:, 1, None, None] * yy + m[:, 2, None, None]
    sy = m[:, 3, None, None] * xx + m[:, 4, None, None] * yy + m[:, 5, None, None]
    flat = x.reshape(n, p, h * w)
    take = lambda iy, ix: torch.gather(flat, 2, (torch.remainder(iy, h) * w + torch.remainder(ix, w)).reshape(n, 1, h * w).expand(n, p, h * w)).reshape(n, p, h, w)
    if kind == A.KIND_MASK and int(recs["flags"][0]) & A.ROT_F:
        x0, y0 = torch.floor(sx), torch.floor(sy)
        ax, ay = (sx - x0).float().unsqueeze(1), (sy - y0).float().unsqueeze(1)
        x0, y0 = x0.long(), y0.long()
        top = torch.lerp(take(y0, x0), take(y0, x0 + 1), ax)
        return torch.lerp(top, torch.lerp(take(y0 + 1, x0), take(y0 + 1, x0 + 1), ax), ay)
    v = take(torch.floor(sy + 0.5).long(), torch.floor(sx + 0.5).long())
    if kind == A.KIND_MASK:
        return v
    if kind == A.KIND_VECTOR:
        ct = torch.from_numpy(recs["cos_t"].copy()).cuda().view(n, 1, 1, 1)
        st = torch.from_numpy(recs["sin_t"].copy()).cuda().view(n, 1, 1, 1)
        c, s = v[:, 0::2], v[:, 1::2]
        return torch.stack([c * ct + s * st, s * ct - c * st], 2).reshape(n, p, h, w)
    k = int(recs["blur_k"].max())
    if k:                                                        # wrap padding of the gathered tile: close to, not the same as, more gathered image
        v = F.avg_pool2d(F.pad(v, (k // 2,) * 4, mode="circular"), k, stride=1)
    if int(recs["flags"][0]) & A.SHOT_F:
        s = float(recs["shot_s"][0])
        v = (torch.poisson(v.pow(2.2) / s) * s).clamp(0, 1).pow(1 / 2.2)
    if int(recs["flags"][0]) & A.GAUSS_F:
        v = (v + float(recs["gauss_sigma"][0]) * torch.randn_like(v)).clamp(0, 1)
    if int(recs["flags"][0]) & A.BC_F:
        v = (v * float(recs["alpha"][0]) + float(recs["beta"][0])).clamp(0, 1)
    return v


def torch_compose(a):
    print(f"{'case':28s} {'batch':>10s} {'us/batch, eager torch':>22s}   (biu_augment_f32: 1 launch per field)")
    for n, hw in SIZES:
        for name, (kind, p, kw) in CASES.items():
            recs = np.stack([A.record_f32(i, hw, hw, **kw) for i in range(n)])
            src = _source(n, p, hw, False)
            us = _timed(lambda i: _torch_compose(src, recs, kind), a.iters, warm=3)
            print(f"{name:28s} {f'{n} x {hw}^2':>10s} {us:22.1f}")


def _launch_cubic(src, coef, rng, dst, par):
    n, p, h, w = src.shape
    st, u8 = C.c_void_p(torch.cuda.current_stream().cuda_stream), int(src.dtype == torch.uint8)
    check(lib.biu_spline_prefilter_f32(C.c_void_p(src.data_ptr()), u8, C.c_void_p(coef.data_ptr()), C.c_void_p(rng.data_ptr()), n, p, h, w,
                                       C.c_void_p(par.data_ptr()), st), "spline_prefilter_f32")
    check(lib.biu_augment_f32_cubic(C.c_void_p(src.data_ptr()), u8, C.c_void_p(coef.data_ptr()), C.c_void_p(rng.data_ptr()), C.c_void_p(dst.data_ptr()),
                                    n, p, h, w, C.c_void_p(par.data_ptr()), st), "augment_f32_cubic")


def _spread(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"


def cubic(a):
    n, hw, geo = 4, 256, dict(scale=1.07, shift=(5, -3))
    print(f"MASK field, f32 source, us per field per batch: median (min .. max) over {a.rounds} rounds of {a.iters} back-to-back calls, alternating")
    print(f"{'batch':>16s} {'rotating':>9s} {'bilinear, 1 launch':>30s} {'cubic, 3 launches':>30s} {'ratio':>6s}")
    for p in (1, 2):
        for rotating in (4, 1):
            recs = np.stack([A.record_f32(i, hw, hw, angle=17.3 + 40 * i if i < rotating else None, **geo) for i in range(n)])
            par = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
            src = _source(n, p, hw, False)
            dst, coef = torch.empty_like(src), torch.empty_like(src)
            rng = torch.empty((n, 2), dtype=torch.float32, device="cuda")
            lin, cub = [], []
            for _ in range(a.rounds):
                lin.append(_timed(lambda i: _launch(src, dst, par, recs, A.KIND_MASK, i), a.iters))
                cub.append(_timed(lambda i: _launch_cubic(src, coef, rng, dst, par), a.iters))
            print(f"{f'{n} x {p} x {hw}^2':>16s} {f'{rotating} of {n}':>9s} {_spread(lin):>30s} {_spread(cub):>30s} {statistics.median(cub) / statistics.median(lin):6.2f}")
    with tempfile.TemporaryDirectory() as tmp:
        st = _make_store(tmp, 80, (256, 256))
        idx = list(range(80))
        feeders = {"linear": DeviceFeeder(st, idx, 4, "cuda", augmenter=A.AugmenterF32.from_store(st, seed=1)),
                   "cubic": DeviceFeeder(st, idx, 4, "cuda", augmenter=A.AugmenterF32.from_store(st, seed=1, target_interp="cubic"))}
        times = {k: [] for k in feeders}
        for rnd in range(a.rounds + 1):                          # round 0 warms up and is dropped
            for k, fd in feeders.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batches = 0
                for _ in fd:
                    torch.cuda.synchronize()
                    batches += 1
                if rnd:
                    times[k].append((time.perf_counter() - t0) * 1e3 / batches)
        print(f"DeviceFeeder epoch, 80 tiles of 256^2 (image u8; mask, distance, orientation f32), batch 4, no training: ms per batch, median (min .. max) over {a.rounds} epochs")
        for k, v in times.items():
            print(f"  {k:8s} {_spread(v)}")


def _make_store(tmp, n, hw):
    fields = {"image": hw, "mask": (1,) + hw, "distance": hw, "orientation": (2,) + hw}
    st = TileStore.create(os.path.join(tmp, "mo2d"), n, fields, {"dim_out": list(hw), "scale_limit": [-0.1, 0.1]},
                          dtypes={"mask": "f32", "distance": "f32", "orientation": "f32"})
    rng = np.random.default_rng(0)
    for i in range(n):
        phi = rng.uniform(0, 2 * np.pi, hw)
        st.maps["image"][i] = rng.integers(0, 256, hw)
        st.maps["mask"][i] = rng.random((1,) + hw) > 0.5
        st.maps["distance"][i] = rng.random(hw) * (rng.random(hw) < 0.6)
        st.maps["orientation"][i] = np.stack([np.cos(phi), np.sin(phi)])
    st.flush()
    return st


def steps(a):
    from bio_image_unet_amd import MultiOutputNestedUNet
    from bio_image_unet_amd.workflow import TrainerMo2d
    with tempfile.TemporaryDirectory() as tmp:
        st = _make_store(tmp, 80, (256, 256))
        torch.manual_seed(0)
        tr = TrainerMo2d(st, 1, network=MultiOutputNestedUNet, batch_size=4, output_heads=HEADS, n_filter=32, val_split=0.2,
                         save_dir=os.path.join(tmp, "out"), device="cuda")
        idx = tr.train_loader.indices
        feeders = {"A1 (no augmenter)": DeviceFeeder(st, idx, 4, "cuda"), "A2 (no augmenter)": DeviceFeeder(st, idx, 4, "cuda"),
                   "B  (augmenter)": DeviceFeeder(st, idx, 4, "cuda", augmenter=A.AugmenterF32.from_store(st, seed=1)),
                   "C  (cubic targets)": DeviceFeeder(st, idx, 4, "cuda", augmenter=A.AugmenterF32.from_store(st, seed=1, target_interp="cubic"))}
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
        print(f"TrainerMo2d MultiOutputNestedUNet n_filter=32 batch 4 (256, 256): synchronised step time, ms, {len(times[k])} steps per variant")
        for k, v in times.items():
            v = sorted(v)
            print(f"  {k:20s} median {statistics.median(v):8.3f}   p10 {v[len(v) // 10]:8.3f}   p90 {v[(9 * len(v)) // 10]:8.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "steps", "torch", "cubic"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    print("python tools/bench_augment_f32.py " + " ".join(sys.argv[1:]))
    {"kernels": kernels, "steps": steps, "torch": torch_compose, "cubic": cubic}[a.mode](a)


if __name__ == "__main__":
    main()
