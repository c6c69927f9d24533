"""What the front of a Predict run costs before the first forward: percentile normalisation and tiling of the raw stack, on the host (numpy, the
default ``preprocess='host'``) and on the device (``preprocess='device'``: ``bio_image_unet_amd/preprocess.py``).  No network is involved.

    python tools/bench_predict_frontend.py [--frames 16] [--size 2048] [--tile 512] [--reps 7] [--warmup 2]

  Predict2D    a uint16 stack (frames, size, size), 'single' normalisation, clip (0, 99.8), tiles (tile, tile), batch of 8
      host     ``np.array(float64)`` + ``normalise_stack`` + ``Predict2D._split`` + the first batch sent up (``.to('cuda')``, synchronised)
      device   upload of the raw stack + order statistics of every image + finalize + the first batch cut, synchronised;
               ``all cut``: the same with every patch of the stack cut, batch by batch
  PredictSiam  the same array as a movie: per frame the host normalises the (previous, current) pair in float64 and tiles it inside the
               frame loop, so its whole-movie time is what the GPU waits for in total and its first-frame time what the first forward waits
               for; the device selects all pairs' statistics in one batch, then cuts per frame

Host clock around work that ends in a device synchronise; the routes run alternately in one process; medians over --reps after --warmup,
with minimum and maximum as the spread.  A last section times selection + finalize and the cutting of every patch with device events on a
stack that is already in HBM, beside the host's time to enqueue them (a few dozen small launches from Python).  The first batches of the two routes are compared byte for byte.  numpy's percentile (a partial
sort) and its elementwise passes run on one core whatever the machine offers; the figures say nothing about a host that parallelises them.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bio_image_unet_amd import workflow as Wf  # noqa: E402
from bio_image_unet_amd.preprocess import DeviceFrontEnd  # noqa: E402

CLIP, BATCH = (0., 99.8), 8


def _bare(cls, **attrs):
    obj = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _row(name, t):
    t = sorted(t)
    print(f"  {name:44s} median {statistics.median(t):10.2f} ms   min {t[0]:10.2f}   max {t[-1]:10.2f}")
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    rng = np.random.default_rng(0)
    raw = (rng.gamma(2.0, 900.0, (a.frames, a.size, a.size)).clip(0, 65535)).astype(np.uint16)        # a skewed, camera-like histogram
    tile = (a.tile, a.tile)
    print(f"tools/bench_predict_frontend.py --frames {a.frames} --size {a.size} --tile {a.tile} --reps {a.reps} --warmup {a.warmup}")
    print(f"input: uint16 {raw.shape} ({raw.nbytes / 2 ** 20:.0f} MiB); normalization_mode 'single', clip {CLIP}, tiles {tile}, first batch = {BATCH} patches")
    print(f"host: thread budget OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')} CPUs for this command; numpy's "
          "percentile (a partial sort) and its elementwise passes are single-threaded and use one of them")
    print("times: host clock, each ending in a device synchronise; routes alternate in one process\n")

    # ---- Predict2D -------------------------------------------------------------------------------------------------
    p2 = _bare(Wf.Predict2D, imgs_shape=raw.shape, resize_dim=tile, add_tile=0)

    def host2d():
        imgs = Wf.normalise_stack(np.array(raw, dtype=np.float64), "single", CLIP, False)
        patches = p2._split(imgs)
        return torch.from_numpy(patches[:BATCH]).to("cuda")

    def dev2d(everything=False):
        fe = DeviceFrontEnd(raw, "cuda")
        fe.normalise("single", CLIP)
        tiles = fe.tiles(p2._origins(), (1,) + tile, out="uint8")
        first = tiles.batch(0, BATCH)
        if everything:
            for b in range(BATCH, len(tiles), BATCH):
                tiles.batch(b, b + BATCH)
        return first

    # ---- PredictSiam -----------------------------------------------------------------------------------------------
    ps = _bare(Wf.PredictSiam, imgs_shape=list(raw.shape), resize_dim=tile, add_tile=0)

    def host_siam(frames):
        first = None
        for i in range(frames):
            prev = (raw[0] if a.frames == 1 else raw[1]) if i == 0 else raw[i - 1]
            pair = Wf.normalise_stack(np.array([prev, raw[i]], dtype=np.float64), "single", CLIP, False).astype("uint8")
            patches = ps._split(pair)
            b = torch.from_numpy(patches[:BATCH]).to("cuda")
            first = b if first is None else first
        return first

    def dev_siam(frames):
        fe = DeviceFrontEnd(raw, "cuda")
        fe.normalise_pairs("single", CLIP)
        pairs = fe.pair_tiles(ps._origins(), tile)
        first = None
        for i in range(frames):
            fr = pairs.frame(i, ps.N)
            for b in range(0, ps.N if frames > 1 else BATCH, BATCH):
                out = fr.batch(b, b + BATCH)
                first = out if first is None else first
        return first

    routes = {"Predict2D host: first batch ready": host2d,
              "Predict2D device: first batch ready": dev2d,
              "Predict2D device: all cut": lambda: dev2d(True),
              "PredictSiam host: first frame's first batch": lambda: host_siam(1),
              "PredictSiam host: whole movie": lambda: host_siam(a.frames),
              "PredictSiam device: first frame's first batch": lambda: dev_siam(1),
              "PredictSiam device: whole movie cut": lambda: dev_siam(a.frames)}
    times, outs = {k: [] for k in routes}, {}
    for i in range(a.warmup + a.reps):
        for k, fn in routes.items():
            ms, out = _clock(fn)
            outs[k] = out.cpu().numpy()
            if i >= a.warmup:
                times[k].append(ms)
    med = {k: _row(k, t) for k, t in times.items()}
    same2d = np.array_equal(outs["Predict2D host: first batch ready"], outs["Predict2D device: first batch ready"])
    same_s = np.array_equal(outs["PredictSiam host: first frame's first batch"], outs["PredictSiam device: first frame's first batch"])
    print(f"\nfirst batches byte-equal between host and device: Predict2D {same2d}, PredictSiam {same_s}")
    print(f"host / device, first batch ready: Predict2D {med['Predict2D host: first batch ready'] / med['Predict2D device: first batch ready']:.1f}, "
          f"PredictSiam whole movie {med['PredictSiam host: whole movie'] / med['PredictSiam device: whole movie cut']:.1f}")
    # the kernels alone, from device events, on data already in HBM
    fe = DeviceFrontEnd(raw, "cuda")
    ev = []
    for _ in range(a.warmup + a.reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        e[0].record()
        fe.normalise("single", CLIP)
        e[1].record()
        h1 = time.perf_counter()
        tiles = fe.tiles(p2._origins(), (1,) + tile, out="uint8")                # (the origin upload stays outside the timed parts)
        torch.cuda.synchronize()
        h2 = time.perf_counter()
        e[2].record()
        for b in range(0, len(tiles), BATCH):
            tiles.batch(b, b + BATCH)
        e[3].record()
        h3 = time.perf_counter()
        torch.cuda.synchronize()
        ev.append((e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3]), (h1 - h0) * 1e3, (h3 - h2) * 1e3))
    ev = ev[a.warmup:]
    sel, cut, hsel, hcut = (statistics.median(v[i] for v in ev) for i in range(4))
    print(f"\ndevice events, stack resident (host ms = the host's time to enqueue the same work; where the two agree the interval is bound by the "
          f"host's launches, not by the kernels):\n  selection + finalize, {a.frames} images  {sel:8.3f} ms   host {hsel:8.3f} ms\n"
          f"  cutting all {len(tiles)} patches in batches of {BATCH}  {cut:8.3f} ms   host {hcut:8.3f} ms")
    print(f"  bytes: the selection reads the stack twice ({2 * raw.nbytes / 2 ** 20:.0f} MiB), the cut reads it once and writes "
          f"{len(tiles) * a.tile * a.tile / 2 ** 20:.0f} MiB")
    if not (same2d and same_s):
        sys.exit(1)


if __name__ == "__main__":
    main()
