"""What preparing a training store costs on the device, stage by stage (``bio_image_unet_amd/dataprep.py``, ``csrc/biu_dataprep.hip``).

    python tools/bench_dataprep.py [--images 16] [--size 2048] [--tile 256] [--reps 3]

uint16 images of size x size with label masks of filled ellipses (0 / 255), prepared as ``prepare_unet(..., skeletonize=True, dilate_mask=-2)``
does it: per image the upload, the percentile statistics, the image tiles, and for the mask binarise -> thin -> x 255 -> dilation with
disk(2) -> tile gather.  Per stage, summed over the images: ``kernel`` = device events around the stage's launches, ``wall`` = host clock
around the stage ending in a device synchronise (so it holds the enqueue cost, the thinning loop's counter reads and the copies back).
Medians over --reps passes after one warm-up pass.  The last line is ``prepare_unet`` itself, store files included.  A record, not a test:
nothing here has a threshold."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bio_image_unet_amd import dataprep as DP  # noqa: E402
from bio_image_unet_amd.preprocess import DeviceFrontEnd  # noqa: E402

CLIP = (0.2, 99.8)


def ellipses(size, seed, count=300):
    rng = np.random.default_rng(seed)
    m = np.zeros((size, size), dtype=np.uint8)
    for _ in range(count):
        cy, cx, a, b = rng.integers(0, size), rng.integers(0, size), rng.integers(5, 41), rng.integers(5, 41)
        y0, y1, x0, x1 = max(cy - a, 0), min(cy + a + 1, size), max(cx - b, 0), min(cx + b + 1, size)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        m[y0:y1, x0:x1][((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2 < 1] = 255
    return m


class Stages:
    def __init__(self):
        self.kernel, self.wall = {}, {}

    def run(self, name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        self.wall[name] = self.wall.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
        self.kernel[name] = self.kernel.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def one_pass(images, masks, tile):
    st, iters = Stages(), []
    for img, msk in zip(images, masks):
        org = [(0, y, x) for y, x in DP.origins_2d(img.shape, tile)]
        fe = st.run("image: upload", lambda: DeviceFrontEnd(img[None], "cuda", depth=1))
        st.run("image: percentile statistics", lambda: fe.normalise("single", CLIP))
        tiles = fe.tiles([(0,) + o for o in org], (1,) + tile, out="uint8", view=tile)
        t = st.run("image: normalise + cut tiles", lambda: tiles.batch(0, len(tiles)))
        st.run("image: tiles to the host", lambda: t.cpu())
        m = st.run("mask: upload", lambda: torch.from_numpy(msk[None]).cuda())
        m = st.run("mask: binarise (lut)", lambda: DP.lut(m, np.arange(256) > 1))

        def thin():
            fg = int(torch.count_nonzero(m).item())
            out = DP.thin(m)
            iters.append((fg, int(torch.count_nonzero(out).item())))
            return out
        m = st.run("mask: thin (blocks of 8 iterations)", thin)
        m = st.run("mask: x 255 (lut)", lambda: DP.lut(m, np.where(np.arange(256) != 0, 255, 0)))
        m = st.run("mask: dilation disk(2)", lambda: DP.morph(m, "dilation", "disk", 2))
        g = st.run("mask: gather tiles", lambda: DP.gather(m, 1, org, (1,) + tile))
        st.run("mask: tiles to the host", lambda: g.cpu())
    return st, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    rng = np.random.default_rng(0)
    images = [(rng.gamma(2.0, 900.0, (a.size, a.size)).clip(0, 65535)).astype(np.uint16) for _ in range(a.images)]
    masks = [ellipses(a.size, i) for i in range(a.images)]
    tile = (a.tile, a.tile)
    print(f"tools/bench_dataprep.py --images {a.images} --size {a.size} --tile {a.tile} --reps {a.reps}")
    print(f"input: {a.images} uint16 images and uint8 masks of {a.size} x {a.size}; skeletonize=True, dilate_mask=-2 (dilation, disk), tiles {tile}, clip {CLIP}")
    one_pass(images[:1], masks[:1], tile)
    passes = [one_pass(images, masks, tile) for _ in range(a.reps)]
    fg = sum(f for f, _ in passes[0][1])
    left = sum(s for _, s in passes[0][1])
    print(f"masks: {fg} foreground pixels ({100.0 * fg / (a.images * a.size * a.size):.1f} %), {left} left after thinning\n")
    print(f"  {'stage (sum over the images, ms)':44s} {'kernel':>10s} {'wall':>10s}")
    names = list(passes[0][0].kernel)
    tk = tw = 0.0
    for n in names:
        k, w = statistics.median(p[0].kernel[n] for p in passes), statistics.median(p[0].wall[n] for p in passes)
        tk, tw = tk + k, tw + w
        print(f"  {n:44s} {k:10.3f} {w:10.3f}")
    print(f"  {'all stages':44s} {tk:10.3f} {tw:10.3f}")
    whole = []
    with tempfile.TemporaryDirectory() as d:
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store = DP.prepare_unet(images, masks, os.path.join(d, f"s{r}"), dim_out=tile, skeletonize=True, dilate_mask=-2, device="cuda")
            whole.append((time.perf_counter() - t0) * 1e3)
        print(f"\nprepare_unet(...), store files written ({store.n} tiles): median {statistics.median(whole[1:]):.1f} ms "
              f"(min {min(whole[1:]):.1f}, max {max(whole[1:]):.1f}; first call {whole[0]:.1f})")


if __name__ == "__main__":
    main()
