"""What rendering training patches straight from whole items costs (feed.CropFeeder, biu_augment_f32_crop) against augmenting stored tiles
(feed.DeviceFeeder + AugmenterF32, biu_augment_f32), and whether the feeder keeps ahead of the training step.

    python tools/bench_augment_crop.py [feeders | cubic] [--rounds 6]

feeders : an epoch of CropFeeder over an ImageStore of 8 items (512 x 640 and 640 x 512; image u8; mask, distance, orientation f32 with NaN
          holes; aug_factor 2, i.e. 80 patches of 256^2) and an epoch of DeviceFeeder + AugmenterF32 over a TileStore with the same number of
          256^2 tiles and the same fields.  No training, the consumer synchronises per batch of 4; the two alternate in one process; ms per
          batch as median (min .. max) over --rounds epochs (a first epoch warms up and is dropped).
step    : the synchronised TrainerMo2d step (MultiOutputNestedUNet(n_filter=32), batch 4, 256^2, a mask, a distance and an orientation head)
          fed by the CropFeeder, in the same process: what the feeder has to keep ahead of.
cubic   : what AugmenterF32(target_interp="cubic") costs on the same ImageStore.  The table build (ImageStore.spline_tables' work, once per
          store and device: SplineTables.build per "mask" field, synchronised; the first build and --rounds repeats), then an epoch of the
          CropFeeder with the linear and with the cubic augmenter, alternating as above, then the synchronised TrainerMo2d step fed by the
          cubic CropFeeder.
"""
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

from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd.feed import CropFeeder, DeviceFeeder, ImageStore, SplineTables, TileStore  # noqa: E402

HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "distance": {"channels": 1, "activation": "relu", "loss": "WeightedDistanceGradientLoss", "weight": 0.25},
         "orientation": {"channels": 2, "activation": None, "loss": "WeightedVectorFieldLoss", "weight": 0.5}}
TILE = (256, 256)
LIMITS = {"scale_limit": [-0.1, 0.1]}


def _fields(rng, hw, holes):
    phi = rng.uniform(0, 2 * np.pi, hw)
    mask = (rng.random(hw) > 0.5).astype(np.float32)
    if holes:                                                    # "no label here": a band and scattered pixels
        mask[hw[0] // 3:hw[0] // 3 + 20] = np.nan
        phi[rng.random(hw) < 0.02] = np.nan
    return {"image": rng.integers(0, 256, hw, dtype=np.uint8), "mask": mask, "distance": (rng.random(hw) * (rng.random(hw) < 0.6)).astype(np.float32),
            "orientation": np.stack([np.cos(phi), np.sin(phi)]).astype(np.float32)}


def _image_store(tmp):
    sizes = [(512, 640), (640, 512)] * 4
    st = ImageStore.create(os.path.join(tmp, "whole"), sizes, {"image": 1, "mask": 1, "distance": 1, "orientation": 2},
                           {"dim_out": list(TILE), "aug_factor": 2, "nan_to_val": 0.0, **LIMITS},
                           dtypes={"image": "u8", "mask": "f32", "distance": "f32", "orientation": "f32"},
                           squeeze={"image": True, "distance": True})
    rng = np.random.default_rng(0)
    for i, hw in enumerate(sizes):
        for k, v in _fields(rng, hw, True).items():
            st.put(i, k, v)
    st.flush()
    return st


def _tile_store(tmp, n):
    st = TileStore.create(os.path.join(tmp, "tiles"), n, {"image": TILE, "mask": (1,) + TILE, "distance": TILE, "orientation": (2,) + TILE},
                          {"dim_out": list(TILE), **LIMITS}, dtypes={"mask": "f32", "distance": "f32", "orientation": "f32"})
    rng = np.random.default_rng(0)
    for i in range(n):
        for k, v in _fields(rng, TILE, False).items():
            st.maps[k][i] = v.reshape(st.maps[k][i].shape)
    st.flush()
    return st


def _spread(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="feeders", choices=["feeders", "cubic"])
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from bio_image_unet_amd import MultiOutputNestedUNet
    from bio_image_unet_amd.workflow import TrainerMo2d
    print("python tools/bench_augment_crop.py " + " ".join(sys.argv[1:]))
    print(f"box: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}, HIP {torch.version.hip}")
    with tempfile.TemporaryDirectory() as tmp:
        whole = _image_store(tmp)
        idx = list(range(len(whole)))
        augment, first = None, "CropFeeder, ImageStore"
        feeders = {first: CropFeeder(whole, idx, 4, "cuda", A.AugmenterF32.from_store(whole, seed=1))}
        if a.mode == "cubic":
            augment, first = A.AugmenterF32.from_store(whole, seed=1, target_interp="cubic"), "CropFeeder, cubic targets"
            arenas = whole.to_device("cuda")[0]
            names = augment.spline_fields(whole)
            build = []
            for rnd in range(a.rounds + 1):                      # the first build is reported on its own: it is the one a Trainer pays
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tabs = {k: SplineTables.build(arenas[k], whole.planes[k], whole.offsets[k], whole.sizes) for k in names}
                torch.cuda.synchronize()
                build.append((time.perf_counter() - t0) * 1e3)
            print(f"table build, {whole.n_items} items of 512 x 640, fields {names}: first {build[0]:.3f} ms, then {_spread(build[1:])} ms; "
                  + ", ".join(f"{k}: {t.nbytes} bytes{'' if t.indicator is None else ' with the indicator'}" for k, t in tabs.items())
                  + f"; the field arenas: {', '.join(str(arenas[k].numel() * arenas[k].element_size()) for k in names)} bytes")
            del tabs
            feeders = {"CropFeeder, linear targets": feeders.pop("CropFeeder, ImageStore"),
                       first: CropFeeder(whole, idx, 4, "cuda", augment, spline=whole.spline_tables("cuda", names))}
        else:
            tiles = _tile_store(tmp, len(whole))
            feeders["DeviceFeeder + AugmenterF32, TileStore"] = DeviceFeeder(tiles, idx, 4, "cuda", augmenter=A.AugmenterF32.from_store(tiles, seed=1))
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
        print(f"feeder epoch, {len(whole)} patches of 256^2 (image u8; mask, distance, orientation f32), batch 4, no training: "
              f"ms per batch, median (min .. max) over {a.rounds} epochs, alternating")
        for k, v in times.items():
            print(f"  {k:40s} {_spread(v)}")
        torch.manual_seed(0)
        tr = TrainerMo2d(whole, 1, network=MultiOutputNestedUNet, batch_size=4, output_heads=HEADS, n_filter=32, val_split=0.2,
                         save_dir=os.path.join(tmp, "out"), device="cuda", augment=augment)
        steps = []
        for rnd in range(a.rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for batch in tr.train_loader:
                loss = tr._total_loss(batch, validating=False)
                tr.optimizer.zero_grad()
                loss.backward()
                tr.optimizer.clip_grad_norm_(1.0)
                tr.optimizer.step()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if rnd:
                    steps.append((t1 - t0) * 1e3)
                t0 = t1
        steps.sort()
        print(f"TrainerMo2d MultiOutputNestedUNet n_filter=32 batch 4 (256, 256) fed by the {first}: synchronised step time, ms, {len(steps)} steps")
        print(f"  median {statistics.median(steps):8.3f}   p10 {steps[len(steps) // 10]:8.3f}   p90 {steps[(9 * len(steps)) // 10]:8.3f}")
        crop = statistics.median(times[first])
        print(f"the feeder needs {crop:.3f} ms per batch, the step {statistics.median(steps):.3f} ms: "
              f"{'the feeder keeps ahead of the step' if crop < statistics.median(steps) else 'THE FEEDER IS SLOWER THAN THE STEP'}")


if __name__ == "__main__":
    main()
