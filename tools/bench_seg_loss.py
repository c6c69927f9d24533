"""What the single-head segmentation losses cost on their own, at the logits shapes of bench.py's configurations: cfg1 calls the criterion
on (1, 256, 256) and cfg2 on (2, 512, 512) (one batch entry per call, unet/train.py:133-134), cfg4 on (4, 1, 128, 128, 128) with the
batch-axis SmoothL1 "time" term (unet3d/train.py:140-145).  No network: the logits are fixed fp32 tensors that require a gradient.

    python tools/bench_seg_loss.py [--steps 200] [--warmup 20]

Forward plus backward of ``BCEDiceLoss(1, 1)`` and ``logcoshTverskyLoss()``, with and without ``time_weight = 0.1`` where the batch has more
than one entry, timed with HIP events.  Reported per row: the median, minimum and 90th percentile over --steps in milliseconds, the median
host time to enqueue the step (where it equals the event time, the step is bound by the host's launches, not by the device), the library's
launches of one step with the median of their summed HIP-event times in microseconds (``biu us``: the device side alone, taken in steps of
their own through the binding's call log), and the loss value.  To compare two builds, run this file from each tree alternately on one
machine (profiles/r14_seg_loss_ab.txt).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bio_image_unet_amd import losses as P  # noqa: E402
from bio_image_unet_amd._lib import lib  # noqa: E402

SHAPES = {"cfg1": (1, 256, 256), "cfg2": (2, 512, 512), "cfg4": (4, 1, 128, 128, 128)}
CRITERIA = {"BCEDiceLoss(1, 1)": lambda: P.BCEDiceLoss(1, 1), "logcoshTverskyLoss()": P.logcoshTverskyLoss}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    g = torch.Generator(device="cuda").manual_seed(1)
    print(f"tools/bench_seg_loss.py --steps {a.steps} --warmup {a.warmup}   (a step = forward + backward of the loss, HIP events around it)")
    print(f"{'shape':6s} {'criterion':22s} {'time':>5s} {'median ms':>10s} {'min ms':>9s} {'p90 ms':>9s} {'host ms':>9s} {'launches':>8s} {'biu us':>8s}   loss")
    for cfg, shape in SHAPES.items():
        x = (torch.randn(shape, device="cuda", generator=g) * 2).requires_grad_(True)
        t = (torch.rand(shape, device="cuda", generator=g) < 0.4).float()
        for name, make in CRITERIA.items():
            for w in (0.0, 0.1) if shape[0] > 1 else (0.0,):
                crit, times, host = make(), [], []
                for i in range(a.warmup + a.steps):
                    x.grad = None
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    h0 = time.perf_counter()
                    e0.record()
                    loss = crit(x, t, time_weight=w) if w else crit(x, t)
                    loss.backward()
                    e1.record()
                    h1 = time.perf_counter()
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        times.append(e0.elapsed_time(e1))
                        host.append((h1 - h0) * 1e3)
                dev = []
                for _ in range(30):          # the library's calls alone, each between two events
                    x.grad = None
                    lib.prof = []
                    (crit(x, t, time_weight=w) if w else crit(x, t)).backward()
                    torch.cuda.synchronize()
                    calls = [c for c in lib.prof if not c[0].endswith("_blocks")]
                    dev.append(sum(c[2].elapsed_time(c[3]) for c in calls) * 1e3)
                    lib.prof = None
                s = sorted(times)
                print(f"{cfg:6s} {name:22s} {w:5.1f} {statistics.median(s):10.4f} {s[0]:9.4f} {s[int(0.9 * (len(s) - 1))]:9.4f} "
                      f"{statistics.median(host):9.4f} {len(calls):8d} {statistics.median(dev):8.1f}   {float(loss.detach()):.8f}")


if __name__ == "__main__":
    main()
