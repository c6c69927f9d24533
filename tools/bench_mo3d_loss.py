"""What the loss side of a 3-D multi-output training step costs at cfg5's extent: three heads at (1, C, 128, 256, 256) -- seg (1 channel),
flow (2 channels), dist (1 channel), every head BCEDiceLoss(1, 1) with weight 1 as in bench.py -- and the same with seg switched to
BCEDiceTemporalLoss.  No network: the head outputs are fixed fp32 tensors that require a gradient, so the figures are the loss side alone.

    python tools/bench_mo3d_loss.py [--steps 30] [--warmup 5]

  per-head  the loop TrainerMo3d ran before the fused node: one ``bio_image_unet_amd.losses`` criterion per head (its own autograd node,
            four biu launches; BCEDiceTemporalLoss adds the eager TemporalConsistencyLoss), ``weight * loss`` and ``total + ...`` in torch
  fused     ``multi_output_unet3d.losses.MultiHeadLoss``: one autograd node, 2 * heads + 2 biu_mo3d_loss_* launches

Forward plus backward of each route is timed with HIP events; the routes run interleaved (per-head, fused, per-head, fused, ...) in one
process, per configuration.  Reported: the median, minimum and 90th percentile over --steps in milliseconds, the median host time to enqueue
the step (``host ms``: where it equals the event time, the step is bound by the host's launches, not by the device), the biu launches one
step issues (the eager torch kernels of the per-head route are not in that count), and the two totals of the last step.
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
from bio_image_unet_amd.multi_output_unet3d import losses as L  # noqa: E402

SPATIAL = (128, 256, 256)
CHANNELS = {"seg": 1, "flow": 2, "dist": 1}
CONFIGS = {"three BCEDiceLoss heads": {"seg": "BCEDiceLoss", "flow": "BCEDiceLoss", "dist": "BCEDiceLoss"},
           "seg switched to BCEDiceTemporalLoss": {"seg": "BCEDiceTemporalLoss", "flow": "BCEDiceLoss", "dist": "BCEDiceLoss"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = {k: (torch.randn((1, c) + SPATIAL, device="cuda", generator=g) * 2).requires_grad_(True) for k, c in CHANNELS.items()}
    tg = {k: (torch.rand((1, c) + SPATIAL, device="cuda", generator=g) < 0.4).float() for k, c in CHANNELS.items()}
    print(f"tools/bench_mo3d_loss.py --steps {a.steps} --warmup {a.warmup}   (one process, routes interleaved)")
    print("heads: " + ", ".join(f"{k} (1, {c}, {', '.join(map(str, SPATIAL))})" for k, c in CHANNELS.items()) + "; fp32, weights 1")
    print("a step = forward + backward of the loss side, HIP events around it\n")
    print(f"{'configuration':40s} {'route':10s} {'median ms':>10s} {'min ms':>9s} {'p90 ms':>9s} {'host ms':>9s} {'biu launches':>13s}   total")
    ok = True
    for title, names in CONFIGS.items():
        heads = {k: {"channels": CHANNELS[k], "loss": names[k], "weight": 1.0} for k in CHANNELS}
        old = {k: (P.BCEDiceTemporalLoss() if n == "BCEDiceTemporalLoss" else P.BCEDiceLoss(1, 1)) for k, n in names.items()}
        fused = L.MultiHeadLoss(heads)

        def per_head():
            total = 0
            for k in heads:
                total = total + heads[k]["weight"] * old[k](xs[k], tg[k])
            return total

        def one_node():
            return fused(xs, tg)

        routes = {"per-head": per_head, "fused": one_node}
        times, host, vals, calls = {k: [] for k in routes}, {k: [] for k in routes}, {}, {}
        for i in range(a.warmup + a.steps):
            for k, fn in routes.items():
                for x in xs.values():
                    x.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                e0.record()
                total = fn()
                total.backward()
                e1.record()
                h1 = time.perf_counter()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
                    host[k].append((h1 - h0) * 1e3)
                vals[k] = float(total.detach())
        for k, fn in routes.items():          # the biu calls of one step, through the binding's call log
            lib.prof = []
            fn().backward()
            torch.cuda.synchronize()
            calls[k] = len([c for c in lib.prof if not c[0].endswith("_blocks")])      # (the *_blocks queries launch nothing)
            lib.prof = None
        for k in routes:
            t = sorted(times[k])
            print(f"{title:40s} {k:10s} {statistics.median(t):10.3f} {t[0]:9.3f} {t[int(0.9 * (len(t) - 1))]:9.3f} "
                  f"{statistics.median(host[k]):9.3f} {calls[k]:13d}   {vals[k]:.8f}")
        mf, mp = statistics.median(times["fused"]), statistics.median(times["per-head"])
        ok = ok and mf <= mp
        print(f"{'':40s} fused <= per-head: {mf <= mp}    per-head / fused = {mp / mf:.2f}\n")
    print(f"fused not slower than per-head in either configuration: {ok}")


if __name__ == "__main__":
    main()
