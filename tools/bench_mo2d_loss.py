"""What the loss side of a 2-D multi-output training step costs: MultiOutputNestedUNet(n_filter=64, deep_supervision=True) in bf16 at batch 4,
256 x 256, three heads (BCEDiceLoss on a sigmoid channel, WeightedVectorFieldLoss on two channels, WeightedDistanceGradientLoss on one),
four supervision levels -> 12 criteria per step.

    python tools/bench_mo2d_loss.py [--steps 30] [--warmup 5] [--only a|b|c] [--count-launches]

  (a) forward + backward of the network alone (the backward is seeded with fixed gradients of the head outputs);
  (b) forward + the criteria as the torch composition on the GPU (the fallback path of bio_image_unet_amd.multi_output_unet.losses, the
      loop of multi_output_unet/train.py:157-181 -- what a user had before the fused criteria) + backward;
  (c) forward + losses.MultiHeadLoss (biu_mo2d_loss_*: 2 * heads + 2 launches) + backward.

No optimizer step in any of them: (b) - (a) and (c) - (a) are the loss side alone.  Every step ends in a device synchronise, as the
reference loop's ``total_loss.item()`` does (in (c) that read carries the deferred range check of BCEDiceLoss).  The three variants run
interleaved in one process (a, b, c, a, b, c, ...); reported: the median over --steps of the host wall time of a step including its
synchronise, and of the device-event time.  ``--only x`` runs one variant (for a kernel trace: ``rocprofv3 --kernel-trace --stats``);
``--count-launches`` prints how many biu_mo2d_loss_* calls one fused step issues.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bio_image_unet_amd as B  # noqa: E402
from bio_image_unet_amd.multi_output_unet import losses as L  # noqa: E402

HEADS = {"seg": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "vec": {"channels": 2, "activation": None, "loss": "WeightedVectorFieldLoss", "weight": 0.5},
         "dist": {"channels": 1, "activation": "relu", "loss": "WeightedDistanceGradientLoss", "weight": 0.25}}
SHAPE = (4, 1, 256, 256)
SUP = [0.5, 0.75, 0.875, 1.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--count-launches", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    m = B.MultiOutputNestedUNet(in_channels=1, output_heads=HEADS, n_filter=64, deep_supervision=True).cuda().train()
    m.set_compute_dtype(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(1)
    n, _, h, w = SHAPE
    x = torch.rand(SHAPE, device="cuda", generator=g)
    tg = {"seg": (torch.rand((n, 1, h, w), device="cuda", generator=g) > 0.5).float(),
          "vec": torch.randn((n, 2, h, w), device="cuda", generator=g) * (torch.rand((n, 1, h, w), device="cuda", generator=g) < 0.6).float(),
          "dist": (torch.rand((n, 1, h, w), device="cuda", generator=g) < 0.6).float() * torch.rand((n, 1, h, w), device="cuda", generator=g)}
    keys = [f"{name}_{l}" for name in HEADS for l in range(1, 5)]
    seeds = {k: torch.randn((n, HEADS[k.rsplit('_', 1)[0]]["channels"], h, w), device="cuda", generator=g) * 1e-6 for k in keys}
    crit = {name: L.get_loss_function(cfg["loss"]) for name, cfg in HEADS.items()}
    fused = L.MultiHeadLoss(HEADS, deep_supervision=True, levels=4, loss_functions=crit)
    params = [p for p in m.parameters()]

    def zero():
        for p in params:
            p.grad = None

    def step_a():
        zero()
        out = m(x)
        torch.autograd.backward([out[k] for k in keys], [seeds[k] for k in keys])
        torch.cuda.synchronize()

    def step_b():
        zero()
        out = m(x)
        total = 0
        for name, cfg in HEADS.items():
            for level, sw in enumerate(SUP, 1):
                total = total + sw * cfg["weight"] * crit[name]._torch(out[f"{name}_{level}"], tg[name])
        total.backward()
        return total.item()

    def step_c():
        zero()
        total = fused(m(x), tg)
        total.backward()
        return fused.item()

    steps = {"a": step_a, "b": step_b, "c": step_c}
    order = [a.only] if a.only else ["a", "b", "c"]
    wall = {k: [] for k in order}
    dev = {k: [] for k in order}
    vals = {}
    for i in range(a.warmup + a.steps):
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            v = steps[k]()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if v is not None:
                vals[k] = v
            if i >= a.warmup:
                wall[k].append((t1 - t0) * 1e3)
                dev[k].append(e0.elapsed_time(e1))
    res = {"model": "MultiOutputNestedUNet", "n_filter": 64, "dtype": "bf16", "shape": list(SHAPE), "heads": {k: v["loss"] for k, v in HEADS.items()},
           "levels": 4, "steps": a.steps, "warmup": a.warmup, "interleaved": a.only is None}
    for k in order:
        res[f"{k}_wall_ms_median"] = round(statistics.median(wall[k]), 3)
        res[f"{k}_wall_ms_min"] = round(min(wall[k]), 3)
        res[f"{k}_wall_ms_p90"] = round(sorted(wall[k])[int(0.9 * (len(wall[k]) - 1))], 3)
        res[f"{k}_device_ms_median"] = round(statistics.median(dev[k]), 3)
    if a.only is None:
        res["loss_side_torch_ms (b-a, wall median)"] = round(res["b_wall_ms_median"] - res["a_wall_ms_median"], 3)
        res["loss_side_fused_ms (c-a, wall median)"] = round(res["c_wall_ms_median"] - res["a_wall_ms_median"], 3)
        res["loss_side_torch_ms (b-a, device median)"] = round(res["b_device_ms_median"] - res["a_device_ms_median"], 3)
        res["loss_side_fused_ms (c-a, device median)"] = round(res["c_device_ms_median"] - res["a_device_ms_median"], 3)
        res["total_b"], res["total_c"] = vals.get("b"), vals.get("c")
    if a.count_launches:
        before = L.launches
        step_c()
        res["fused_loss_launches_per_step"] = L.launches - before
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
