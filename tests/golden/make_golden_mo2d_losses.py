"""Generate ``mo2d_losses.npz`` in this directory from the REFERENCE criteria of the 2-D multi-output trainer.

Run in the build container only (the reference is absent on the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mo2d_losses.py

``multi_output_unet/losses.py`` imports nothing but torch; it is loaded by file path with ``make_golden.load``.  Only tensors and a JSON
meta blob leave this script.  Per case the fixture holds the loss and ``d loss / d input`` of the reference class evaluated in float64
and in float32 on the same (float32-representable) inputs, and the float32-vs-float64 deviation (relative to the value for the loss, to
the largest gradient entry for the gradient): the tests bound the HIP kernels by a multiple of that deviation.

  meta_json                    {"cases": [{name, cls, kwargs, set, grad}], "ds": {...}}
  in.<set>.x / .t              shared inputs (float32): prob_* probabilities strictly inside (0, 1) against binary masks, reg_* regression
                               pairs, vec_* two-channel vector fields; *_main is 2 x C x 32 x 48, *_odd 2 x 2 x 5 x 7
  <case>.loss64 / .loss32 / .grad64 / .grad32 / .dev_loss / .dev_grad
  bce_clamp.*                  forward only: exact 0 and 1 against mismatching targets pin nn.BCELoss's -100 clamp (66.8977)
  ds.*                         one deep-supervision total, three heads x four levels, by the loop of multi_output_unet/train.py:157-181
"""
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402

R = G.load("ref_mo2d_losses", "multi_output_unet/losses.py")

CASES = [
    ("bcedice", "BCEDiceLoss", dict(bce_weight=0.3, dice_weight=0.7), "prob"),
    ("dice", "BCEDiceLoss", dict(bce_weight=0, dice_weight=1), "prob"),
    ("tversky", "TverskyLoss", dict(alpha=0.3, beta=0.7, smooth=0.5), "prob"),
    ("logcosh_tversky", "logcoshTverskyLoss", dict(alpha=0.6, beta=0.4, smooth=2), "prob"),
    ("mse", "MSELoss", {}, "reg"),
    ("mae", "MAELoss", {}, "reg"),
    ("huber", "HuberLoss", dict(delta=0.5), "reg"),
    ("distgrad", "DistanceGradientLoss", dict(alpha=0.7), "reg"),
    ("wdistgrad", "WeightedDistanceGradientLoss", dict(alpha=0.6, beta=0.7), "reg"),
    ("wvf", "WeightedVectorFieldLoss", dict(beta=0.7, magnitude_weight=0.45), "vec"),
]
SHAPES = {"main": {"prob": (2, 1, 32, 48), "reg": (2, 1, 32, 48), "vec": (2, 2, 32, 48)},
          "odd": {"prob": (2, 2, 5, 7), "reg": (2, 2, 5, 7), "vec": (2, 2, 5, 7)}}


def draw(kind, shape, g):
    if kind == "prob":
        x = torch.rand(shape, generator=g) * 0.98 + 0.01
        t = (torch.rand(shape, generator=g) < 0.4).float()
        assert float(x.min()) > 0 and float(x.max()) < 1
    elif kind == "reg":
        x = torch.randn(shape, generator=g) * 0.6
        t = (torch.rand(shape, generator=g) < 0.6).float() * torch.rand(shape, generator=g) * 1.5
        frac = float((t > 0).float().mean())
        assert 0.2 <= frac <= 0.8, frac
        small = float(((x - t).abs() < 0.5).float().mean())
        assert 0.25 <= small <= 0.75, small            # both Huber branches (delta = 0.5) hold at least a quarter of the elements
    else:
        n, _, h, w = shape
        x = torch.randn(shape, generator=g) * 0.7
        t = torch.randn(shape, generator=g) * (torch.rand((n, 1, h, w), generator=g) < 0.6).float()
        zero = float(((t[:, 0] == 0) & (t[:, 1] == 0)).float().mean())
        assert 0.2 <= zero <= 0.8, zero
    return x, t


def run(crit, x, t, dt, grad=True):
    xi = x.to(dt).clone().requires_grad_(grad)
    loss = crit(xi, t.to(dt))
    if grad:
        loss.backward()
    return loss.detach(), (xi.grad.detach() if grad else None)


def main():
    g = torch.Generator().manual_seed(2024)
    arrays, meta = {}, {"cases": []}
    sets = {}
    for size, by_kind in SHAPES.items():
        for kind, shape in by_kind.items():
            sets[f"{kind}_{size}"] = draw(kind, shape, g)
    for k, (x, t) in sets.items():
        arrays[f"in.{k}.x"], arrays[f"in.{k}.t"] = x.numpy(), t.numpy()
    for name, cls, kw, kind in CASES:
        assert cls in ("MSELoss", "MAELoss") or kw, name          # non-default arguments for every parametrised class
        for size in SHAPES:
            case = f"{name}_{size}"
            x, t = sets[f"{kind}_{size}"]
            crit = getattr(R, cls)(**kw)
            l64, g64 = run(crit, x, t, torch.float64)
            l32, g32 = run(crit, x, t, torch.float32)
            arrays[f"{case}.loss64"], arrays[f"{case}.loss32"] = l64.numpy(), l32.numpy()
            arrays[f"{case}.grad64"], arrays[f"{case}.grad32"] = g64.numpy(), g32.numpy()
            arrays[f"{case}.dev_loss"] = np.float64(abs(float(l32) - float(l64)) / abs(float(l64)))
            arrays[f"{case}.dev_grad"] = np.float64(float((g32.double() - g64).abs().max()) / float(g64.abs().max()))
            meta["cases"].append(dict(name=case, cls=cls, kwargs=kw, set=f"{kind}_{size}", grad=True))
            print(f"{case:28s} loss {float(l64):.8f}  dev {float(arrays[f'{case}.dev_loss']):.2e} / {float(arrays[f'{case}.dev_grad']):.2e}")
    # the -100 clamp, forward only
    x, t = torch.tensor([0.0, 1.0, 0.5]).view(1, 1, 1, 3), torch.tensor([1.0, 0.0, 1.0]).view(1, 1, 1, 3)
    crit = R.BCEDiceLoss(bce_weight=1, dice_weight=0)
    l64, _ = run(crit, x, t, torch.float64, grad=False)
    l32, _ = run(crit, x, t, torch.float32, grad=False)
    assert abs(float(l64) - 66.8977) < 1e-4, float(l64)
    arrays["in.clamp.x"], arrays["in.clamp.t"] = x.numpy(), t.numpy()
    arrays["bce_clamp.loss64"], arrays["bce_clamp.loss32"] = l64.numpy(), l32.numpy()
    arrays["bce_clamp.dev_loss"] = np.float64(abs(float(l32) - float(l64)) / abs(float(l64)))
    meta["cases"].append(dict(name="bce_clamp", cls="BCEDiceLoss", kwargs=dict(bce_weight=1, dice_weight=0), set="clamp", grad=False))
    # one deep-supervision total: the loop of multi_output_unet/train.py:157-181 with levels = 4
    heads = {"seg": {"channels": 1, "loss": "BCEDiceLoss", "weight": 1.0, "kind": "prob"},
             "vec": {"channels": 2, "loss": "WeightedVectorFieldLoss", "weight": 0.5, "kind": "vec"},
             "dist": {"channels": 1, "loss": "WeightedDistanceGradientLoss", "weight": 0.25, "kind": "reg"}}
    sup = [0.5, 0.75, 0.875, 1.0]
    fns = {"seg": R.BCEDiceLoss(), "vec": R.WeightedVectorFieldLoss(), "dist": R.WeightedDistanceGradientLoss()}
    preds, tgts = {}, {}
    for name, cfg in heads.items():
        shape = (2, cfg["channels"], 16, 24)
        for level in range(1, 5):
            preds[f"{name}_{level}"], tg = draw(cfg["kind"], shape, g)
        tgts[name] = tg
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        total = 0
        for name, cfg in heads.items():
            for level, weight in enumerate(sup, 1):
                total += weight * cfg["weight"] * fns[name](preds[f"{name}_{level}"].to(dt), tgts[name].to(dt))
        arrays[f"ds.total{tag}"] = total.numpy()
    for k, v in preds.items():
        arrays[f"ds.pred.{k}"] = v.numpy()
    for k, v in tgts.items():
        arrays[f"ds.target.{k}"] = v.numpy()
    arrays["ds.dev"] = np.float64(abs(float(arrays["ds.total32"]) - float(arrays["ds.total64"])) / abs(float(arrays["ds.total64"])))
    meta["ds"] = {"heads": {k: {kk: vv for kk, vv in v.items() if kk != "kind"} for k, v in heads.items()}, "levels": 4, "sup": sup}
    arrays["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(G.HERE, "mo2d_losses.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes; ds total", float(arrays["ds.total64"]), "dev", float(arrays["ds.dev"]))
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
