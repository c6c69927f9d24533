"""Generate ``mo3d_losses.npz`` in this directory from the REFERENCE criteria of the 3-D multi-output trainer.

Run in the build container only (the reference is absent on the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mo3d_losses.py

``multi_output_unet3d/losses.py`` imports nothing but torch; it is loaded by file path with ``make_golden.load``.  Only tensors and a JSON
meta blob leave this script.  Per case the fixture holds the loss and ``d loss / d logits`` of the reference class evaluated in float64
and in float32 on the same (float32-representable) inputs, and the float32-vs-float64 deviation (relative to the value for the loss, to
the largest gradient entry for the gradient): the tests bound the HIP kernels by a multiple of that deviation.

  meta_json                    {"cases": [{name, cls, args, set, grad}]}
  in.<set>.x / .t              shared inputs (float32): logits ``randn * 2`` against binary masks of density 0.4; ``odd`` is
                               2 x 2 x 5 x 6 x 7 (neither C D H W nor H W a multiple of 4), ``pair`` 2 x 1 x 2 x 8 x 8 (a single z-pair)
  <case>.loss64 / .loss32 / .grad64 / .grad32 / .dev_loss / .dev_grad

No z-neighbour pair of ``x`` is closer than 1e-4 (the seed moves on until that holds), so the ``sign`` of the temporal gradient is the
same in float32 and float64.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402

R = G.load("ref_mo3d_losses", "multi_output_unet3d/losses.py")

# (case, class, positional arguments): the five names as Trainer._get_loss_function constructs them (train.py:149-162), then one
# non-default parameter set each for BCEDice, Tversky and logcoshTversky
CASES = [
    ("bcedice", "BCEDiceLoss", [1, 1]),
    ("dice", "BCEDiceLoss", [0, 1]),
    ("tversky", "TverskyLoss", []),
    ("logcosh_tversky", "logcoshTverskyLoss", []),
    ("temporal", "BCEDiceTemporalLoss", []),
    ("bcedice_p", "BCEDiceLoss", [0.3, 0.7]),
    ("tversky_p", "TverskyLoss", [0.3, 0.7, 0.5]),
    ("logcosh_tversky_p", "logcoshTverskyLoss", [0.6, 0.4, 2]),
]
SHAPES = {"odd": (2, 2, 5, 6, 7), "pair": (2, 1, 2, 8, 8)}
MIN_GAP = 1e-4


def draw(shape, seed):
    while True:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(shape, generator=g) * 2
        t = (torch.rand(shape, generator=g) < 0.4).float()
        gap = float((x[:, :, 1:] - x[:, :, :-1]).abs().min())
        if gap >= MIN_GAP:
            return x, t, seed, gap
        seed += 1


def run(crit, x, t, dt):
    xi = x.to(dt).clone().requires_grad_(True)
    loss = crit(xi, t.to(dt))
    loss.backward()
    return loss.detach(), xi.grad.detach()


def main():
    arrays, meta = {}, {"cases": [], "seeds": {}}
    sets = {}
    for i, (name, shape) in enumerate(SHAPES.items()):
        x, t, seed, gap = draw(shape, 3000 + 100 * i)
        assert float((x[:, :, 1:] - x[:, :, :-1]).abs().min()) >= MIN_GAP
        sets[name] = (x, t)
        meta["seeds"][name] = seed
        arrays[f"in.{name}.x"], arrays[f"in.{name}.t"] = x.numpy(), t.numpy()
        print(f"set {name}: shape {shape} seed {seed} closest z-pair {gap:.3e}")
    for name, cls, args in CASES:
        for size, (x, t) in sets.items():
            case = f"{name}_{size}"
            crit = getattr(R, cls)(*args)
            l64, g64 = run(crit, x, t, torch.float64)
            l32, g32 = run(crit, x, t, torch.float32)
            arrays[f"{case}.loss64"], arrays[f"{case}.loss32"] = l64.numpy(), l32.numpy()
            arrays[f"{case}.grad64"], arrays[f"{case}.grad32"] = g64.numpy(), g32.numpy()
            arrays[f"{case}.dev_loss"] = np.float64(abs(float(l32) - float(l64)) / abs(float(l64)))
            arrays[f"{case}.dev_grad"] = np.float64(float((g32.double() - g64).abs().max()) / float(g64.abs().max()))
            meta["cases"].append(dict(name=case, cls=cls, args=args, set=size, grad=True))
            print(f"{case:28s} loss {float(l64):.8f}  dev {float(arrays[f'{case}.dev_loss']):.2e} / {float(arrays[f'{case}.dev_grad']):.2e}")
    arrays["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(G.HERE, "mo3d_losses.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
