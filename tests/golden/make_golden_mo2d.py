"""Generate the fixtures of the 2-D multi-output networks in this directory from the REFERENCE implementation.

Run in the build container only (the reference is absent on the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mo2d.py

``multi_output_unet/multi_output_unet.py`` and ``multi_output_nested_unet.py`` import nothing but torch; they are loaded by file
path with ``make_golden.load`` and driven through ``make_golden.dump`` (same fixture layout as ``make_golden.py``, which this script
leaves untouched).  Only tensors leave it.  Every case: ``init_weights`` (kaiming normal on every Conv2d), batch 2, 32 x 48 inputs,
n_filter 2 for the four-level networks and 4 for the three-level one (each fixture stays under 1 MiB), loss = the reference trainer's (multi_output_unet/train.py:157-180) with MSE as each head's criterion.

``nested3_f4_ds``: ``MultiOutputNestedUNet_3Levels`` hands its ``dilation`` entries to ``VGGBlock``'s ``dropout`` position
(multi_output_nested_unet.py:174-177).  The fixture is built with ``dilation=(0, 0, 0, 0)`` there -- dropout 0, convolution dilation 1 --
which is what the package's ``MultiOutputNestedUNet_3Levels(dilation=False)`` computes ("Nested U-Net++").
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import make_golden as G  # noqa: E402

mo_mod = G.load("ref_multi_output_unet", "multi_output_unet/multi_output_unet.py")
nested_mod = G.load("ref_multi_output_nested_unet", "multi_output_unet/multi_output_nested_unet.py")

HEADS3 = {"seg": {"channels": 1, "activation": "sigmoid", "loss": "MSELoss", "weight": 1.0},
          "vec": {"channels": 2, "activation": None, "loss": "MSELoss", "weight": 0.5},
          "dist": {"channels": 1, "activation": "tanh", "loss": "MSELoss", "weight": 0.25}}
HEADS2 = {"seg": {"channels": 1, "activation": "sigmoid", "loss": "MSELoss", "weight": 1.0},
          "dist": {"channels": 1, "activation": "relu", "loss": "MSELoss", "weight": 0.5}}
SUP = {3: [0.5, 0.75, 1.0], 4: [0.5, 0.75, 0.875, 1.0]}
_clip = torch.nn.utils.clip_grad_norm_


def _clip_fresh_grads(params, max_norm, *a, **k):
    """``make_golden.dump`` stores ``p.grad.numpy()`` -- views of the gradients -- before it clips them in place; with a gradient norm
    above ``max_norm`` (these cases) the fixture would hold the clipped gradients.  Clip fresh copies instead."""
    params = list(params)
    for p in params:
        if p.grad is not None:
            p.grad = p.grad.clone()
    return _clip(params, max_norm, *a, **k)

LOSS = "multi_output_unet/train.py:157-186: sum_heads [sum_levels sup_l *] weight * MSE(activated out, target), clip_grad_norm_, Adam(1e-3)"


def case(name, model, ctor, ref_ctor, make, heads, levels, ds, clip):
    torch.manual_seed(11)
    m = make(**ref_ctor)
    m.apply(G.ref_init_weights)
    cin = ctor.get("in_channels", 1)
    x = torch.rand(2, cin, 32, 48)
    tgt = {k: torch.rand(2, v["channels"], 32, 48) for k, v in heads.items()}

    def loss_fn(outs):
        total = 0
        for k, v in heads.items():
            if ds:
                for lvl, sw in enumerate(SUP[levels], 1):
                    total = total + sw * v["weight"] * F.mse_loss(outs[f"{k}_{lvl}"], tgt[k])
            else:
                total = total + v["weight"] * F.mse_loss(outs[k], tgt[k])
        return total

    with torch.no_grad():
        names = list(m(x))
    torch.nn.utils.clip_grad_norm_ = _clip_fresh_grads
    G.dump(name, dict(model=model, ctor=ctor, levels=levels, seed=11, init="init_weights", loss=LOSS), m, {"x": x}, tgt, loss_fn, names,
           lambda mod, x=x: mod(x), clip=clip)
    torch.nn.utils.clip_grad_norm_ = _clip


def main():
    case("mo2d_f2", "MultiOutputUnet", dict(in_channels=1, output_heads=HEADS3, n_filter=2), dict(in_channels=1, output_heads=HEADS3, n_filter=2),
         mo_mod.MultiOutputUnet, HEADS3, 4, False, None)
    case("nested_f2", "MultiOutputNestedUNet", dict(in_channels=1, output_heads=HEADS3, n_filter=2),
         dict(in_channels=1, output_heads=HEADS3, n_filter=2), nested_mod.MultiOutputNestedUNet, HEADS3, 4, False, None)
    kw = dict(in_channels=2, output_heads=HEADS2, n_filter=2, deep_supervision=True, dilation=[1, 2, 1, 1, 2])
    case("nested_f2_ds", "MultiOutputNestedUNet", kw, kw, nested_mod.MultiOutputNestedUNet, HEADS2, 4, True, 1.0)
    case("nested3_f4_ds", "MultiOutputNestedUNet_3Levels", dict(in_channels=1, output_heads=HEADS2, n_filter=4, deep_supervision=True),
         dict(in_channels=1, output_heads=HEADS2, n_filter=4, deep_supervision=True, dilation=(0, 0, 0, 0)),
         nested_mod.MultiOutputNestedUNet_3Levels, HEADS2, 3, True, 1.0)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
