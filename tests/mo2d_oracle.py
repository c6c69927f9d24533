"""Functional restatement of the 2-D multi-output networks of ``bio_image_unet.multi_output_unet`` -- TEST INFRASTRUCTURE.

``MultiOutputUnet.forward`` (multi_output_unet/multi_output_unet.py:91-134) and the nested U-Net++ forwards of
``MultiOutputNestedUNet`` / ``_3Levels`` (multi_output_nested_unet.py:116-156, 208-240), composed from ``oracle/unet_oracle.py``'s
own primitives so that fp64 runs, ``forced_decisions`` / ``record_decisions`` and ``emulate_bf16`` carry over unchanged.

A VGG block's ``conv1`` / ``bn1`` (``conv2`` / ``bn2``) are handed to ``unet_oracle.conv_block`` through an aliasing view with the
``{name}.0.*`` / ``{name}.1.*`` keys it reads: the same tensor objects, so gradients and running statistics land on the real keys.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import unet_oracle as O

State = Dict[str, torch.Tensor]


def _stage(sd: State, blk: str, i: int) -> State:
    v = {"s.0.weight": sd[f"{blk}.conv{i}.weight"], "s.0.bias": sd[f"{blk}.conv{i}.bias"]}
    for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        key = f"{blk}.bn{i}.{k}"
        if key in sd:
            v[f"s.1.{k}"] = sd[key]
    return v


def vgg_block(sd: State, blk: str, x: torch.Tensor, *, training: bool, dilation: int = 1) -> torch.Tensor:
    """``VGGBlock.forward`` (multi_output_nested_unet.py:44-55): two conv -> BatchNorm -> LeakyReLU(0.1) -> Dropout(0) stages."""
    x = O.conv_block(_stage(sd, blk, 1), "s", x, training=training, dilation=dilation)
    return O.conv_block(_stage(sd, blk, 2), "s", x, training=training, dilation=dilation)


def up_bilinear(t: torch.Tensor) -> torch.Tensor:
    """``nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True)`` (multi_output_nested_unet.py:73); the result is stored."""
    return O.st(F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True))


def _heads(sd: State, trunk: torch.Tensor, key: str, cfg: dict) -> torch.Tensor:
    return O.head_activation(F.conv2d(trunk, sd[f"output_layers.{key}.weight"], sd[f"output_layers.{key}.bias"]), cfg.get("activation"))


def mo2d_forward(sd: State, x: torch.Tensor, output_heads: Dict[str, dict], *, training: bool = True) -> Dict[str, torch.Tensor]:
    """``MultiOutputUnet.forward``: the 2-D U-Net body (dilation 1) and one activated 1x1 head per entry of ``output_heads``."""
    m4, skips = O._encoder2d(sd, O.emu_input(x), training, 1)
    t = O.conv_block(sd, "middle_conv1", m4, training=training)
    t = O.conv_block(sd, "middle_conv2", t, training=training)
    for lvl, skip in zip((1, 2, 3, 4), reversed(skips)):
        t = O.checked_concat(O.up_conv_t(sd, f"up{lvl}", t), skip)
        t = O.conv_block(sd, f"decode{2 * lvl - 1}", t, training=training)
        t = O.conv_block(sd, f"decode{2 * lvl}", t, training=training)
    return {name: _heads(sd, t, name, cfg) for name, cfg in output_heads.items()}


def nested_forward(sd: State, x: torch.Tensor, output_heads: Dict[str, dict], *, levels: int = 4, deep_supervision: bool = False,
                   train_mode: bool = True, dilation=False, training: bool = True,
                   cat_paths: Optional[Dict[str, str]] = None) -> Dict[str, torch.Tensor]:
    """The nested U-Net++ forward with ``levels`` pooling steps, in the reference's order of evaluation.  ``cat_paths`` (the engine's
    ``cat_paths``): a concatenation the engine materialised with a copy stores its prefix (matters for ``emulate_bf16`` only)."""
    L = levels
    dil = dilation if dilation is not False else (1,) * (L + 1)
    X = {(0, 0): vgg_block(sd, "conv0_0", O.emu_input(x), training=training, dilation=dil[0])}
    for k in range(1, L + 1):
        X[(k, 0)] = vgg_block(sd, f"conv{k}_0", O.st(O._maxpool(X[(k - 1, 0)])), training=training, dilation=dil[k])
        for j in range(1, k + 1):
            r = k - j
            prefix = torch.cat([X[(r, i)] for i in range(j)], 1)
            if cat_paths is not None and cat_paths.get(f"conv{r}_{j}") == "copy":
                prefix = O.st(prefix)
            X[(r, j)] = vgg_block(sd, f"conv{r}_{j}", torch.cat([prefix, up_bilinear(X[(r + 1, j - 1)])], 1), training=training)
    out = {}
    for name, cfg in output_heads.items():
        if deep_supervision and train_mode:
            for l in range(1, L + 1):
                out[f"{name}_{l}"] = _heads(sd, X[(0, l)], f"{name}_{l}", cfg)
            out[name] = out[f"{name}_{L}"]
        else:
            out[name] = _heads(sd, X[(0, L)], f"{name}_{L}" if deep_supervision else name, cfg)
    return out


def supervision_weights(levels: int):
    """The reference trainer's per-level weights (multi_output_unet/train.py:164-170)."""
    return {3: [0.5, 0.75, 1.0], 4: [0.5, 0.75, 0.875, 1.0]}[levels]


def weighted_mse(pred: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor], output_heads: Dict[str, dict], *,
                 deep_supervision: bool = False, levels: int = 4):
    """The reference trainer's total loss (multi_output_unet/train.py:157-180) with MSE as every head's criterion."""
    total = 0
    for name, cfg in output_heads.items():
        w = cfg.get("weight", 1.0)
        if deep_supervision:
            for l, sw in enumerate(supervision_weights(levels), 1):
                total = total + sw * w * F.mse_loss(pred[f"{name}_{l}"], targets[name])
        else:
            total = total + w * F.mse_loss(pred[name], targets[name])
    return total
