"""Loss criteria of the reference trainers (the scalar the backward pass starts from): reductions over the fp32 logits tensor the
head kernel emits.  BCEDiceLoss, TverskyLoss and logcoshTverskyLoss run as fused passes on the multi-head loss kernels
(:class:`_SegCriterion`) where :func:`_fusable` holds; the rest, and every other input, is the torch composition.

Mirrors ``bio_image_unet/unet/losses.py``: BCELoss2d (:5-37), SoftDiceLoss (:40-75), BCEDiceLoss (:78-112),
logcoshDiceLoss (:115-142), TverskyLoss (:145-191), logcoshTverskyLoss (:194-239) -- same class names, constructor
arguments and forward(logits, targets) contract.
"""
import math

import torch
from torch import nn


class BCELoss2d(nn.Module):
    def __init__(self, weight=None, size_average=True):
        super().__init__()
        self.bce_loss = nn.BCEWithLogitsLoss(weight=weight, reduction="mean" if size_average else "sum")

    def forward(self, logits, targets):
        return self.bce_loss(logits, targets)


K_BCEDICE, K_TVERSKY, K_LCTVERSKY, K_TEMPORAL, K_PAIRSL1 = range(5)      # the kinds of biu_mo3d_term (include/biu.h)


def soft_dice(logits, targets, smooth=1.0):
    n = targets.size(0)
    p, t = torch.sigmoid(logits).reshape(n, -1), targets.reshape(n, -1)
    score = 2.0 * ((p * t).sum(1) + smooth) / (p.sum(1) + t.sum(1) + smooth)
    return 1 - score.mean()


def tversky_index(probs, targets, alpha, beta, smooth):
    p, t = probs.reshape(-1), targets.reshape(-1)
    tp = (p * t).sum()
    fp = ((1 - t) * p).sum()
    fn = (t * (1 - p)).sum()
    return (tp + smooth) / (tp + alpha * fp + beta * fn + smooth)


class SoftDiceLoss(nn.Module):
    def __init__(self, smooth=1.0):
        super().__init__()
        self.smooth = smooth

    def forward(self, logits, targets):
        return soft_dice(logits, targets, self.smooth)


def _dims5(shape):
    """The ``[n, c, d, h, w]`` the loss kernels take: the real extents at rank 5, ``(n, c, 1, 1, rest)`` otherwise (only the elements per
    sample matter to these kinds)."""
    if len(shape) == 5:
        return tuple(shape)
    n, c = shape[0], (shape[1] if len(shape) > 1 else 1)
    return (n, c, 1, 1, math.prod(shape[1:]) // c)


def _fusable(logits, targets):
    """Whether the fused pass takes the call: CUDA fp32 contiguous tensors of equal shape and rank >= 1, at most 65535 samples (one grid
    row each) and every extent of :func:`_dims5` below 2**31 (the kernels take them as ``int``); anything else runs the torch composition."""
    return (logits.is_cuda and logits.dtype == torch.float32 and targets.dtype == torch.float32 and logits.shape == targets.shape
            and logits.is_contiguous() and targets.is_contiguous() and logits.numel() > 0 and logits.shape[0] <= 65535
            and (logits.numel() < 2 ** 31 or max(_dims5(logits.shape)) < 2 ** 31))


class _SegCriterion(nn.Module):
    """A single-head criterion is a one-term plan of the multi-head loss (``multi_output_unet3d.losses``: ``_Plan``, ``_FusedMo3d``;
    ``csrc/biu_mo3d_loss.hip``), two terms with the 3-D trainer's ``time_weight * SmoothL1(logits[1:], logits[:-1])``
    (unet3d/train.py:140-145): one autograd node, one pass over (logits, targets) each way."""
    kind = -1

    def _fused(self, logits, targets, time_weight):
        from .multi_output_unet3d import losses as M          # lazily, as _lib: the package's import order stays
        n = logits.shape[0]
        w = float(time_weight) if n > 1 else 0.0
        plans = self.__dict__.setdefault("_plans", {})
        key = (logits.shape, logits.device, self._params(), w)
        if key not in plans:
            plans[key] = M._Plan([(self, _dims5(logits.shape), 1.0)], logits.device, time_weight=w)
        loss = M._FusedMo3d.apply(plans[key], (targets,), (0,), logits)
        if time_weight and n <= 1:      # a batch of one: nn.SmoothL1Loss over empty slices is nan in the reference, and so here
            loss = loss + float("nan")
        return loss


class BCEDiceLoss(_SegCriterion):
    kind = K_BCEDICE

    def __init__(self, alpha, beta):
        super().__init__()
        self.bce, self.dice, self.alpha, self.beta = BCELoss2d(), SoftDiceLoss(), alpha, beta

    def _params(self):
        return (float(self.alpha), float(self.beta), float(self.dice.smooth))

    def forward(self, logits, targets, time_weight: float = 0.0):
        """``time_weight`` adds the 3-D trainer's ``SmoothL1(logits[1:], logits[:-1]) * time_weight`` to the same fused pass."""
        if _fusable(logits, targets):
            return self._fused(logits, targets, time_weight)
        loss = self.alpha * self.bce(logits, targets) + self.beta * self.dice(logits, targets)
        if time_weight:
            loss = loss + nn.functional.smooth_l1_loss(logits[1:], logits[:-1]) * time_weight
        return loss


class logcoshDiceLoss(nn.Module):
    def __init__(self):
        super().__init__()
        self.dice = SoftDiceLoss()

    def forward(self, logits, targets):
        x = self.dice(logits, targets)
        return torch.log((torch.exp(x) + torch.exp(-x)) / 2)


class TverskyLoss(_SegCriterion):
    kind = K_TVERSKY

    def __init__(self, alpha=0.5, beta=0.5, smooth=1):
        super().__init__()
        self.alpha, self.beta, self.smooth = alpha, beta, smooth

    def _params(self):
        return (float(self.alpha), float(self.beta), float(self.smooth))

    def forward(self, inputs, targets, time_weight: float = 0.0):
        if _fusable(inputs, targets):
            return self._fused(inputs, targets, time_weight)
        x = 1 - tversky_index(torch.sigmoid(inputs), targets, self.alpha, self.beta, self.smooth)
        loss = torch.log(torch.cosh(x)) if self.kind == K_LCTVERSKY else x
        if time_weight:
            loss = loss + nn.functional.smooth_l1_loss(inputs[1:], inputs[:-1]) * time_weight
        return loss


class logcoshTverskyLoss(TverskyLoss):
    kind = K_LCTVERSKY


class weightedBCELoss(nn.Module):
    """BCE on sigmoid(logits) with weight alpha where target >= 0.5, beta elsewhere, mean over elements
    (``siam_unet/losses.py:109-148``)."""

    def __init__(self, alpha=1, beta=0.1):
        super().__init__()
        self.alpha, self.beta = alpha, beta

    def forward(self, logits, targets):
        probs = torch.sigmoid(logits)
        weights = torch.where(targets >= 0.5, torch.full_like(targets, self.alpha), torch.full_like(targets, self.beta))
        return torch.mean(nn.functional.binary_cross_entropy(probs, targets, reduction="none") * weights)


class BCELoss2dProb(nn.Module):
    """The Siam package's ``BCELoss2d`` (``siam_unet/losses.py:73-105``): ``nn.BCELoss`` on ``sigmoid(logits)`` -- NOT
    ``BCEWithLogitsLoss``.  Same value in the bulk; where fp32 ``sigmoid`` saturates (|logit| > ~17) its log terms clamp at
    -100 and the gradient vanishes, which ``BCEWithLogits`` does not do, so the reference arithmetic is kept verbatim."""

    def __init__(self, weight=None, reduction="mean", **kwargs):
        super().__init__()
        self.bce_loss = nn.BCELoss(weight, reduction=reduction)

    def forward(self, logits, targets):
        return self.bce_loss(torch.sigmoid(logits).view(-1), targets.view(-1))


class BCEDiceLossSiam(nn.Module):
    """``siam_unet.BCEDiceLoss`` (``siam_unet/losses.py:5-39``): alpha * BCELoss(sigmoid) + beta * SoftDice
    (``score.sum() / num``, the same number as the 2-D package's ``score.mean()``)."""

    def __init__(self, alpha, beta):
        super().__init__()
        self.bce, self.dice, self.alpha, self.beta = BCELoss2dProb(), SoftDiceLoss(), alpha, beta

    def forward(self, logits, targets):
        return self.alpha * self.bce(logits, targets) + self.beta * self.dice(logits, targets)


class TemporalConsistencyLoss(nn.Module):
    """L1 between consecutive slices of axis 2 of a (B, C, Z, X, Y) prediction (``multi_output_unet3d/losses.py``)."""

    def forward(self, predictions):
        return nn.functional.l1_loss(predictions[:, :, 1:, :, :], predictions[:, :, :-1, :, :])


class BCEDiceTemporalLoss(nn.Module):
    """``w0 * BCEDice(1, 1) + w1 * TemporalConsistency`` (``multi_output_unet3d/losses.py``, default weights (1.0, 0.1))."""

    def __init__(self, loss_params=(1.0, 0.1)):
        super().__init__()
        self.bce_dice_loss = BCEDiceLoss(1, 1)
        self.temporal_consistency_loss = TemporalConsistencyLoss()
        self.loss_params = loss_params

    def forward(self, predictions, targets):
        return (self.loss_params[0] * self.bce_dice_loss(predictions, targets) +
                self.loss_params[1] * self.temporal_consistency_loss(predictions))
