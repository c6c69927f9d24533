"""Criteria of the 3-D multi-output trainer (``bio_image_unet/multi_output_unet3d/losses.py``): same class names, constructor arguments
and ``forward(logits, targets)`` as the reference.  They treat the tensor the model returned for a head as LOGITS (``p = sigmoid(x)``).

On CUDA fp32 contiguous ``[N, C, D, H, W]`` tensors of equal shape every criterion is one fused pass each way (``biu_mo3d_loss_*``,
``csrc/biu_mo3d_loss.hip``); otherwise (CPU tensors, other dtypes, other ranks) the plain torch composition below runs.
:class:`MultiHeadLoss` evaluates the trainer's whole ``sum_heads weight_h * criterion_h(pred_h, target_h)``
(``multi_output_unet3d/train.py``) as ONE autograd node: a forward launch per head plus one finishing launch, and one coefficient launch
plus a backward launch per head.  The temporal term of ``BCEDiceTemporalLoss`` (L1 between neighbouring z-planes) rides in the same two
passes, and the validation pass's second activation is applied in the forward kernel's registers.

The single-head criteria of ``bio_image_unet_amd.losses`` (the other families) run on the same plan and the same autograd function, as
one-term plans; their batch-axis SmoothL1 "time" term (``_Plan(time_weight=...)``) is a term of the table with two launches of its own.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F
from torch import nn

from .._lib import biu_mo3d_term, check, lib, stream as _stream
from ..losses import K_BCEDICE, K_LCTVERSKY, K_PAIRSL1, K_TEMPORAL, K_TVERSKY, soft_dice, tversky_index

MAX_TERMS, SLOTS, SAVED_HEADER = 16, 8, 32
ACT_CODE = {"sigmoid": 1, "tanh": 2, "relu": 3}      # engine._ACT_CODE; anything else is no activation, softmax goes through torch

launches = 0      # biu_mo3d_loss_* / biu_pair_smooth_l1_* calls issued by this module (tests assert the launch plan with it)


def _fusable(logits, targets):
    return (torch.is_tensor(logits) and torch.is_tensor(targets) and logits.is_cuda and logits.dtype == torch.float32
            and targets.dtype == torch.float32 and logits.shape == targets.shape and logits.dim() == 5 and logits.is_contiguous()
            and targets.is_contiguous() and logits.numel() > 0 and logits.shape[0] <= 65535)


def _call(name, *args):
    global launches
    launches += 1
    check(getattr(lib, name)(*args), name[4:])


def _p(t, floats=0):
    return C.c_void_p(t.data_ptr() + 4 * floats)


class _Plan:
    """The launch plan of one configuration: per head (criterion, shape, weight) its slice of the partial workspace, its first row of
    ``saved`` / ``coef``, and the term table ``biu_mo3d_loss_finish`` / ``_coef`` read, uploaded once.  ``time_weight`` appends the
    K_PAIRSL1 term on the first head's tensor: ``time_weight * SmoothL1(x[1:], x[:-1])`` over the batch axis (n > 1)."""

    def __init__(self, heads, device, time_weight=0.0):
        self.heads, terms, off, row, goff = [], [], 0, 0, 0
        for crit, shape, weight in heads:
            n, c, d, h, w = shape
            numel = n * c * d * h * w
            rows = lib.biu_mo3d_loss_blocks(numel)
            p = crit._params()
            self.heads.append((crit.kind, shape, off, row, goff, numel))
            terms.append(biu_mo3d_term(crit.kind, rows, off, n, numel // n, n * c * (d - 1) * h * w, p[0], p[1], p[2], float(weight)))
            off += n * rows * SLOTS
            row += n
            goff += (numel + 3) // 4 * 4          # every head's gradient starts 16-byte aligned in the one buffer
        self.pair = None
        if time_weight:
            n, per = heads[0][1][0], self.heads[0][5] // heads[0][1][0]
            rows = lib.biu_pair_smooth_l1_blocks((n - 1) * per)
            self.pair = (n, per, off, row)
            terms.append(biu_mo3d_term(K_PAIRSL1, rows, off, 1, per, (n - 1) * per, 0.0, 0.0, 0.0, float(time_weight)))
            off += rows * SLOTS
            row += 1
        self.ws_floats, self.nterms, self.nrows, self.grad_floats = off, len(terms), row, goff
        raw = bytes((biu_mo3d_term * len(terms))(*terms))
        self.terms = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        self.saved = None


class _FusedMo3d(torch.autograd.Function):
    """``sum_heads weight * criterion(x, target)`` over the heads of a :class:`_Plan` (``include/biu.h``: biu_mo3d_loss_*).  ``codes`` are
    the heads' ``pre_act`` codes, forward only: a head that needs a gradient arrives activated, with code 0."""

    @staticmethod
    def forward(ctx, plan, targets, codes, *xs):
        dev = xs[0].device
        ws = torch.empty(plan.ws_floats, dtype=torch.float32, device=dev)
        saved = torch.empty(SAVED_HEADER + SLOTS * plan.nrows, dtype=torch.float32, device=dev)
        st = _stream()
        for (kind, (n, c, d, h, w), off, _, _, _), x, tg, code in zip(plan.heads, xs, targets, codes):
            _call("biu_mo3d_loss_fwd", kind, code, _p(x), _p(tg), n, c, d, h, w, _p(ws, off), st)
        if plan.pair:
            n, per, off, _ = plan.pair
            _call("biu_pair_smooth_l1_fwd", _p(xs[0]), n, per, _p(ws, off), st)
        _call("biu_mo3d_loss_finish", _p(plan.terms), plan.nterms, _p(ws), _p(saved), st)
        assert not any(codes) or not any(ctx.needs_input_grad), "pre_act is forward only"
        ctx.save_for_backward(*xs)
        ctx.plan, ctx.targets, ctx.saved = plan, targets, saved
        plan.saved = saved
        return saved[0]

    @staticmethod
    def backward(ctx, g):
        plan, xs, saved = ctx.plan, ctx.saved_tensors, ctx.saved
        g = g.reshape(1).to(torch.float32).contiguous()
        coef = torch.empty(plan.nrows * 4, dtype=torch.float32, device=g.device)
        st = _stream()
        _call("biu_mo3d_loss_coef", _p(plan.terms), plan.nterms, _p(g), _p(saved), _p(coef), st)
        # the gradients of all heads in one go; a single head needs no views
        flat = torch.empty(plan.grad_floats, dtype=torch.float32, device=g.device) if len(xs) > 1 else None
        grads = []
        for (kind, (n, c, d, h, w), _, row, goff, numel), x, tg in zip(plan.heads, xs, ctx.targets):
            dx = flat[goff:goff + numel].view(x.shape) if flat is not None else torch.empty_like(x)
            _call("biu_mo3d_loss_bwd", kind, _p(x), _p(tg), n, c, d, h, w, _p(coef, 4 * row), _p(dx), st)
            grads.append(dx)
        if plan.pair:
            n, per, _, row = plan.pair
            _call("biu_pair_smooth_l1_bwd", _p(xs[0]), n, per, _p(coef, 4 * row), _p(grads[0]), 1, st)
        return (None, None, None) + tuple(grads)


class _Criterion(nn.Module):
    kind = -1

    def _params(self):        # (p0, p1, p2) of biu_mo3d_term
        return (0.0, 0.0, 0.0)

    def _torch(self, logits, targets):
        raise NotImplementedError

    def forward(self, logits, targets):
        if not _fusable(logits, targets):
            return self._torch(logits, targets)
        shape = tuple(logits.shape)
        plans = self.__dict__.setdefault("_plans", {})
        key = (shape, logits.device, self._params())
        if key not in plans:
            plans[key] = _Plan([(self, shape, 1.0)], logits.device)
        return _FusedMo3d.apply(plans[key], (targets,), (0,), logits)


class BCEDiceLoss(_Criterion):
    """``alpha * BCEWithLogits(mean) + beta * (1 - mean_n 2 (sum_n p t + 1) / (sum_n p + sum_n t + 1))`` (losses.py:81-116)."""
    kind = K_BCEDICE

    def __init__(self, alpha, beta):
        super().__init__()
        self.alpha, self.beta = alpha, beta

    def _params(self):
        return (float(self.alpha), float(self.beta), 1.0)          # p2: the Dice smooth

    def _torch(self, logits, targets):
        return self.alpha * F.binary_cross_entropy_with_logits(logits, targets) + self.beta * soft_dice(logits, targets)


class DiceLoss(BCEDiceLoss):
    """The trainer's ``"DiceLoss"``: ``BCEDiceLoss(0, 1)`` (train.py:149-162)."""

    def __init__(self):
        super().__init__(0, 1)


class TverskyLoss(_Criterion):
    """``1 - (TP + s) / (TP + alpha FP + beta FN + s)`` over the whole tensor (losses.py:150-197)."""
    kind = K_TVERSKY

    def __init__(self, alpha=0.5, beta=0.5, smooth=1):
        super().__init__()
        self.alpha, self.beta, self.smooth = alpha, beta, smooth

    def _params(self):
        return (float(self.alpha), float(self.beta), float(self.smooth))

    def _torch(self, inputs, targets):
        return 1 - tversky_index(torch.sigmoid(inputs), targets, self.alpha, self.beta, self.smooth)


class logcoshTverskyLoss(TverskyLoss):
    """``log cosh(1 - Tversky)`` (losses.py:200-247)."""
    kind = K_LCTVERSKY

    def _torch(self, inputs, targets):
        return torch.log(torch.cosh(1 - tversky_index(torch.sigmoid(inputs), targets, self.alpha, self.beta, self.smooth)))


class TemporalConsistencyLoss(nn.Module):
    """L1 between consecutive slices of axis 2 of a (B, C, Z, X, Y) prediction (losses.py:250-263); inside ``BCEDiceTemporalLoss`` it is
    part of the fused pass, on its own it is this torch composition."""

    def forward(self, predictions):
        return F.l1_loss(predictions[:, :, 1:, :, :], predictions[:, :, :-1, :, :])


class BCEDiceTemporalLoss(_Criterion):
    """``w0 * BCEDice(1, 1) + w1 * mean |x[:, :, 1:] - x[:, :, :-1]|`` (losses.py:266-298); ``nan`` at ``D = 1``, as the reference."""
    kind = K_TEMPORAL

    def __init__(self, loss_params=(1.0, 0.1)):
        super().__init__()
        self.bce_dice_loss = BCEDiceLoss(1, 1)
        self.temporal_consistency_loss = TemporalConsistencyLoss()
        self.loss_params = loss_params

    def _params(self):
        return (float(self.loss_params[0]), float(self.loss_params[1]), 0.0)

    def _torch(self, predictions, targets):
        return (self.loss_params[0] * self.bce_dice_loss._torch(predictions, targets) +
                self.loss_params[1] * self.temporal_consistency_loss(predictions))


LOSS_TABLE = {"BCEDiceLoss": lambda: BCEDiceLoss(1, 1), "DiceLoss": lambda: BCEDiceLoss(0, 1), "TverskyLoss": TverskyLoss,
              "logcoshTverskyLoss": logcoshTverskyLoss, "BCEDiceTemporalLoss": BCEDiceTemporalLoss}


def get_loss_function(loss_name):
    """``Trainer._get_loss_function`` (train.py:149-162): the five names."""
    if loss_name not in LOSS_TABLE:
        raise ValueError(f'Loss "{loss_name}" not defined!')
    return LOSS_TABLE[loss_name]()


_FIVE = (BCEDiceLoss, DiceLoss, TverskyLoss, logcoshTverskyLoss, BCEDiceTemporalLoss)


def _activate(x, activation):
    fn = {"sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu, "softmax": lambda t: torch.softmax(t, dim=1)}
    return fn[activation](x) if activation in fn else x


class MultiHeadLoss(nn.Module):
    """The trainer's total over all heads as one autograd node.

    ``output_heads``: the network's head dictionary (``'loss'`` names a criterion of this module, ``'weight'`` defaults to 1);
    ``loss_functions`` overrides the criteria by head name.  ``forward(pred, targets, pre_activations=None)`` takes the network's output
    dictionary and the targets by head name (``[N, D, H, W]`` targets gain a channel axis).  ``pre_activations`` names per head an
    activation applied to the prediction before its criterion -- the validation pass of the reference, which activates the already
    activated outputs once more: sigmoid, tanh and relu run in the forward kernel's registers when no gradient is required, softmax (and
    any activation under autograd) runs in torch first.  Heads whose criterion is not one of this module's five, or whose tensors are not
    fusable, are evaluated per class and added in torch."""

    def __init__(self, output_heads, loss_functions=None):
        super().__init__()
        self.output_heads = output_heads
        self.loss_functions = dict(loss_functions or {name: get_loss_function(cfg["loss"]) for name, cfg in output_heads.items()})
        self.loss_weights = {name: cfg.get("weight", 1.0) for name, cfg in output_heads.items()}
        self._plans = {}

    def forward(self, pred, targets, pre_activations=None):
        fused, rest, total = [], [], 0
        for name in self.output_heads:
            x, tg = pred[name], targets[name]
            if tg.dim() == 4:
                tg = tg.unsqueeze(1)
            crit, wt = self.loss_functions[name], self.loss_weights[name]
            act = pre_activations.get(name) if pre_activations else None
            code = ACT_CODE.get(act, 0)
            if act == "softmax" or (code and torch.is_grad_enabled() and x.requires_grad):
                x, code = _activate(x, act), 0
            if type(crit) in _FIVE and _fusable(x, tg) and len(fused) < MAX_TERMS:
                fused.append((crit, x, tg, wt, code))
            else:
                rest.append((crit, _activate(x, act) if code else x, tg, wt))
        if fused:
            dev = fused[0][1].device
            key = tuple((c.kind, c._params(), tuple(x.shape), float(w)) for c, x, _, w, _ in fused) + (dev,)
            if key not in self._plans:
                self._plans[key] = _Plan([(c, tuple(x.shape), w) for c, x, _, w, _ in fused], dev)
            total = _FusedMo3d.apply(self._plans[key], tuple(f[2] for f in fused), tuple(f[4] for f in fused), *[f[1] for f in fused])
        for crit, x, tg, wt in rest:
            total = total + wt * crit(x, tg)
        return total
