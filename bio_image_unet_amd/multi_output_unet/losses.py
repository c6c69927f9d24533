"""Criteria of the 2-D multi-output trainer (``bio_image_unet/multi_output_unet/losses.py``) on ACTIVATED head outputs: same class
names, constructor arguments and ``forward(inputs, targets)`` as the reference.

On CUDA fp32 contiguous tensors of equal shape every criterion is one fused pass each way (``biu_mo2d_loss_*``,
``csrc/biu_mo2d_loss.hip``); otherwise (CPU tensors, other dtypes, broadcast shapes) the plain torch composition below runs.
:class:`MultiHeadLoss` evaluates the trainer's whole ``sum_heads sum_levels sup_l * weight_h * criterion(pred, target)``
(``multi_output_unet/train.py:157-181``) as ONE autograd node: a forward launch per head plus one finishing launch, and one
coefficient launch plus a backward launch per head.

These differ from ``bio_image_unet_amd.losses`` (the other families' criteria, which take LOGITS): no sigmoid is applied here,
``BCEDiceLoss(bce_weight, dice_weight)`` sums over the whole tensor rather than per sample, and six of the ten are regression losses.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F
from torch import nn

from .._lib import stream as _stream
from ..losses import tversky_index

K_BCEDICE, K_TVERSKY, K_LCTVERSKY, K_MSE, K_MAE, K_HUBER, K_DGRAD, K_WDGRAD, K_WVF = range(9)
MAX_LEVELS, MAX_TERMS, SLOTS = 4, 32, 8

launches = 0      # biu_mo2d_loss_* calls issued by this module (tests assert the launch plan with it)


def _fusable(inputs, targets):
    return (torch.is_tensor(inputs) and torch.is_tensor(targets) and inputs.is_cuda and inputs.dtype == torch.float32
            and targets.dtype == torch.float32 and inputs.shape == targets.shape and inputs.dim() == 4 and inputs.is_contiguous()
            and targets.is_contiguous() and inputs.numel() > 0)


def _call(name, *args):
    global launches
    from .._lib import check, lib
    launches += 1
    check(getattr(lib, name)(*args), name[4:])


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _Plan:
    """The launch plan of one configuration: per head (criterion, shape, level weights) its slice of the partial workspace, and the
    term table ``biu_mo2d_loss_finish`` / ``_coef`` read, uploaded once."""

    def __init__(self, heads, device):
        from .._lib import biu_mo2d_term, lib
        self.heads, terms, off = [], [], 0
        for crit, shape, weights in heads:
            n, c, h, w = shape
            numel = n * c * h * w
            nb = lib.biu_mo2d_loss_blocks(numel)
            p = crit._params()
            self.heads.append((crit.kind, crit._elem(), shape, len(weights), off, len(terms)))
            for l, wt in enumerate(weights):
                terms.append(biu_mo2d_term(crit.kind, nb, off + l * nb * SLOTS, numel, n * h * w, p[0], p[1], p[2], float(wt)))
            off += len(weights) * nb * SLOTS
        self.ws_floats, self.nterms = off, len(terms)
        raw = bytes((biu_mo2d_term * len(terms))(*terms))
        self.terms = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        self.saved = None
        self.has_range = any(h[0] == K_BCEDICE for h in self.heads)


class _FusedMo2d(torch.autograd.Function):
    """``sum_terms weight * criterion(pred, target)`` over the heads and levels of a :class:`_Plan` (``include/biu.h``: biu_mo2d_loss_*).
    ``preds`` are the heads' level tensors, flattened in plan order."""

    @staticmethod
    def forward(ctx, plan, targets, *preds):
        dev = preds[0].device
        ws = torch.empty(plan.ws_floats, dtype=torch.float32, device=dev)
        saved = torch.empty(8 + 8 * plan.nterms, dtype=torch.float32, device=dev)
        st, k = _stream(), 0
        for (kind, (ea, eb), (n, c, h, w), nlev, off, _), tg in zip(plan.heads, targets):
            _call("biu_mo2d_loss_fwd", kind, ea, eb, _ptrs(preds[k:k + nlev]), nlev, C.c_void_p(tg.data_ptr()), n, c, h, w,
                  C.c_void_p(ws.data_ptr() + 4 * off), st)
            k += nlev
        _call("biu_mo2d_loss_finish", C.c_void_p(plan.terms.data_ptr()), plan.nterms, C.c_void_p(ws.data_ptr()), C.c_void_p(saved.data_ptr()), st)
        ctx.save_for_backward(*preds)
        ctx.plan, ctx.targets, ctx.saved = plan, targets, saved
        plan.saved = saved
        return saved[0]

    @staticmethod
    def backward(ctx, g):
        plan, preds, saved = ctx.plan, ctx.saved_tensors, ctx.saved
        g = g.reshape(1).to(torch.float32).contiguous()
        coef = torch.empty(plan.nterms * 4, dtype=torch.float32, device=g.device)
        st, k = _stream(), 0
        _call("biu_mo2d_loss_coef", C.c_void_p(plan.terms.data_ptr()), plan.nterms, C.c_void_p(g.data_ptr()), C.c_void_p(saved.data_ptr()),
              C.c_void_p(coef.data_ptr()), st)
        grads = [torch.empty_like(p) for p in preds]
        for (kind, (ea, eb), (n, c, h, w), nlev, _, t0), tg in zip(plan.heads, ctx.targets):
            _call("biu_mo2d_loss_bwd", kind, ea, eb, _ptrs(preds[k:k + nlev]), nlev, C.c_void_p(tg.data_ptr()), n, c, h, w,
                  C.c_void_p(coef.data_ptr() + 16 * t0), _ptrs(grads[k:k + nlev]), st)
            k += nlev
        return (None, None) + tuple(grads)


def check_range(saved):
    """The reference's ``assert torch.all((x >= 0) & (x <= 1))`` of ``BCEDiceLoss`` from the out-of-range counts the fused pass leaves
    in ``saved[1:3]`` (one host read)."""
    bad_in, bad_tg = saved[1:3].tolist()
    assert bad_in == 0, "Inputs must be between 0 and 1"
    assert bad_tg == 0, "Targets must be between 0 and 1"


class _Criterion(nn.Module):
    kind = -1

    def _params(self):        # (p0, p1, p2) of biu_mo2d_term
        return (0.0, 0.0, 0.0)

    def _elem(self):          # (ea, eb) of biu_mo2d_loss_fwd / _bwd
        return (0.0, 0.0)

    def _torch(self, inputs, targets):
        raise NotImplementedError

    def _fused(self, inputs, targets):
        shape = tuple(inputs.shape)
        plans = self.__dict__.setdefault("_plans", {})
        key = (shape, inputs.device, self._params(), self._elem())
        if key not in plans:
            plans[key] = _Plan([(self, shape, [1.0])], inputs.device)
        plan = plans[key]
        loss = _FusedMo2d.apply(plan, (targets,), inputs)
        if self.kind == K_BCEDICE:
            check_range(plan.saved)        # a criterion called on its own asserts at once, as the reference does
        return loss

    def forward(self, inputs, targets):
        if _fusable(inputs, targets):
            return self._fused(inputs, targets)
        return self._torch(inputs, targets)


# classification -------------------------------------------------------------------------------------------------------------------
class BCEDiceLoss(_Criterion):
    """``bce_weight * BCELoss(p, t) + dice_weight * (1 - (2 sum pt + 1e-5) / (sum p + sum t + 1e-5))``, sums over the whole tensor
    (losses.py:8-28)."""
    kind = K_BCEDICE

    def __init__(self, bce_weight=0.5, dice_weight=0.5):
        super().__init__()
        self.bce_weight, self.dice_weight = bce_weight, dice_weight
        self.bce = nn.BCELoss()

    def _params(self):
        return (float(self.bce_weight), float(self.dice_weight), 0.0)

    def _torch(self, inputs, targets):
        assert torch.all((inputs >= 0) & (inputs <= 1)), "Inputs must be between 0 and 1"
        assert torch.all((targets >= 0) & (targets <= 1)), "Targets must be between 0 and 1"
        smooth = 1e-5
        dice = 1 - (2. * (inputs * targets).sum() + smooth) / (inputs.sum() + targets.sum() + smooth)
        return self.bce_weight * self.bce(inputs, targets) + self.dice_weight * dice


class TverskyLoss(_Criterion):
    """``1 - (TP + s) / (TP + alpha FP + beta FN + s)`` on probabilities (losses.py:31-49)."""
    kind = K_TVERSKY

    def __init__(self, alpha=0.5, beta=0.5, smooth=1):
        super().__init__()
        self.alpha, self.beta, self.smooth = alpha, beta, smooth

    def _params(self):
        return (float(self.alpha), float(self.beta), float(self.smooth))

    def _torch(self, inputs, targets):
        return 1 - tversky_index(inputs, targets, self.alpha, self.beta, self.smooth)


class logcoshTverskyLoss(TverskyLoss):
    """``log cosh(1 - Tversky)`` (losses.py:52-70)."""
    kind = K_LCTVERSKY

    def _torch(self, inputs, targets):
        return torch.log(torch.cosh(1 - tversky_index(inputs, targets, self.alpha, self.beta, self.smooth)))


# regression -----------------------------------------------------------------------------------------------------------------------
class MSELoss(_Criterion):
    kind = K_MSE

    def _torch(self, inputs, targets):
        return ((inputs - targets) ** 2).mean()


class MAELoss(_Criterion):
    kind = K_MAE

    def _torch(self, inputs, targets):
        return torch.abs(inputs - targets).mean()


class HuberLoss(_Criterion):
    kind = K_HUBER

    def __init__(self, delta=1.0):
        super().__init__()
        self.delta = delta

    def _params(self):
        return (float(self.delta), 0.0, 0.0)

    def _elem(self):
        return (float(self.delta), 0.0)

    def _torch(self, inputs, targets):
        diff = torch.abs(inputs - targets)
        return torch.where(diff < self.delta, 0.5 * diff ** 2, self.delta * (diff - 0.5 * self.delta)).mean()


def gradient_loss(pred, target):
    """MSE between the spatial derivatives (``torch.gradient`` along H and W) of ``pred`` and ``target`` (losses.py:102-112)."""
    dy_t, dx_t = torch.gradient(target, dim=(-2, -1))
    dy_p, dx_p = torch.gradient(pred, dim=(-2, -1))
    return F.mse_loss(dy_p, dy_t) + F.mse_loss(dx_p, dx_t)


class DistanceGradientLoss(_Criterion):
    """``MSE + alpha * gradient_loss`` (losses.py:115-132)."""
    kind = K_DGRAD

    def __init__(self, alpha=1):
        super().__init__()
        self.alpha = alpha

    def _params(self):
        return (float(self.alpha), 0.0, 0.0)

    def _torch(self, pred, target):
        return F.mse_loss(pred, target) + self.alpha * gradient_loss(pred, target)


class WeightedDistanceGradientLoss(_Criterion):
    """MSE + MAE + ``alpha`` * gradient loss of ``pred * w`` against ``target * w``, ``w = beta`` where ``target > 0`` else ``1 - beta``
    (losses.py:135-153)."""
    kind = K_WDGRAD

    def __init__(self, alpha=1.0, beta=0.5):
        super().__init__()
        self.alpha, self.beta = alpha, beta

    def _params(self):
        return (float(self.alpha), float(self.beta), 0.0)

    def _elem(self):
        return (float(self.beta), 1.0 - float(self.beta))

    def _torch(self, pred, target):
        w = torch.where(target > 0, self.beta, 1.0 - self.beta)
        pw, tw = pred * w, target * w
        return F.mse_loss(pw, tw) + F.l1_loss(pw, tw) + self.alpha * gradient_loss(pw, tw)


class WeightedVectorFieldLoss(_Criterion):
    """Two-channel vector fields (B, 2, H, W): weighted MSE + MAE of the components plus ``magnitude_weight`` * MSE of the weighted squared
    magnitudes; ``w = beta`` where the true vector is non-zero, else ``1 - beta`` (losses.py:156-189)."""
    kind = K_WVF

    def __init__(self, beta=0.5, magnitude_weight=0.3):
        super().__init__()
        self.beta, self.magnitude_weight = beta, magnitude_weight

    def _params(self):
        return (float(self.beta), float(self.magnitude_weight), 0.0)

    def _elem(self):
        return (float(self.beta), 1.0 - float(self.beta))

    def forward(self, pred_vectors, true_vectors):
        if _fusable(pred_vectors, true_vectors) and pred_vectors.shape[1] == 2:
            return self._fused(pred_vectors, true_vectors)
        return self._torch(pred_vectors, true_vectors)

    def _torch(self, pred_vectors, true_vectors):
        valid = ~((true_vectors[:, 0] == 0) & (true_vectors[:, 1] == 0))
        w = torch.where(valid, self.beta, 1.0 - self.beta)
        pw, tw = pred_vectors * w[:, None], true_vectors * w[:, None]
        mag = F.mse_loss(torch.sum(pred_vectors ** 2, dim=1) * w, torch.sum(true_vectors ** 2, dim=1) * w)
        return F.mse_loss(pw, tw) + F.l1_loss(pw, tw) + self.magnitude_weight * mag


LOSS_TABLE = {
    "BCEDiceLoss": BCEDiceLoss, "DiceLoss": lambda: BCEDiceLoss(bce_weight=0, dice_weight=1), "TverskyLoss": TverskyLoss,
    "logcoshTverskyLoss": logcoshTverskyLoss, "MSELoss": MSELoss, "MAELoss": MAELoss, "HuberLoss": HuberLoss,
    "DistanceGradientLoss": DistanceGradientLoss, "WeightedDistanceGradientLoss": WeightedDistanceGradientLoss,
    "WeightedVectorFieldLoss": WeightedVectorFieldLoss,
}


def get_loss_function(loss_name):
    """``Trainer._get_loss_function`` (train.py:107-130): the ten names, default constructor arguments."""
    if loss_name not in LOSS_TABLE:
        raise ValueError(f'Loss "{loss_name}" not defined!')
    return LOSS_TABLE[loss_name]()


def supervision_weights(levels):
    """Weights of the deep-supervision levels (train.py:166-172)."""
    if levels == 3:
        return [0.5, 0.75, 1.0]
    if levels == 4:
        return [0.5, 0.75, 0.875, 1.0]
    raise ValueError(f'N = {levels} levels not valid. Choose N=3 or N=4 according to network architecture.')


class MultiHeadLoss(nn.Module):
    """The trainer's total over all heads and deep-supervision levels as one autograd node.

    ``output_heads``: the network's head dictionary (``'loss'`` names a criterion of this module, ``'weight'`` defaults to 1);
    ``loss_functions`` overrides the criteria by head name.  ``forward(outputs, targets)`` takes the network's output dictionary
    (``name_1 ... name_L`` under deep supervision, else ``name``) and the targets by head name (3-D targets gain a channel axis).
    Heads whose criterion is not one of this module's ten, or whose tensors are not fusable, are evaluated per class and added in torch.
    ``weights`` overrides the level weights for one call (the validation pass of the reference always uses three).

    The ``[0, 1]`` assertion of ``BCEDiceLoss`` is deferred: :meth:`item` reads the total and the out-of-range counts in one host read
    and raises ``AssertionError`` like the reference; :meth:`check_range` does the check alone."""

    def __init__(self, output_heads, deep_supervision=False, levels=4, loss_functions=None):
        super().__init__()
        self.output_heads, self.deep_supervision, self.levels = output_heads, deep_supervision, levels
        self.loss_functions = dict(loss_functions or {name: get_loss_function(cfg["loss"]) for name, cfg in output_heads.items()})
        self.loss_weights = {name: cfg.get("weight", 1.0) for name, cfg in output_heads.items()}
        self._plans, self._plan, self._total = {}, None, None

    def _level_weights(self, weights):
        if not self.deep_supervision:
            return None
        return list(weights) if weights is not None else supervision_weights(self.levels)

    def forward(self, outputs, targets, weights=None):
        sup = self._level_weights(weights)
        fused, rest, total = [], [], 0
        for name in self.output_heads:
            tg = targets[name]
            if tg.dim() == 3:
                tg = tg.unsqueeze(1)
            crit, hw = self.loss_functions[name], self.loss_weights[name]
            preds = [outputs[f"{name}_{l}"] for l in range(1, len(sup) + 1)] if sup else [outputs[name]]
            wts = [s * hw for s in sup] if sup else [hw]
            ok = (type(crit) in _TEN and len(preds) <= MAX_LEVELS and all(_fusable(p, tg) for p in preds)
                  and (crit.kind != K_WVF or tg.shape[1] == 2) and sum(len(f[2]) for f in fused) + len(preds) <= MAX_TERMS)
            (fused if ok else rest).append((crit, tg.contiguous() if ok else tg, wts, preds))
        self._plan = None
        if fused:
            dev = fused[0][3][0].device
            key = tuple((id(c), c._params(), c._elem(), tuple(t.shape), tuple(w)) for c, t, w, _ in fused) + (dev,)
            if key not in self._plans:
                self._plans[key] = _Plan([(c, tuple(t.shape), w) for c, t, w, _ in fused], dev)
            self._plan = plan = self._plans[key]
            total = _FusedMo2d.apply(plan, tuple(t for _, t, _, _ in fused), *[p for f in fused for p in f[3]])
        for crit, tg, wts, preds in rest:
            for wt, p in zip(wts, preds):
                total = total + wt * crit(p, tg)
        self._total = total
        return total

    def check_range(self):
        if self._plan is not None and self._plan.saved is not None and self._plan.has_range:
            check_range(self._plan.saved)

    def item(self):
        """The last total as a float, with the deferred range assertion, in one host read when every head was fused."""
        if self._plan is not None and self._total is not None and self._total.data_ptr() == self._plan.saved.data_ptr():
            v, bad_in, bad_tg = self._plan.saved[:3].tolist()
            assert bad_in == 0, "Inputs must be between 0 and 1"
            assert bad_tg == 0, "Targets must be between 0 and 1"
            return v
        self.check_range()
        return float(self._total)


_TEN = (BCEDiceLoss, TverskyLoss, logcoshTverskyLoss, MSELoss, MAELoss, HuberLoss, DistanceGradientLoss, WeightedDistanceGradientLoss,
        WeightedVectorFieldLoss)
