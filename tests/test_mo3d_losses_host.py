"""CPU-side checks of the 3-D multi-output criteria (no GPU): the torch fallback of every class of
``bio_image_unet_amd.multi_output_unet3d.losses`` against the reference's numbers (tests/golden/mo3d_losses.npz, written by
tests/golden/make_golden_mo3d_losses.py) at 1e-5, the bound tests/test_oracle_golden.py uses; the constructor contracts, the names of
``get_loss_function`` and the ``[N, D, H, W]`` target view of ``MultiHeadLoss``."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "mo3d_losses.npz"))
META = json.loads(bytes(Z["meta_json"]).decode())
CASES = {c["name"]: c for c in META["cases"]}
TOL = 1e-5

from bio_image_unet_amd.multi_output_unet3d import losses as L  # noqa: E402


def test_fixture_holds_the_cases_the_trainer_constructs():
    want = {("BCEDiceLoss", (1, 1)), ("BCEDiceLoss", (0, 1)), ("TverskyLoss", ()), ("logcoshTverskyLoss", ()), ("BCEDiceTemporalLoss", ()),
            ("BCEDiceLoss", (0.3, 0.7)), ("TverskyLoss", (0.3, 0.7, 0.5)), ("logcoshTverskyLoss", (0.6, 0.4, 2))}
    for size, shape in (("odd", (2, 2, 5, 6, 7)), ("pair", (2, 1, 2, 8, 8))):
        assert {(c["cls"], tuple(c["args"])) for c in CASES.values() if c["set"] == size} == want
        x = Z[f"in.{size}.x"]
        assert x.shape == shape and x.dtype == np.float32
        assert float(np.abs(x[:, :, 1:] - x[:, :, :-1]).min()) >= 1e-4          # the temporal sign is the same in float32 and float64
        assert set(np.unique(Z[f"in.{size}.t"])) == {0.0, 1.0}


@pytest.mark.parametrize("case", list(CASES))
def test_fallback_equals_reference(case):
    c = CASES[case]
    crit = getattr(L, c["cls"])(*c["args"])
    x = torch.from_numpy(Z[f"in.{c['set']}.x"]).clone().requires_grad_(True)
    t = torch.from_numpy(Z[f"in.{c['set']}.t"])
    loss = crit(x, t)
    loss.backward()
    want, g = float(Z[f"{case}.loss64"]), torch.from_numpy(Z[f"{case}.grad64"])
    assert abs(float(loss.detach()) - want) <= TOL * abs(want), (float(loss.detach()), want)
    assert float((x.grad.double() - g).abs().max()) <= TOL * float(g.abs().max())
    # and in float64 the composition is the reference's arithmetic
    x64 = torch.from_numpy(Z[f"in.{c['set']}.x"]).double().requires_grad_(True)
    l64 = crit(x64, t.double())
    l64.backward()
    assert abs(float(l64.detach()) - want) <= 1e-12 * abs(want)
    assert float((x64.grad - g).abs().max()) <= 1e-12 * float(g.abs().max())


def test_constructor_signatures():
    def args(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    empty = inspect.Parameter.empty
    assert args(L.BCEDiceLoss) == [("alpha", empty), ("beta", empty)]
    assert args(L.DiceLoss) == []
    assert args(L.TverskyLoss) == [("alpha", 0.5), ("beta", 0.5), ("smooth", 1)]
    assert args(L.logcoshTverskyLoss) == [("alpha", 0.5), ("beta", 0.5), ("smooth", 1)]
    assert args(L.BCEDiceTemporalLoss) == [("loss_params", (1.0, 0.1))]
    for cls in (L.BCEDiceLoss, L.TverskyLoss, L.logcoshTverskyLoss, L.BCEDiceTemporalLoss):
        assert list(inspect.signature(cls.forward).parameters)[1:] == ["logits", "targets"]
    d = L.DiceLoss()
    assert isinstance(d, L.BCEDiceLoss) and (d.alpha, d.beta) == (0, 1)
    sig = inspect.signature(L.MultiHeadLoss.__init__).parameters
    assert list(sig)[1:] == ["output_heads", "loss_functions"] and sig["loss_functions"].default is None
    fsig = inspect.signature(L.MultiHeadLoss.forward).parameters
    assert list(fsig)[1:] == ["pred", "targets", "pre_activations"] and fsig["pre_activations"].default is None
    assert isinstance(L.launches, int)


def test_get_loss_function_names_and_error_text():
    import bio_image_unet_amd.multi_output_unet3d as M
    assert M.losses is L and M.MultiHeadLoss is L.MultiHeadLoss and M.BCEDiceTemporalLoss is L.BCEDiceTemporalLoss
    names = {"BCEDiceLoss": (L.BCEDiceLoss, (1, 1)), "DiceLoss": (L.BCEDiceLoss, (0, 1)), "TverskyLoss": (L.TverskyLoss, None),
             "logcoshTverskyLoss": (L.logcoshTverskyLoss, None), "BCEDiceTemporalLoss": (L.BCEDiceTemporalLoss, None)}
    assert set(L.LOSS_TABLE) == set(names)
    for get in (L.get_loss_function, M.Trainer._get_loss_function):
        for n, (cls, ab) in names.items():
            crit = get(n)
            assert type(crit) is cls, n
            if ab is not None:
                assert (crit.alpha, crit.beta) == ab
        t = get("BCEDiceTemporalLoss")
        assert tuple(t.loss_params) == (1.0, 0.1)
        with pytest.raises(ValueError, match='Loss "Focal" not defined!'):
            get("Focal")


def _f(v):
    return float(v.detach())


HEADS = {"a": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "b": {"channels": 1, "activation": "tanh", "loss": "logcoshTverskyLoss", "weight": 0.5},
         "c": {"channels": 1, "activation": "relu", "loss": "BCEDiceTemporalLoss", "weight": 2.0}}


def test_multi_head_loss_cpu_target_view_and_pre_activations():
    """On CPU tensors every head goes through torch: the total is the weighted sum, a ``[N, D, H, W]`` target is viewed as
    ``[N, 1, D, H, W]``, and ``pre_activations`` activates the prediction before its criterion (softmax over the channels)."""
    g = torch.Generator().manual_seed(0)
    pred = {k: (torch.randn(2, 1, 3, 4, 5, generator=g) * 2).requires_grad_(True) for k in HEADS}
    tg4 = {k: (torch.rand(2, 3, 4, 5, generator=g) < 0.4).float() for k in HEADS}
    mh = L.MultiHeadLoss(HEADS)
    before = L.launches
    total = mh(pred, tg4)
    want = sum(cfg["weight"] * mh.loss_functions[k](pred[k], tg4[k].unsqueeze(1)) for k, cfg in HEADS.items())
    assert abs(_f(total) - _f(want)) <= 1e-6 * abs(_f(want))
    assert _f(total) == _f(mh(pred, {k: v.unsqueeze(1) for k, v in tg4.items()}))
    total.backward()
    assert all(p.grad is not None and p.grad.shape == p.shape for p in pred.values())
    acts = {"a": "sigmoid", "b": "softmax", "c": None}
    fn = {"a": torch.sigmoid, "b": lambda t: torch.softmax(t, dim=1), "c": lambda t: t}
    got = mh(pred, tg4, pre_activations=acts)
    want = sum(cfg["weight"] * mh.loss_functions[k](fn[k](pred[k]), tg4[k].unsqueeze(1)) for k, cfg in HEADS.items())
    assert abs(_f(got) - _f(want)) <= 1e-6 * abs(_f(want))
    assert L.launches == before                # nothing fused on the CPU
    # a foreign criterion is added through torch
    mixed = L.MultiHeadLoss(HEADS, loss_functions={**mh.loss_functions, "b": torch.nn.L1Loss()})
    want = (mh.loss_functions["a"](pred["a"], tg4["a"].unsqueeze(1)) + 0.5 * torch.nn.functional.l1_loss(pred["b"], tg4["b"].unsqueeze(1))
            + 2.0 * mh.loss_functions["c"](pred["c"], tg4["c"].unsqueeze(1)))
    assert abs(_f(mixed(pred, tg4)) - _f(want)) <= 1e-6 * abs(_f(want))


def test_temporal_single_plane_is_nan_on_the_cpu():
    x, t = torch.randn(2, 1, 1, 4, 4), (torch.rand(2, 1, 1, 4, 4) < 0.4).float()
    assert torch.isnan(L.BCEDiceTemporalLoss()(x, t))
    assert torch.isfinite(L.BCEDiceLoss(1, 1)(x, t))
