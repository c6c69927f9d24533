"""CPU-side checks of the 2-D multi-output workflow (no GPU): the torch fallback of every criterion of
``bio_image_unet_amd.multi_output_unet.losses`` against the reference's own float32 numbers (tests/golden/mo2d_losses.npz, written by
tests/golden/make_golden_mo2d_losses.py), ``MultiHeadLoss`` against the reference trainer's deep-supervision total, the constructor
contracts, and the tiling arithmetic of ``PredictMo2d``."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "mo2d_losses.npz"))
META = json.loads(bytes(Z["meta_json"]).decode())
CASES = {c["name"]: c for c in META["cases"]}


def _mod():
    import bio_image_unet_amd.multi_output_unet as M
    return M


@pytest.mark.parametrize("case", list(CASES))
def test_fallback_equals_reference_fp32(case):
    """loss to 1e-6 relative, gradient to 1e-6 of the largest gradient entry, against the reference classes in float32."""
    c = CASES[case]
    crit = getattr(_mod().losses, c["cls"])(**c["kwargs"])
    x = torch.from_numpy(Z[f"in.{c['set']}.x"]).clone().requires_grad_(c["grad"])
    t = torch.from_numpy(Z[f"in.{c['set']}.t"])
    loss = crit(x, t)
    want = float(Z[f"{case}.loss32"])
    assert abs(float(loss.detach()) - want) <= 1e-6 * abs(want), (float(loss.detach()), want)
    if c["grad"]:
        loss.backward()
        g = torch.from_numpy(Z[f"{case}.grad32"])
        assert float((x.grad - g).abs().max()) <= 1e-6 * float(g.abs().max())


def test_bce_clamp_value():
    """nn.BCELoss clamps both logs at -100: [0, 1, .5] against [1, 0, 1] is (100 + 100 + log 2) / 3."""
    crit = _mod().BCEDiceLoss(bce_weight=1, dice_weight=0)
    got = float(crit(torch.tensor([0.0, 1.0, 0.5]).view(1, 1, 1, 3), torch.tensor([1.0, 0.0, 1.0]).view(1, 1, 1, 3)))
    assert abs(got - 66.8977) < 1e-3
    assert abs(got - float(Z["bce_clamp.loss64"])) <= 1e-6 * got


def _ds_tensors(dtype=torch.float32):
    out = {k[len("ds.pred."):]: torch.from_numpy(Z[k]).to(dtype) for k in Z.files if k.startswith("ds.pred.")}
    tg = {k[len("ds.target."):]: torch.from_numpy(Z[k]).to(dtype) for k in Z.files if k.startswith("ds.target.")}
    return out, tg


def test_multi_head_loss_cpu_equals_reference_total():
    ds = META["ds"]
    mh = _mod().MultiHeadLoss(ds["heads"], deep_supervision=True, levels=ds["levels"])
    out, tg = _ds_tensors()
    total = mh(out, tg)
    want = float(Z["ds.total32"])
    assert abs(float(total) - want) <= 1e-6 * abs(want)
    assert abs(mh.item() - want) <= 1e-6 * abs(want)
    out64, tg64 = _ds_tensors(torch.float64)
    assert abs(float(mh(out64, tg64)) - float(Z["ds.total64"])) <= 1e-12 * abs(want)
    # three weights on levels 1-3, as the reference's validation pass uses them
    three = mh(out, tg, weights=[0.5, 0.75, 1.0])
    L = _mod().losses
    fns = {"seg": L.BCEDiceLoss(), "vec": L.WeightedVectorFieldLoss(), "dist": L.WeightedDistanceGradientLoss()}
    ref = sum(w * ds["heads"][n]["weight"] * fns[n](out[f"{n}_{l}"], tg[n]) for n in fns for l, w in enumerate([0.5, 0.75, 1.0], 1))
    assert abs(float(three) - float(ref)) <= 1e-6 * abs(float(ref))
    with pytest.raises(ValueError, match="levels not valid"):
        _mod().MultiHeadLoss(ds["heads"], deep_supervision=True, levels=5)(out, tg)


def test_constructor_signatures_and_loss_names():
    M = _mod()
    L = M.losses

    def args(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    assert args(L.BCEDiceLoss) == [("bce_weight", 0.5), ("dice_weight", 0.5)]
    assert args(L.TverskyLoss) == [("alpha", 0.5), ("beta", 0.5), ("smooth", 1)]
    assert args(L.logcoshTverskyLoss) == [("alpha", 0.5), ("beta", 0.5), ("smooth", 1)]
    assert args(L.HuberLoss) == [("delta", 1.0)]
    assert args(L.DistanceGradientLoss) == [("alpha", 1)]
    assert args(L.WeightedDistanceGradientLoss) == [("alpha", 1.0), ("beta", 0.5)]
    assert args(L.WeightedVectorFieldLoss) == [("beta", 0.5), ("magnitude_weight", 0.3)]
    assert callable(L.gradient_loss) and isinstance(L.MSELoss(), torch.nn.Module) and isinstance(L.MAELoss(), torch.nn.Module)
    get = M.Trainer._get_loss_function
    names = {"BCEDiceLoss": L.BCEDiceLoss, "DiceLoss": L.BCEDiceLoss, "TverskyLoss": L.TverskyLoss, "logcoshTverskyLoss": L.logcoshTverskyLoss,
             "MSELoss": L.MSELoss, "MAELoss": L.MAELoss, "HuberLoss": L.HuberLoss, "DistanceGradientLoss": L.DistanceGradientLoss,
             "WeightedDistanceGradientLoss": L.WeightedDistanceGradientLoss, "WeightedVectorFieldLoss": L.WeightedVectorFieldLoss}
    for n, cls in names.items():
        assert type(get(n)) is cls, n
    d = get("DiceLoss")
    assert (d.bce_weight, d.dice_weight) == (0, 1)
    with pytest.raises(ValueError, match='Loss "Focal" not defined!'):
        get("Focal")


def test_trainer_and_predict_are_exported():
    M = _mod()
    from bio_image_unet_amd import workflow
    assert M.Trainer is workflow.TrainerMo2d and M.Predict is workflow.PredictMo2d
    sig = inspect.signature(M.Trainer.__init__).parameters
    assert list(sig)[1:] == ["dataset", "num_epochs", "network", "levels", "batch_size", "lr", "in_channels", "output_heads", "n_filter",
                             "deep_supervision", "dilation", "val_split", "save_dir", "save_name", "save_iter", "load_weights", "device"]
    assert sig["network"].default is M.MultiOutputNestedUNet and sig["levels"].default == 4 and sig["lr"].default == 1e-4
    assert sig["n_filter"].default == 64 and sig["batch_size"].default == 4 and sig["deep_supervision"].default is False
    psig = inspect.signature(M.Predict.__init__).parameters
    assert list(psig)[1:6] == ["imgs", "model_params", "result_path", "network", "max_patch_size"]
    assert psig["max_patch_size"].default == (1024, 1024) and psig["clip_threshold"].default == (0., 99.98)


def test_predict_tiling_arithmetic():
    """Patch size, tile origins and weight planes of ``PredictMo2d`` against a numpy restatement of ``multi_output_unet/predict.py:153-177,
    259-269``, for an extent that needs 2 x 3 tiles and gets 3 x 4 with ``add_tile=1``.  Unpinned by the reference itself: its predictor
    imports ``tifffile``, which is not installed (as for the other families' predictors)."""
    P = _mod().Predict
    shape, max_patch, add = (3, 90, 150), (60, 60), 1
    (ph, pw), n_x, n_y, (H, W), xs, ys = P.geometry(shape, max_patch, add)
    assert (ph, pw) == (64, 64)                      # min(extent, max) rounded up to a multiple of 16
    assert (n_x, n_y) == (2 + 1, 3 + 1) and (H, W) == (90, 150)
    assert xs.dtype == np.uint16 and list(xs) == [int(v) for v in np.linspace(0, 90 - 64, 3)] == [0, 13, 26]
    assert list(ys) == [int(v) for v in np.linspace(0, 150 - 64, 4)] == [0, 28, 57, 86]
    # an image smaller than the rounded patch is padded up to it
    (ph2, pw2), n_x2, n_y2, (H2, W2), xs2, ys2 = P.geometry((1, 40, 100), (1024, 1024), 0)
    assert (ph2, pw2, n_x2, n_y2, H2, W2) == (48, 112, 1, 1, 48, 112) and list(xs2) == [0] and list(ys2) == [0]
    for j in range(n_x):
        for k in range(n_y):
            want = np.ones((ph, pw), dtype="float32")
            if j > 0:
                want[:20, :] = 0
            if j < n_x - 1:
                want[-20:, :] = 0
            if k > 0:
                want[:, :20] = 0
            if k < n_y - 1:
                want[:, -20:] = 0
            assert np.array_equal(P.weight_plane(j, k, n_x, n_y, (ph, pw)), want), (j, k)
    # normalisation is to [0, 1]
    g = np.random.default_rng(0)
    imgs = g.random((2, 16, 16)).astype("float32") * 1000
    out = P._preprocess(imgs.copy(), "single", (0., 99.98))
    assert out.min() == 0.0 and out.max() == 1.0
    with pytest.raises(ValueError, match="normalization_mode"):
        P._preprocess(imgs.copy(), "each", (0., 99.98))
