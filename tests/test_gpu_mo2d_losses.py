"""The 2-D multi-output workflow on the GPU: the fused criteria (``biu_mo2d_loss_*``) through the C ABI and through the classes against the
reference's float64 numbers (tests/golden/mo2d_losses.npz), ``MultiHeadLoss``'s launch plan, and ``TrainerMo2d`` / ``PredictMo2d``.

Bound of every value / gradient comparison: ``max(16 x the reference's own float32-vs-float64 deviation, 2e-6)`` -- relative to the value
for a loss, to the largest gradient entry for a gradient.  16 allows for a different summation order and the device's log / cosh; the
floor is 16 fp32 ulps for cases where the reference lands exactly."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bio_image_unet_amd as B  # noqa: E402
import bio_image_unet_amd.multi_output_unet as MO  # noqa: E402
from bio_image_unet_amd._lib import BiuError, biu_mo2d_term  # noqa: E402
from bio_image_unet_amd.multi_output_unet import losses as L  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402
from tests import mo2d_oracle as M  # noqa: E402
from tests.gpu_util import lib, ptr, stream  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "mo2d_losses.npz"))
META = json.loads(bytes(Z["meta_json"]).decode())
CASES = {c["name"]: c for c in META["cases"]}
FLOOR = 2e-6


def bound(dev):
    return max(16.0 * float(dev), FLOOR)


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def abi_total(crit, preds, target, weights, g=1.0):
    """One head through the five entry points of include/biu.h: (total, per-term losses, out-of-range counts, gradients)."""
    n, c, h, w = target.shape
    nb = lib.biu_mo2d_loss_blocks(target.numel())
    p, (ea, eb) = crit._params(), crit._elem()
    terms = (biu_mo2d_term * len(preds))(*[biu_mo2d_term(crit.kind, nb, l * nb * 8, target.numel(), n * h * w, p[0], p[1], p[2], wt)
                                         for l, wt in enumerate(weights)])
    tdev = torch.frombuffer(bytearray(bytes(terms)), dtype=torch.uint8).cuda()
    ws = torch.full((len(preds) * nb * 8,), float("nan"), device="cuda")
    saved = torch.full((8 + 8 * len(preds),), float("nan"), device="cuda")
    rc = lib.biu_mo2d_loss_fwd(crit.kind, ea, eb, _ptrs(preds), len(preds), ptr(target), n, c, h, w, ptr(ws), stream())
    if rc != 0:
        grads = [torch.empty_like(q) for q in preds]
        assert lib.biu_mo2d_loss_bwd(crit.kind, ea, eb, _ptrs(preds), len(preds), ptr(target), n, c, h, w, ptr(ws), _ptrs(grads), stream()) == rc
        return rc
    assert lib.biu_mo2d_loss_finish(ptr(tdev), len(preds), ptr(ws), ptr(saved), stream()) == 0
    gd = torch.tensor([g], device="cuda")
    coef = torch.empty(4 * len(preds), device="cuda")
    assert lib.biu_mo2d_loss_coef(ptr(tdev), len(preds), ptr(gd), ptr(saved), ptr(coef), stream()) == 0
    grads = [torch.full_like(q, float("nan")) for q in preds]
    assert lib.biu_mo2d_loss_bwd(crit.kind, ea, eb, _ptrs(preds), len(preds), ptr(target), n, c, h, w, ptr(coef), _ptrs(grads), stream()) == 0
    torch.cuda.synchronize()
    s = saved.cpu()
    return float(s[0]), [float(s[8 + 8 * i]) for i in range(len(preds))], (float(s[1]), float(s[2])), [q.cpu() for q in grads]


def _case(case):
    c = CASES[case]
    crit = getattr(L, c["cls"])(**c["kwargs"])
    return c, crit, torch.from_numpy(Z[f"in.{c['set']}.x"]).cuda(), torch.from_numpy(Z[f"in.{c['set']}.t"]).cuda()


def _check(case, c, loss, grad):
    want = float(Z[f"{case}.loss64"])
    err = abs(loss - want) / abs(want)
    print(f"{case}: loss rel err {err:.3e} (bound {bound(Z[f'{case}.dev_loss']):.3e})", end="")
    assert err <= bound(Z[f"{case}.dev_loss"]), (case, loss, want, err)
    if c["grad"]:
        g64 = torch.from_numpy(Z[f"{case}.grad64"])
        gerr = float((grad.double() - g64).abs().max()) / float(g64.abs().max())
        print(f"  grad rel err {gerr:.3e} (bound {bound(Z[f'{case}.dev_grad']):.3e})")
        assert gerr <= bound(Z[f"{case}.dev_grad"]), (case, gerr)


@pytest.mark.parametrize("case", list(CASES))
def test_c_abi_vs_reference_fp64(case):
    """Every kind through biu_mo2d_loss_fwd / _finish / _coef / _bwd: value and gradient against the reference in float64; two levels of
    one launch (the same prediction twice, weights 1 and 0.5) give the same per-term value and gradients in proportion."""
    c, crit, x, t = _case(case)
    total, per, oob, grads = abi_total(crit, [x, x.clone()], t, [1.0, 0.5])
    assert oob == (0.0, 0.0)
    assert per[0] == per[1] and abs(total - 1.5 * per[0]) <= 1e-6 * abs(total)
    _check(case, c, per[0], grads[0])
    assert torch.equal(grads[1], 0.5 * grads[0]) or float((grads[1] - 0.5 * grads[0]).abs().max()) <= 1e-7 * float(grads[0].abs().max())


@pytest.mark.parametrize("case", list(CASES))
def test_classes_vs_reference_fp64(case):
    c, crit, x, t = _case(case)
    x.requires_grad_(c["grad"])
    loss = crit(x, t)
    if c["grad"]:
        (3.0 * loss).backward()           # an upstream factor reaches the coefficients through the device scalar
    _check(case, c, float(loss.detach()), x.grad.cpu() / 3.0 if c["grad"] else None)


CONFIGS = [("BCEDiceLoss", dict(bce_weight=0.3, dice_weight=0.7), "prob"), ("BCEDiceLoss", dict(bce_weight=0, dice_weight=1), "prob"),
           ("TverskyLoss", dict(alpha=0.3, beta=0.7, smooth=0.5), "prob"), ("logcoshTverskyLoss", dict(alpha=0.6, beta=0.4, smooth=2), "prob"),
           ("MSELoss", {}, "reg"), ("MAELoss", {}, "reg"), ("HuberLoss", dict(delta=0.5), "reg"), ("DistanceGradientLoss", dict(alpha=0.7), "reg"),
           ("WeightedDistanceGradientLoss", dict(alpha=0.6, beta=0.7), "reg"), ("WeightedVectorFieldLoss", dict(beta=0.7, magnitude_weight=0.45), "vec")]


def _draw(kind, shape, g):
    if kind == "prob":
        return torch.rand(shape, generator=g) * 0.98 + 0.01, (torch.rand(shape, generator=g) < 0.4).float()
    if kind == "reg":
        return torch.randn(shape, generator=g) * 0.6, (torch.rand(shape, generator=g) < 0.6).float() * torch.rand(shape, generator=g) * 1.5
    n, _, h, w = shape
    return torch.randn(shape, generator=g) * 0.7, torch.randn(shape, generator=g) * (torch.rand((n, 1, h, w), generator=g) < 0.6).float()


@pytest.mark.parametrize("shape", [(4, 2, 256, 256), (3, 2, 37, 53)])
@pytest.mark.parametrize("cfg", CONFIGS, ids=[f"{c[0]}{i}" for i, c in enumerate(CONFIGS)])
def test_large_random_vs_fallback_fp64(cfg, shape):
    """A larger case and one whose H, W are no multiples of 4 (scalar kernels) against the torch composition evaluated in float64 on the
    CPU; the bound takes the composition's own float32 deviation on the same inputs."""
    cls, kw, kind = cfg
    g = torch.Generator().manual_seed(sum(shape) + len(cls))
    x, t = _draw(kind, shape, g)
    crit = getattr(L, cls)(**kw)

    def cpu(dt):
        xi = x.to(dt).clone().requires_grad_(True)
        loss = crit(xi, t.to(dt))
        loss.backward()
        return float(loss.detach()), xi.grad
    l64, g64 = cpu(torch.float64)
    l32, g32 = cpu(torch.float32)
    xd = x.cuda().requires_grad_(True)
    loss = crit(xd, t.cuda())
    loss.backward()
    err = abs(float(loss.detach()) - l64) / abs(l64)
    gerr = float((xd.grad.cpu().double() - g64).abs().max()) / float(g64.abs().max())
    bl, bg = bound(abs(l32 - l64) / abs(l64)), bound(float((g32.double() - g64).abs().max()) / float(g64.abs().max()))
    print(f"{cls} {shape}: loss {err:.3e} (bound {bl:.3e})  grad {gerr:.3e} (bound {bg:.3e})")
    assert err <= bl and gerr <= bg


def test_two_calls_are_bit_equal():
    g = torch.Generator().manual_seed(7)
    for cls, kw, kind in CONFIGS:
        x, t = _draw(kind, (2, 2, 64, 96), g)
        runs = []
        for _ in range(2):
            xd = x.cuda().requires_grad_(True)
            loss = getattr(L, cls)(**kw)(xd, t.cuda())
            loss.backward()
            runs.append((loss.detach().cpu(), xd.grad.cpu()))
        assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), cls
        assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), cls


@pytest.mark.parametrize("cls", ["DistanceGradientLoss", "WeightedDistanceGradientLoss"])
def test_gradient_kinds_refuse_extent_one(cls):
    crit = getattr(L, cls)()
    x, t = torch.rand(2, 1, 1, 16, device="cuda"), torch.rand(2, 1, 1, 16, device="cuda")
    assert abi_total(crit, [x], t, [1.0]) == -1                 # BIU_ERR_SHAPE, forward and backward
    assert b"torch.gradient" in lib.biu_last_error()
    with pytest.raises(BiuError):
        crit(x, t)
    xw, tw = torch.rand(2, 1, 16, 1, device="cuda"), torch.rand(2, 1, 16, 1, device="cuda")
    assert abi_total(crit, [xw], tw, [1.0]) == -1
    # the vector-field kind takes two channels
    assert abi_total(L.WeightedVectorFieldLoss(), [torch.rand(1, 3, 4, 4, device="cuda")], torch.rand(1, 3, 4, 4, device="cuda"), [1.0]) == -1


def test_bce_dice_out_of_range_raises():
    crit = L.BCEDiceLoss()
    x, t = torch.rand(2, 1, 16, 16, device="cuda"), (torch.rand(2, 1, 16, 16, device="cuda") > 0.5).float()
    crit(x, t)
    bad = x.clone()
    bad[1, 0, 3, 5] = 1.5
    with pytest.raises(AssertionError, match="Inputs must be between 0 and 1"):
        crit(bad, t)
    tb = t.clone()
    tb[0, 0, 0, 0] = -0.25
    with pytest.raises(AssertionError, match="Targets must be between 0 and 1"):
        crit(x, tb)
    nan = x.clone()
    nan[0, 0, 1, 1] = float("nan")
    with pytest.raises(AssertionError, match="Inputs"):
        crit(nan, t)
    # deferred in MultiHeadLoss: no error until the total is read
    mh = L.MultiHeadLoss({"a": {"channels": 1, "loss": "BCEDiceLoss"}})
    total = mh({"a": bad}, {"a": t})
    assert total.is_cuda
    with pytest.raises(AssertionError, match="Inputs must be between 0 and 1"):
        mh.item()


def test_deep_supervision_total_vs_reference_fp64():
    ds = META["ds"]
    out = {k[len("ds.pred."):]: torch.from_numpy(Z[k]).cuda().requires_grad_(True) for k in Z.files if k.startswith("ds.pred.")}
    tg = {k[len("ds.target."):]: torch.from_numpy(Z[k]).cuda() for k in Z.files if k.startswith("ds.target.")}
    mh = L.MultiHeadLoss(ds["heads"], deep_supervision=True, levels=4)
    before = L.launches
    total = mh(out, tg)
    total.backward()
    assert L.launches - before == 2 * len(ds["heads"]) + 2          # a forward and a backward launch per head, finish, coef
    want = float(Z["ds.total64"])
    err = abs(float(total.detach()) - want) / abs(want)
    print(f"ds total rel err {err:.3e} (bound {bound(Z['ds.dev']):.3e})")
    assert err <= bound(Z["ds.dev"])
    assert abs(mh.item() - want) <= bound(Z["ds.dev"]) * abs(want)
    # gradients against the torch composition in float64 on the CPU
    o64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in out.items()}
    L.MultiHeadLoss(ds["heads"], deep_supervision=True, levels=4)(o64, {k: v.cpu().double() for k, v in tg.items()}).backward()
    for k in out:
        gerr = float((out[k].grad.cpu().double() - o64[k].grad).abs().max()) / float(o64[k].grad.abs().max())
        assert gerr <= FLOOR, (k, gerr)


HEADS2 = {"a": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss"},
          "b": {"channels": 2, "activation": "relu", "weight": 0.5, "loss": "WeightedVectorFieldLoss"}}


def test_multi_head_loss_on_network_outputs_equals_per_class_sum():
    """``nested_ds_f16`` of tests/test_gpu_mo2d.py (F = 16, deep supervision, 2 x 1 x 64 x 64): the fused total and its gradients w.r.t.
    every level's output equal the weighted sum of per-class calls, in 2 * heads + 2 launches; a head with a foreign criterion is added
    in torch."""
    torch.manual_seed(0)
    m = B.MultiOutputNestedUNet(in_channels=1, output_heads=HEADS2, n_filter=16, deep_supervision=True, dilation=(1, 2, 1, 1, 2)).cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 1, 64, 64, generator=g).cuda()
    tg = {"a": (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda(),
          "b": (torch.randn(2, 2, 64, 64, generator=g) * (torch.rand(2, 1, 64, 64, generator=g) < 0.6).float()).cuda()}
    with torch.no_grad():
        out = m(x)
    keys = [f"{n}_{l}" for n in HEADS2 for l in range(1, 5)]
    leaves = {k: out[k].detach().clone().requires_grad_(True) for k in keys}
    mh = L.MultiHeadLoss(HEADS2, deep_supervision=True, levels=4)
    before = L.launches
    total = mh(leaves, tg)
    total.backward()
    assert L.launches - before == 2 * 2 + 2
    fused = {k: v.grad.clone() for k, v in leaves.items()}
    ref_leaves = {k: out[k].detach().clone().requires_grad_(True) for k in keys}
    ref = 0
    for n, cfg in HEADS2.items():
        for l, sw in enumerate([0.5, 0.75, 0.875, 1.0], 1):
            ref = ref + sw * cfg.get("weight", 1.0) * mh.loss_functions[n](ref_leaves[f"{n}_{l}"], tg[n])
    ref.backward()
    assert abs(float(total) - float(ref)) <= FLOOR * abs(float(ref))
    for k in keys:
        assert float((fused[k] - ref_leaves[k].grad).abs().max()) <= FLOOR * float(ref_leaves[k].grad.abs().max()), k
    # a criterion that is not one of the ten goes through torch and is added
    mixed = L.MultiHeadLoss(HEADS2, deep_supervision=True, levels=4, loss_functions={"a": mh.loss_functions["a"], "b": torch.nn.L1Loss()})
    before = L.launches
    t2 = mixed({k: v.detach() for k, v in leaves.items()}, tg)
    assert L.launches - before == 2
    want = sum(sw * (mh.loss_functions["a"](leaves[f"a_{l}"].detach(), tg["a"]) + 0.5 * torch.nn.functional.l1_loss(leaves[f"b_{l}"].detach(), tg["b"]))
               for l, sw in enumerate([0.5, 0.75, 0.875, 1.0], 1))
    assert abs(float(t2) - float(want)) <= 1e-5 * abs(float(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# Trainer / Predict
# ---------------------------------------------------------------------------------------------------------------------------------
HEADS3 = {"a": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
          "b": {"channels": 2, "activation": None, "loss": "WeightedVectorFieldLoss", "weight": 0.5},
          "c": {"channels": 1, "activation": "relu", "loss": "WeightedDistanceGradientLoss", "weight": 0.25}}


class Items(torch.utils.data.Dataset):
    """The reference data set's item contract: 'image' (H, W) and one target per head, (C, H, W) or (H, W)."""
    aug_factor, clip_threshold, gauss_noise_lims, shot_noise_lims, brightness_contrast, random_rotate = 1, (0., 99.98), None, None, None, False

    def __init__(self, n, dim, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.dim_out = dim
        self.items = []
        for _ in range(n):
            self.items.append({"image": torch.rand(dim, generator=g),
                               "a": (torch.rand((1,) + dim, generator=g) > 0.5).float(),
                               "b": torch.randn((2,) + dim, generator=g) * (torch.rand((1,) + dim, generator=g) < 0.6).float(),
                               "c": (torch.rand(dim, generator=g) < 0.6).float() * torch.rand(dim, generator=g)})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _dead(k):
    return k.endswith((".conv1.bias", ".conv2.bias", ".0.bias"))


def test_trainer_step_vs_oracle(tmp_path):
    """One training step of ``TrainerMo2d`` on ``MultiOutputNestedUNet(n_filter=16, deep_supervision=True)`` with mixed criteria against the
    fp64 oracle (tests/mo2d_oracle.py forward + the torch composition of the criteria in float64 + ``O.adam_step(..., clip=1.0)``) on the
    engine's own branch decisions, with the bounds of tests/test_gpu_mo2d.py::test_trainer_step_clip_adam."""
    from tests import insitu
    torch.manual_seed(5)
    tr = MO.Trainer(Items(10, (32, 32)), 1, levels=4, batch_size=2, lr=1e-3, output_heads=HEADS3, n_filter=16, deep_supervision=True,
                    save_dir=str(tmp_path), device="cuda")
    assert isinstance(tr.model, B.MultiOutputNestedUNet) and tr.model.deep_supervision
    sd = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    batch = next(iter(tr.train_loader))
    loss = tr._total_loss(batch, validating=False)
    tr.optimizer.zero_grad()
    loss.backward()
    q = insitu.extract_decisions(list(tr.model._engines.values())[-1][-1])
    norm = float(tr.optimizer.clip_grad_norm_(1.0))
    tr.optimizer.step()
    got_loss = tr.criterion.item()
    torch.cuda.synchronize()
    x = batch["image"].unsqueeze(1)
    tg = {k: (batch[k].unsqueeze(1) if batch[k].dim() == 3 else batch[k]).double() for k in HEADS3}
    osd = O.clone_state({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, requires_grad=True)
    with O.forced_decisions(q):
        out = M.nested_forward(osd, x.double(), HEADS3, levels=4, deep_supervision=True, training=True)
        o_loss = L.MultiHeadLoss(HEADS3, deep_supervision=True, levels=4)(out, tg)
        o_grads = O.grads_of(o_loss, osd)
    upd, o_norm = O.adam_step({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, o_grads, lr=1e-3, clip=1.0)
    assert abs(got_loss - float(o_loss)) < 1e-3 * max(1.0, abs(float(o_loss))), (got_loss, float(o_loss))
    assert abs(norm - float(o_norm)) < 1e-3 * float(o_norm)
    msd = tr.model.state_dict()
    for k, want in upd.items():
        if _dead(k):
            continue
        live = o_grads[k].abs() > 1e-3 * float(o_grads[k].abs().max())
        d = (msd[k].cpu().double() - sd[k].double()) - (want - sd[k].double())
        assert float(d[live].abs().max()) < 1e-4, k


def test_trainer_validation_quirks(tmp_path):
    """Validation re-applies the head activation (softmax included) to the activated outputs, weights levels 1-3 with [0.5, 0.75, 1.0] on
    the four-level network, and leaves the model in train mode."""
    torch.manual_seed(2)
    tr = MO.Trainer(Items(10, (32, 32)), 1, levels=4, batch_size=2, output_heads=HEADS3, n_filter=16, deep_supervision=True,
                    save_dir=str(tmp_path), device="cuda")
    tr.activations["b"] = "softmax"
    batch = next(iter(tr.val_loader))
    with torch.no_grad():
        got = float(tr._total_loss(batch, validating=True))
        pred = tr.model(batch["image"].unsqueeze(1).cuda())        # train mode: the same batch statistics, the same outputs
    assert tr.model.training
    act = {"a": torch.sigmoid, "b": lambda t: torch.softmax(t, dim=1), "c": torch.relu}
    want = 0
    for n, cfg in HEADS3.items():
        t = batch[n].double()
        t = t.unsqueeze(1) if t.dim() == 3 else t
        for l, sw in enumerate([0.5, 0.75, 1.0], 1):
            want = want + sw * cfg["weight"] * tr.loss_functions[n](act[n](pred[f"{n}_{l}"].cpu().double()), t)
    assert abs(got - float(want)) <= 1e-5 * abs(float(want)), (got, float(want))
    with pytest.raises(ValueError, match="levels not valid"):
        bad = MO.Trainer(Items(4, (32, 32)), 1, levels=5, batch_size=2, output_heads=HEADS3, n_filter=16, deep_supervision=True,
                         save_dir=str(tmp_path), device="cuda")
        bad._total_loss(next(iter(bad.train_loader)), validating=False)


def test_trainer_start_checkpoint_and_predict(tmp_path):
    """``start()`` for two epochs on a ten-item in-memory data set writes a checkpoint with the reference's keys; ``PredictMo2d`` loads it.
    The stitched result of a 3-image stack tiled 2 x 2 with overlap equals the numpy restatement of the reference's ``__stitch``
    (multi_output_unet/predict.py:234-285) fed with the engine's own eval outputs rounded to float16, including pixels that only the
    mean fill reaches (the columns between the two tiles' safe margins)."""
    torch.manual_seed(3)
    tr = MO.Trainer(Items(10, (32, 32)), 2, levels=4, batch_size=2, lr=1e-3, output_heads=HEADS3, n_filter=16, deep_supervision=True,
                    save_dir=str(tmp_path), save_name="mo2d.pt", device="cuda")
    tr.start()
    path = os.path.join(str(tmp_path), "mo2d.pt")
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert set(state) == {"epoch", "epoch_start", "best_loss", "state_dict", "optimizer", "lr", "n_filter", "deep_supervision", "dilation",
                          "batch_size", "augmentation", "clip_threshold", "gauss_noise_lims", "shot_noise_lims", "brightness_contrast",
                          "random_rotate", "in_channels", "output_heads"}
    assert state["deep_supervision"] is True and state["n_filter"] == 16 and state["output_heads"] == HEADS3
    assert float(state["best_loss"]) < float("inf")

    g = np.random.default_rng(0)
    imgs = (g.random((3, 50, 80)) * 900 + 17).astype("float32")
    pr = MO.Predict(imgs.copy(), path, max_patch_size=(48, 48), batch_size=4, device="cuda")
    assert pr.patch_size == (48, 48) and (pr.N_x, pr.N_y) == (2, 2) and list(pr.X_start) == [0, 2] and list(pr.Y_start) == [0, 32]
    assert not pr.model.training and pr.model.train_mode is False
    # numpy restatement: normalise, cut, predict with the predictor's own model in the same batches, stitch
    norm = imgs.copy()
    for i, img in enumerate(norm):
        img = np.clip(img, a_min=np.nanpercentile(img, 0.), a_max=np.percentile(img, 99.98))
        img = img - np.min(img)
        norm[i] = img / np.max(img)
    patches = np.stack([norm[n, xs:xs + 48, ys:ys + 48] for n in range(3) for xs in (0, 2) for ys in (0, 32)])
    res = {k: np.zeros((12, HEADS3[k]["channels"], 48, 48), dtype="float16") for k in HEADS3}
    with torch.no_grad():
        for b in range(0, 12, 4):
            out = pr.model(torch.from_numpy(patches[b:b + 4]).cuda().view(-1, 1, 48, 48))
            for k in HEADS3:
                res[k][b:b + 4] = out[k].cpu().numpy()
    saw_fill = False
    for k in HEADS3:
        c = HEADS3[k]["channels"]
        acc = np.zeros((3, c, 50, 80), dtype="float32")
        wsum = np.zeros_like(acc)
        for n in range(3):
            tiles = res[k][n * 4:(n + 1) * 4].reshape(2, 2, c, 48, 48)
            for j, xs in enumerate((0, 2)):
                for kk, ys in enumerate((0, 32)):
                    patch = tiles[j, kk]
                    w = np.ones_like(patch)
                    if j > 0:
                        w[..., :20, :] = 0
                    if j < 1:
                        w[..., -20:, :] = 0
                    if kk > 0:
                        w[..., :20] = 0
                    if kk < 1:
                        w[..., -20:] = 0
                    acc[n, :, xs:xs + 48, ys:ys + 48] += patch * w
                    wsum[n, :, xs:xs + 48, ys:ys + 48] += w
        np.divide(acc, wsum, out=acc, where=wsum > 0)
        acc[wsum == 0] = res[k].mean()
        saw_fill = saw_fill or bool((wsum == 0).any())
        want = np.squeeze(acc)
        got = pr.result[k]
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (k, np.abs(got - want).max())
    assert saw_fill
