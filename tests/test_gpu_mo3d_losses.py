"""The fused criteria of the 3-D multi-output family on the GPU (``biu_mo3d_loss_*``): through the C ABI and through the classes against
the reference's float64 numbers (tests/golden/mo3d_losses.npz), ``MultiHeadLoss``'s launch plan, and one ``TrainerMo3d`` step.

Bound of every value / gradient comparison, as in tests/test_gpu_mo2d_losses.py: ``max(16 x the reference's own float32-vs-float64
deviation, 2e-6)`` -- relative to the value for a loss, to the largest gradient entry for a gradient.  16 allows for a different summation
order and the device's exp / log / cosh; the floor is 16 fp32 ulps for cases where the reference lands exactly.  Where the reference is
the torch composition of the module evaluated in float64 on the CPU, the deviation is that composition's own in float32 on the same
inputs.  Random logits are ``randn * 2`` and no z-neighbour pair is closer than 1e-4, so the sign of the temporal gradient is the same in
float32 and float64 (``_draw`` moves the seed on until that holds)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bio_image_unet_amd.multi_output_unet3d as MO  # noqa: E402
from bio_image_unet_amd._lib import BiuError, biu_mo3d_term  # noqa: E402
from bio_image_unet_amd.multi_output_unet3d import losses as L  # noqa: E402
from tests.gpu_util import lib, ptr, stream  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "mo3d_losses.npz"))
META = json.loads(bytes(Z["meta_json"]).decode())
CASES = {c["name"]: c for c in META["cases"]}
FLOOR = 2e-6
HDR, SLOTS = 32, 8


def bound(dev):
    return max(16.0 * float(dev), FLOOR)


def abi_head(crit, x, t, pre_act=0, weight=1.0, g=1.0, backward=True):
    """One head through the five entry points of include/biu.h: (total, the head's value, gradient or None)."""
    n, c, d, h, w = x.shape
    rows = lib.biu_mo3d_loss_blocks(x.numel())
    p = crit._params()
    term = (biu_mo3d_term * 1)(biu_mo3d_term(crit.kind, rows, 0, n, x.numel() // n, n * c * (d - 1) * h * w, p[0], p[1], p[2], weight))
    tdev = torch.frombuffer(bytearray(bytes(term)), dtype=torch.uint8).cuda()
    ws = torch.full((n * rows * SLOTS,), float("nan"), device="cuda")
    saved = torch.full((HDR + SLOTS * n,), float("nan"), device="cuda")
    assert lib.biu_mo3d_loss_fwd(crit.kind, pre_act, ptr(x), ptr(t), n, c, d, h, w, ptr(ws), stream()) == 0
    assert lib.biu_mo3d_loss_finish(ptr(tdev), 1, ptr(ws), ptr(saved), stream()) == 0
    grad = None
    if backward:
        gd = torch.tensor([g], device="cuda")
        coef = torch.full((4 * n,), float("nan"), device="cuda")
        assert lib.biu_mo3d_loss_coef(ptr(tdev), 1, ptr(gd), ptr(saved), ptr(coef), stream()) == 0
        grad = torch.full_like(x, float("nan"))
        assert lib.biu_mo3d_loss_bwd(crit.kind, ptr(x), ptr(t), n, c, d, h, w, ptr(coef), ptr(grad), stream()) == 0
    torch.cuda.synchronize()
    s = saved.cpu()
    return float(s[0]), float(s[1]), (grad.cpu() if backward else None)


def _case(case):
    c = CASES[case]
    crit = getattr(L, c["cls"])(*c["args"])
    return crit, torch.from_numpy(Z[f"in.{c['set']}.x"]).cuda(), torch.from_numpy(Z[f"in.{c['set']}.t"]).cuda()


def _check(what, loss, grad, l64, g64, dev_loss, dev_grad):
    err = abs(loss - l64) / abs(l64)
    print(f"{what}: loss rel err {err:.3e} (bound {bound(dev_loss):.3e})", end="")
    gerr = None
    if grad is not None:
        gerr = float((grad.double() - g64).abs().max()) / float(g64.abs().max())
        print(f"  grad rel err {gerr:.3e} (bound {bound(dev_grad):.3e})", end="")
    print()
    assert err <= bound(dev_loss), (what, loss, l64, err)
    assert gerr is None or gerr <= bound(dev_grad), (what, gerr)


def _check_case(case, loss, grad):
    _check(case, loss, grad, float(Z[f"{case}.loss64"]), torch.from_numpy(Z[f"{case}.grad64"]), Z[f"{case}.dev_loss"], Z[f"{case}.dev_grad"])


@pytest.mark.parametrize("case", list(CASES))
def test_c_abi_vs_reference_fp64(case):
    """Every fixture case through biu_mo3d_loss_fwd / _finish / _coef / _bwd; a head weight of 0.5 with an upstream gradient of 2 gives
    half the total and the same gradient."""
    crit, x, t = _case(case)
    total, per, grad = abi_head(crit, x, t)
    assert total == per
    _check_case(case, per, grad)
    total2, per2, grad2 = abi_head(crit, x, t, weight=0.5, g=2.0)
    assert per2 == per and abs(total2 - 0.5 * per) <= 1e-7 * abs(per)
    assert float((grad2 - grad).abs().max()) <= 1e-7 * float(grad.abs().max())


@pytest.mark.parametrize("case", list(CASES))
def test_classes_vs_reference_fp64(case):
    crit, x, t = _case(case)
    x.requires_grad_(True)
    loss = crit(x, t)
    (3.0 * loss).backward()           # an upstream factor reaches the coefficients through the device scalar
    _check_case(case, float(loss.detach()), x.grad.cpu() / 3.0)


KINDS = [("BCEDiceLoss", (1, 1)), ("DiceLoss", ()), ("TverskyLoss", (0.3, 0.7, 0.5)), ("logcoshTverskyLoss", (0.6, 0.4, 2)),
         ("BCEDiceTemporalLoss", ((0.7, 0.3),))]
KIND_IDS = [k[0] for k in KINDS]


def _draw(shape, seed):
    while True:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(shape, generator=g) * 2
        t = (torch.rand(shape, generator=g) < 0.4).float()
        if shape[2] == 1 or float((x[:, :, 1:] - x[:, :, :-1]).abs().min()) >= 1e-4:
            return x, t
        seed += 1


def _cpu(crit, x, t, dt, act=None, grad=True):
    """The torch composition of the module on the CPU in ``dt``: (value, gradient)."""
    xi = x.to(dt).clone().requires_grad_(grad)
    loss = crit(act(xi) if act else xi, t.to(dt))
    if grad:
        loss.backward()
    return float(loss.detach()), (xi.grad if grad else None)


_INPUTS = {}


def _inputs(shape):
    if shape not in _INPUTS:
        _INPUTS[shape] = _draw(shape, 11 * sum(shape))
    return _INPUTS[shape]


@pytest.mark.parametrize("shape", [(3, 2, 5, 37, 53), (2, 1, 16, 64, 64), (2, 1, 2, 8, 8)], ids=["odd", "vec", "pair"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_random_vs_fallback_fp64(kind, shape):
    """Odd extents with two channels (scalar kernels; pairs must not cross channels), a vector-path shape with more than one partial row
    per sample, and a single z-pair."""
    if shape == (2, 1, 16, 64, 64):
        assert lib.biu_mo3d_loss_blocks(int(np.prod(shape))) > 1
    x, t = _inputs(shape)
    crit = getattr(L, kind[0])(*kind[1])
    l64, g64 = _cpu(crit, x, t, torch.float64)
    l32, g32 = _cpu(crit, x, t, torch.float32)
    xd = x.cuda().requires_grad_(True)
    loss = crit(xd, t.cuda())
    loss.backward()
    _check(f"{kind[0]} {shape}", float(loss.detach()), xd.grad.cpu(), l64, g64, abs(l32 - l64) / abs(l64),
           float((g32.double() - g64).abs().max()) / float(g64.abs().max()))


def test_single_plane_temporal_is_nan_others_finite():
    x, t = _inputs((2, 2, 1, 9, 12))
    for name, args in KINDS:
        crit = getattr(L, name)(*args)
        xd = x.cuda().requires_grad_(True)
        loss = crit(xd, t.cuda())
        loss.backward()
        if name == "BCEDiceTemporalLoss":
            assert torch.isnan(loss), name
            assert all(np.isnan(v) for v in abi_head(crit, x.cuda(), t.cuda(), backward=False)[:2])
            assert bool(torch.isfinite(xd.grad).all())          # the BCEDice part's gradient; no pair, no temporal term
        else:
            l64, g64 = _cpu(crit, x, t, torch.float64)
            l32, g32 = _cpu(crit, x, t, torch.float32)
            _check(f"{name} D=1", float(loss.detach()), xd.grad.cpu(), l64, g64, abs(l32 - l64) / abs(l64),
                   float((g32.double() - g64).abs().max()) / float(g64.abs().max()))


ACTS = [None, torch.sigmoid, torch.tanh, torch.relu]


@pytest.mark.parametrize("shape", [(2, 2, 3, 6, 7), (2, 1, 4, 8, 16)], ids=["scalar", "vec"])
@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_pre_act_forward_only(code, shape):
    """``pre_act`` applies the activation to x in registers before everything else: criterion(act(x), t), for x of both signs."""
    x, t = _inputs(shape)
    assert float(x.min()) < -1 and float(x.max()) > 1
    for name, args in (KINDS[3], KINDS[4]):
        crit = getattr(L, name)(*args)
        l64, _ = _cpu(crit, x, t, torch.float64, ACTS[code], grad=False)
        l32, _ = _cpu(crit, x, t, torch.float32, ACTS[code], grad=False)
        _, got, _ = abi_head(crit, x.cuda(), t.cuda(), pre_act=code, backward=False)
        _check(f"{name} pre_act {code} {shape}", got, None, l64, None, abs(l32 - l64) / abs(l64), 0.0)


def test_two_calls_are_bit_equal():
    x, t = _inputs((2, 1, 16, 64, 64))
    for name, args in KINDS:
        runs = []
        for _ in range(2):
            xd = x.cuda().requires_grad_(True)
            loss = getattr(L, name)(*args)(xd, t.cuda())
            loss.backward()
            runs.append((loss.detach().cpu(), xd.grad.cpu()))
        assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), name
        assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), name


def test_unaligned_pointers_take_the_scalar_path():
    """A tensor that starts 4 bytes into an allocation is contiguous but not 16-byte aligned: the scalar kernels run and give what the
    vector kernels give on an aligned copy, up to the summation order."""
    shape = (2, 1, 4, 8, 16)
    x, t = _inputs(shape)
    n = x.numel()
    for name, args in KINDS:
        crit = getattr(L, name)(*args)
        res = []
        for off in (0, 1):
            xb, tb = torch.zeros(n + 4, device="cuda"), torch.zeros(n + 4, device="cuda")
            xd, td = xb[off:off + n].view(shape), tb[off:off + n].view(shape)
            xd.copy_(x), td.copy_(t)
            assert xd.is_contiguous() and xd.data_ptr() % 16 == 4 * off
            xd.requires_grad_(True)
            loss = crit(xd, td)
            g, = torch.autograd.grad(loss, xd)
            res.append((float(loss.detach()), g.cpu()))
        assert abs(res[1][0] - res[0][0]) <= FLOOR * abs(res[0][0]), name
        assert float((res[1][1] - res[0][1]).abs().max()) <= FLOOR * float(res[0][1].abs().max()), name


def test_sample_past_2_31_elements():
    """A sample of 2^31 elements takes 64-bit z arithmetic.  The same memory read as (1, 2, D, H, W) -- one sample of 2^31 -- and as
    (2, 1, D, H, W) -- two samples of 2^30, 32-bit z arithmetic -- holds the same elements and the same z-pairs (none crosses a channel or
    a sample), so the merged sums agree up to their order, and with equal coefficients the two backward passes are bit-equal.  x doubles
    as the target to keep the footprint at two tensors (uniform in (-0.5, 1.5): both signs, and no sum that cancels to zero); the second
    gradient overwrites the first after a checksum."""
    d, h, w = 4096, 512, 512
    x = torch.empty(2 * d * h * w, device="cuda")
    x.uniform_(-0.5, 1.5, generator=torch.Generator(device="cuda").manual_seed(1))
    crit = L.BCEDiceTemporalLoss()
    p = crit._params()
    coef = torch.tensor([1e-3, 2e-3, -3e-3, 0.5] * 2, device="cuda")
    dx = torch.empty_like(x)
    sums, checks = [], []
    for n, c in ((1, 2), (2, 1)):
        rows = lib.biu_mo3d_loss_blocks(x.numel())
        term = (biu_mo3d_term * 1)(biu_mo3d_term(crit.kind, rows, 0, n, x.numel() // n, n * c * (d - 1) * h * w, p[0], p[1], p[2], 1.0))
        tdev = torch.frombuffer(bytearray(bytes(term)), dtype=torch.uint8).cuda()
        ws = torch.full((n * rows * SLOTS,), float("nan"), device="cuda")
        saved = torch.full((HDR + SLOTS * n,), float("nan"), device="cuda")
        assert lib.biu_mo3d_loss_fwd(crit.kind, 0, ptr(x), ptr(x), n, c, d, h, w, ptr(ws), stream()) == 0
        assert lib.biu_mo3d_loss_finish(ptr(tdev), 1, ptr(ws), ptr(saved), stream()) == 0
        dx.fill_(float("nan"))
        assert lib.biu_mo3d_loss_bwd(crit.kind, ptr(x), ptr(x), n, c, d, h, w, ptr(coef), ptr(dx), stream()) == 0
        sums.append(saved[HDR:].view(n, SLOTS).double().sum(0).cpu())
        checks.append((int(dx.view(torch.int64).sum()), int(dx.view(torch.int32).max()), int(dx.view(torch.int32).min()),
                       bool(torch.isfinite(dx[-(1 << 20):]).all())))
    del dx, x
    torch.cuda.empty_cache()
    print("sums", sums[0].tolist(), sums[1].tolist())
    assert bool((sums[0][:5] != 0).all()) and checks[0][3]
    assert float(((sums[0] - sums[1]).abs() / sums[0].abs().clamp_min(1e-30))[:5].max()) <= FLOOR
    assert checks[0] == checks[1]


HEADS = {"a": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "b": {"channels": 1, "activation": "tanh", "loss": "logcoshTverskyLoss", "weight": 0.5},
         "c": {"channels": 1, "activation": "relu", "loss": "BCEDiceTemporalLoss", "weight": 2.0}}
ACT = {"a": torch.sigmoid, "b": torch.tanh, "c": torch.relu}


def test_multi_head_loss_equals_per_class_sum_and_launch_plan():
    shape = (2, 1, 6, 10, 12)
    xs, tg = {}, {}
    for i, k in enumerate(HEADS):
        xs[k], tg[k] = _draw(shape, 50 + i)
        xs[k], tg[k] = xs[k].cuda(), tg[k].cuda()
    tg["b"] = tg["b"][:, 0]              # [N, D, H, W]: viewed as [N, 1, D, H, W]
    leaves = {k: v.clone().requires_grad_(True) for k, v in xs.items()}
    mh = L.MultiHeadLoss(HEADS)
    before = L.launches
    total = mh(leaves, tg)
    total.backward()
    assert L.launches - before == 2 * 3 + 2          # a forward and a backward launch per head, finish, coef
    tg5 = {k: (v.unsqueeze(1) if v.dim() == 4 else v) for k, v in tg.items()}
    want = 0
    for k, cfg in HEADS.items():
        ref = xs[k].clone().requires_grad_(True)
        per = mh.loss_functions[k](ref, tg5[k])
        per.backward()
        want = want + cfg["weight"] * float(per.detach())
        gerr = float((leaves[k].grad - cfg["weight"] * ref.grad).abs().max()) / float(ref.grad.abs().max() * cfg["weight"])
        print(f"head {k}: grad rel err {gerr:.3e}")
        assert gerr <= FLOOR, (k, gerr)
    assert abs(float(total.detach()) - want) <= FLOOR * abs(want), (float(total.detach()), want)
    # forward only, the activations in the kernel: 3 + 1 launches
    acts = {k: cfg["activation"] for k, cfg in HEADS.items()}
    before = L.launches
    with torch.no_grad():
        val = mh(xs, tg, pre_activations=acts)
    assert L.launches - before == 3 + 1
    l64 = sum(cfg["weight"] * _cpu(mh.loss_functions[k], xs[k].cpu(), tg5[k].cpu(), torch.float64, ACT[k], grad=False)[0] for k, cfg in HEADS.items())
    l32 = sum(cfg["weight"] * _cpu(mh.loss_functions[k], xs[k].cpu(), tg5[k].cpu(), torch.float32, ACT[k], grad=False)[0] for k, cfg in HEADS.items())
    _check("validation total", float(val), None, l64, None, abs(l32 - l64) / abs(l64), 0.0)
    # under autograd the activation runs in torch first and the gradient flows through it
    lv = {k: v.clone().requires_grad_(True) for k, v in xs.items()}
    got = mh(lv, tg, pre_activations=acts)
    got.backward()
    assert abs(float(got.detach()) - l64) <= bound(abs(l32 - l64) / abs(l64)) * abs(l64)
    for k, cfg in HEADS.items():
        _, g64 = _cpu(mh.loss_functions[k], xs[k].cpu(), tg5[k].cpu(), torch.float64, ACT[k])
        _, g32 = _cpu(mh.loss_functions[k], xs[k].cpu(), tg5[k].cpu(), torch.float32, ACT[k])
        gerr = float((lv[k].grad.cpu().double() - cfg["weight"] * g64).abs().max()) / float(g64.abs().max() * cfg["weight"])
        assert gerr <= bound(float((g32.double() - g64).abs().max()) / float(g64.abs().max())), (k, gerr)
    # a softmax pre-activation goes through torch, the fused pass follows
    before = L.launches
    with torch.no_grad():
        sm = mh(xs, tg, pre_activations={"a": "softmax", "b": None, "c": None})
    assert L.launches - before == 3 + 1
    want_sm = (float(mh.loss_functions["a"](torch.softmax(xs["a"], dim=1), tg5["a"])) + 0.5 * float(mh.loss_functions["b"](xs["b"], tg5["b"]))
               + 2.0 * float(mh.loss_functions["c"](xs["c"], tg5["c"])))
    assert abs(float(sm) - want_sm) <= FLOOR * abs(want_sm)
    # a criterion that is not one of the five goes through torch and is added; so does a head whose tensors are not fusable
    mixed = L.MultiHeadLoss(HEADS, loss_functions={**mh.loss_functions, "b": torch.nn.L1Loss()})
    lm = {k: v.clone().requires_grad_(True) for k, v in xs.items()}
    before = L.launches
    t2 = mixed(lm, tg)
    t2.backward()
    assert L.launches - before == 2 * 2 + 2
    want2 = (float(mh.loss_functions["a"](xs["a"], tg5["a"])) + 0.5 * float(torch.nn.functional.l1_loss(xs["b"], tg5["b"]))
             + 2.0 * float(mh.loss_functions["c"](xs["c"], tg5["c"])))
    assert abs(float(t2.detach()) - want2) <= 1e-5 * abs(want2)
    assert torch.equal(lm["a"].grad, leaves["a"].grad) and torch.equal(lm["c"].grad, leaves["c"].grad)
    before = L.launches
    with torch.no_grad():
        t3 = mh({**xs, "c": xs["c"].transpose(3, 4)}, {**tg, "c": tg["c"].transpose(3, 4)})         # not contiguous
    assert L.launches - before == 2 + 1
    want3 = (float(mh.loss_functions["a"](xs["a"], tg5["a"])) + 0.5 * float(mh.loss_functions["b"](xs["b"], tg5["b"]))
             + 2.0 * float(mh.loss_functions["c"](xs["c"].transpose(3, 4).contiguous(), tg["c"].transpose(3, 4).contiguous())))
    assert abs(float(t3) - want3) <= 1e-5 * abs(want3)


def test_bad_arguments_return_a_status():
    """Every refusal happens on the host, before anything is launched."""
    x, t = torch.zeros(1, 1, 2, 4, 4, device="cuda"), torch.zeros(1, 1, 2, 4, 4, device="cuda")
    ws, st = torch.zeros(64, device="cuda"), stream()
    fwd, bwd = lib.biu_mo3d_loss_fwd, lib.biu_mo3d_loss_bwd

    def refused(rc):
        assert rc != 0 and lib.biu_last_error()
    refused(fwd(0, 0, ptr(x), ptr(t), 0, 1, 2, 4, 4, ptr(ws), st))             # n = 0
    refused(fwd(0, 0, ptr(x), ptr(t), 1, 1, 0, 4, 4, ptr(ws), st))             # d = 0
    refused(fwd(0, 0, None, ptr(t), 1, 1, 2, 4, 4, ptr(ws), st))               # null pointers
    refused(fwd(0, 0, ptr(x), None, 1, 1, 2, 4, 4, ptr(ws), st))
    refused(fwd(0, 0, ptr(x), ptr(t), 1, 1, 2, 4, 4, None, st))
    refused(fwd(4, 0, ptr(x), ptr(t), 1, 1, 2, 4, 4, ptr(ws), st))             # unknown kind
    assert b"unknown kind" in lib.biu_last_error()
    refused(fwd(0, 4, ptr(x), ptr(t), 1, 1, 2, 4, 4, ptr(ws), st))             # unknown activation code
    refused(fwd(0, 0, ptr(x), ptr(t), 65536, 1, 2, 4, 4, ptr(ws), st))         # more samples than grid rows
    refused(bwd(0, ptr(x), ptr(t), 0, 1, 2, 4, 4, ptr(ws), ptr(ws), st))
    refused(bwd(0, ptr(x), ptr(t), 1, 1, 2, 4, 4, None, ptr(ws), st))
    refused(bwd(0, ptr(x), ptr(t), 1, 1, 2, 4, 4, ptr(ws), None, st))
    refused(bwd(-1, ptr(x), ptr(t), 1, 1, 2, 4, 4, ptr(ws), ptr(ws), st))
    refused(lib.biu_mo3d_loss_finish(None, 1, ptr(ws), ptr(ws), st))
    refused(lib.biu_mo3d_loss_finish(ptr(ws), 0, ptr(ws), ptr(ws), st))
    refused(lib.biu_mo3d_loss_finish(ptr(ws), 17, ptr(ws), ptr(ws), st))
    refused(lib.biu_mo3d_loss_finish(ptr(ws), 1, None, ptr(ws), st))
    refused(lib.biu_mo3d_loss_coef(ptr(ws), 1, None, ptr(ws), ptr(ws), st))
    refused(lib.biu_mo3d_loss_coef(ptr(ws), 0, ptr(ws), ptr(ws), ptr(ws), st))
    refused(lib.biu_mo3d_loss_coef(ptr(ws), 1, ptr(ws), ptr(ws), None, st))
    assert lib.biu_mo3d_loss_blocks(0) == 1 and lib.biu_mo3d_loss_blocks(1 << 40) == 1024
    torch.cuda.synchronize()
    with pytest.raises(BiuError):
        L._call("biu_mo3d_loss_fwd", 9, 0, ptr(x), ptr(t), 1, 1, 2, 4, 4, ptr(ws), st)


class Vols(torch.utils.data.Dataset):
    """The reference data set's item contract: 'volume' (D, H, W) and one target per head, (C, D, H, W) or (D, H, W)."""
    aug_factor, dim_out = 1, (8, 16, 16)

    def __init__(self, n=8):
        g = torch.Generator().manual_seed(0)
        self.items = [{"volume": torch.rand(8, 16, 16, generator=g), "a": (torch.rand(1, 8, 16, 16, generator=g) > 0.5).float(),
                       "b": (torch.rand(8, 16, 16, generator=g) > 0.5).float(), "c": (torch.rand(1, 8, 16, 16, generator=g) > 0.5).float()}
                      for _ in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_trainer_step_equals_per_head_route(tmp_path):
    """One ``TrainerMo3d`` step: the value of ``_total_loss`` and the parameter gradients after ``backward()`` against the per-head route
    (the loop the trainer ran before the fused node, restated from ``tr.loss_functions`` and ``tr.loss_weights``), and the validation value
    against the second-activation quirk.  The model stays in train mode, so a second forward of the same batch gives the same outputs.
    Values are bounded against the torch composition in float64 on the model's outputs; a parameter gradient is linear in the heads'
    gradients, so its bound takes their float32 deviation.  Conv biases in front of a BatchNorm have a true gradient of 0 (rounding noise
    only) and are left out, as in tests/test_gpu_workflow.py."""
    torch.manual_seed(5)
    tr = MO.Trainer(Vols(), HEADS, 1, use_interpolation=True, batch_size=2, n_filter=4, save_dir=str(tmp_path / "m"), device="cuda")
    assert isinstance(tr.head_loss, L.MultiHeadLoss) and tr.head_loss.loss_functions == tr.loss_functions
    batch = next(iter(tr.train_loader))
    x = batch["volume"].unsqueeze(1).cuda()
    y = {k: (batch[k].unsqueeze(1) if batch[k].dim() == 4 else batch[k]).cuda() for k in HEADS}
    before = L.launches
    loss = tr._total_loss(batch, validating=False)
    tr.optimizer.zero_grad()
    loss.backward()
    assert L.launches - before == 2 * 3 + 2
    fused = {k: p.grad.detach().clone() for k, p in tr.model.named_parameters()}
    # the per-head route
    pred = tr.model(x)
    total = 0
    for name in HEADS:
        total = total + tr.loss_weights[name] * tr.loss_functions[name](pred[name], y[name])
    tr.optimizer.zero_grad()
    total.backward()
    l64 = l32 = 0.0
    dev_grad = 0.0
    for name in HEADS:
        p, t = pred[name].detach().cpu(), y[name].cpu()
        a64, g64 = _cpu(tr.loss_functions[name], p, t, torch.float64)
        a32, g32 = _cpu(tr.loss_functions[name], p, t, torch.float32)
        l64, l32 = l64 + tr.loss_weights[name] * a64, l32 + tr.loss_weights[name] * a32
        dev_grad = max(dev_grad, float((g32.double() - g64).abs().max()) / float(g64.abs().max()))
    dev = abs(l32 - l64) / abs(l64)
    _check("trainer total", float(loss.detach()), None, l64, None, dev, 0.0)
    _check("per-head total", float(total.detach()), None, l64, None, dev, 0.0)
    worst = 0.0
    for k, p in tr.model.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("output_layers"):
            continue
        err = float((fused[k] - p.grad).abs().max()) / float(p.grad.abs().max())
        worst = max(worst, err)
        assert err <= bound(dev_grad), (k, err)
    print(f"parameter gradients: worst rel err {worst:.3e} (bound {bound(dev_grad):.3e})")
    # validation: the activation once more on the activated outputs
    before = L.launches
    with torch.no_grad():
        got = float(tr._total_loss(batch, validating=True))
        pred = tr.model(x)
    assert L.launches - before == 3 + 1 and tr.model.training
    v64 = sum(tr.loss_weights[n] * _cpu(tr.loss_functions[n], pred[n].cpu(), y[n].cpu(), torch.float64, ACT[n], grad=False)[0] for n in HEADS)
    v32 = sum(tr.loss_weights[n] * _cpu(tr.loss_functions[n], pred[n].cpu(), y[n].cpu(), torch.float32, ACT[n], grad=False)[0] for n in HEADS)
    _check("validation total", got, None, v64, None, abs(v32 - v64) / abs(v64), 0.0)
