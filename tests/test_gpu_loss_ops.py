"""The single-head segmentation losses of ``bio_image_unet_amd.losses`` on the multi-head loss kernels (``biu_mo3d_loss_*``, a one-term plan;
``biu_pair_smooth_l1_fwd/bwd`` for the batch-axis "time" term, a table term of its own) at their grid limits, and ``biu_head_dlogits``,
against float64 on the host.

Elements per sample are chosen by the launch geometry (``biu_mo3d_loss_blocks(n per)`` block rows per sample: one per 4096 elements of
the whole tensor, at most 1024; ``k_mo3d_finish`` merges a sample's rows with 64 lanes striding over them).  Rows at n = 1 / 2 / 3:

  1                        1 / 1 / 1         a single element
  2049                     1 / 2 / 2         two blocks, the second nearly empty
  64 * 2048 + 1            33 / 65 / 97      65 and 97 rows: the lane stride of the merge takes its second lap
  1024 * 2048 + 3*2048 + 5 514 / 1024 / 1024 the block cap is reached and blocks run their grid-stride loop more than once

Every size is odd, so these run the scalar (V = 1) kernels; the 16-byte ones are covered by the bit-equality with the 3-D criteria below
and by ``test_gpu_mo3d_losses.py``.

Logits are N(0, 3) with 1 % planted at each of +0.0, -0.0, +-20 and +-90 (at +-90 the fp32 sigmoid is exactly 0 or 1); targets are binary or
soft (uniform in [0, 1]).  Value and gradient are checked with the bounds of ``test_fused_seg_losses_against_the_reference_expressions``
against the same float64 expressions (``oracle.unet_oracle``, ``torch.nn.functional.smooth_l1_loss``)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import check, lib, ptr, stream  # noqa: E402

SIZES = [1, 2049, 64 * 2048 + 1, 1024 * 2048 + 3 * 2048 + 5]
ROWS = {1: [1, 1, 33, 514], 2: [1, 2, 65, 1024], 3: [1, 2, 97, 1024]}      # by batch size, in the order of SIZES
BATCHES = {"n1": (1, 0.0), "n3": (3, 0.0), "n2+time": (2, 0.2)}
LOSSES = ["bcedice", "tversky", "logcosh_tversky"]
VALUE_RTOL, GRAD_RTOL, GRAD_ATOL = 2e-6, 2e-4, 2e-6
PLANTED = (0.0, -0.0, 20.0, -20.0, 90.0, -90.0)


def make_inputs(per, n, soft, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * n + (1000 if soft else 0))
    total = n * per
    lg = torch.randn(total, generator=g) * 3
    k = total // 100
    for j, v in enumerate(PLANTED):                              # 1 % each, spread over the whole tensor
        lg[torch.arange(k) * 100 + 7 * j] = v
    r = torch.rand(total, generator=g)
    tg = r if soft else (r > 0.5).float()
    return lg.view(n, 1, per), tg.view(n, 1, per)


def criterion(which):
    from bio_image_unet_amd.losses import BCEDiceLoss, TverskyLoss, logcoshTverskyLoss
    from oracle import unet_oracle as O
    if which == "bcedice":
        return BCEDiceLoss(0.3, 0.7), lambda l, t: O.bce_dice_loss(l, t, 0.3, 0.7)
    if which == "tversky":
        return TverskyLoss(0.3, 0.7), lambda l, t: O.tversky_loss(l, t, 0.3, 0.7)
    return logcoshTverskyLoss(0.6, 0.4), lambda l, t: O.logcosh_tversky_loss(l, t, 0.6, 0.4)


def reference(which, lg, tg, w_time, dt):
    """The eager expression in ``dt`` on the host: (loss, d (1.3 loss) / d logits)."""
    l, t = lg.detach().to(dt).clone().requires_grad_(True), tg.to(dt)
    ref = criterion(which)[1](l, t)
    if w_time:
        ref = ref + w_time * torch.nn.functional.smooth_l1_loss(l[1:], l[:-1])
    (ref * 1.3).backward()
    return float(ref.detach()), l.grad.double()


def deviation(loss, grad, ref, gref):
    """(relative value error, gradient excess over rtol, relative to the largest reference entry)."""
    gmax = float(gref.abs().max())
    return (abs(loss - ref) / max(1.0, abs(ref)),
            float(((grad - gref).abs() - GRAD_RTOL * gref.abs()).max()) / gmax if gmax > 0 else float((grad - gref).abs().max()))


def run_fused(which, lg_dev, tg_dev, w_time):
    l = lg_dev.clone().requires_grad_(True)
    crit = criterion(which)[0]
    loss = crit(l, tg_dev, time_weight=w_time) if w_time else crit(l, tg_dev)
    (loss * 1.3).backward()
    return float(loss.detach()), l.grad.cpu().double()


@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("per", SIZES)
def test_loss_fused_seg_losses_at_the_grid_limits(per, batch, soft):
    n, w_time = BATCHES[batch]
    assert lib.biu_mo3d_loss_blocks(n * per) == ROWS[n][SIZES.index(per)]
    lg, tg = make_inputs(per, n, soft)
    if n * per >= 600:
        p = torch.sigmoid(lg)
        assert float(p.max()) == 1.0 and float(p.min()) < 1.2e-38 and int((lg == 0).sum()) >= 2 * (n * per // 100)      # saturated in fp32
    lg_dev, tg_dev = lg.cuda(), tg.cuda()
    for which in LOSSES:
        loss, grad = run_fused(which, lg_dev, tg_dev, w_time)
        ref, gref = reference(which, lg, tg, w_time, torch.float64)
        dv, dg = deviation(loss, grad, ref, gref)
        print(f"seg loss {which:16s} per {per:8d} {batch:8s} {'soft' if soft else 'binary':6s}: loss {loss:.8f} ref {ref:.8f} "
              f"value dev {dv:.2e} (bound {VALUE_RTOL:.0e}) grad excess {dg:.2e} (bound {GRAD_ATOL:.0e})")
        assert np.isfinite(loss) and bool(torch.isfinite(grad).all())
        assert dv <= VALUE_RTOL, (which, loss, ref)
        assert dg <= GRAD_ATOL, (which, dg)


def _ulp_err(got, want64):
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want64) / ulp).max())


def _mo3d_bwd(lg_dev, tg_dev, n, per, coef, dst):
    """``biu_mo3d_loss_bwd`` of the BCE-Dice kind on ``[n, 1, 1, 1, per]`` with given ``coef[n][4]`` (no temporal term: ct = 0)."""
    return lib.biu_mo3d_loss_bwd(0, ptr(lg_dev), ptr(tg_dev), n, 1, 1, 1, per, ptr(coef), ptr(dst), stream())


@pytest.mark.parametrize("per", [2049, 64 * 2048 + 1])
def test_loss_bwd_accumulate_adds_onto_the_buffer(per):
    """``biu_mo3d_loss_bwd`` (which has no accumulate mode) writes its n * per elements and nothing past them; ``accumulate = 1`` of
    ``biu_pair_smooth_l1_bwd`` onto a non-zero buffer == buffer + the ``accumulate = 0`` result, within 1 ulp (one fp32 addition)."""
    n = 3
    lg, tg = make_inputs(per, n, True, seed=5)
    lg_dev, tg_dev = lg.cuda().contiguous(), tg.cuda().contiguous()
    base = (torch.randn(n * per, generator=torch.Generator().manual_seed(9)) * 0.5 + 2.0)
    assert float(base.abs().min()) > 0
    coef = torch.tensor([[0.7, -0.3, 0.45, 0.0], [-1.1, 0.2, 0.05, 0.0], [0.25, 0.9, -0.6, 0.0]], dtype=torch.float32).cuda()
    ctime = torch.tensor([0.37], dtype=torch.float32).cuda()
    for name, call in (("mo3d_loss_bwd", lambda dst, acc: _mo3d_bwd(lg_dev, tg_dev, n, per, coef, dst)),
                       ("pair_smooth_l1_bwd", lambda dst, acc: lib.biu_pair_smooth_l1_bwd(ptr(lg_dev), n, per, ptr(ctime), ptr(dst), acc, stream()))):
        plain = torch.full((n * per + 8,), float("nan"), device="cuda")
        check(call(plain, 0), name)
        p = plain.cpu().numpy()
        assert np.isnan(p[n * per:]).all() and np.isfinite(p[:n * per]).all()
        assert float(np.abs(p[:n * per]).max()) > 0.1                 # the gradient is not a rounding-size addend
        if name == "mo3d_loss_bwd":
            continue
        onto = torch.cat([base, torch.full((8,), float("nan"))]).cuda()
        check(call(onto, 1), name)
        o = onto.cpu().numpy()
        assert np.isnan(o[n * per:]).all()
        err = _ulp_err(o[:n * per], base.numpy().astype(np.float64) + p[:n * per].astype(np.float64))
        print(f"{name} accumulate, per {per}: worst deviation from buffer + plain {err:.3f} ulp")
        assert err <= 1.0, name


def test_loss_bce_dice_bwd_against_float64():
    """The element-wise gradient formula of ``biu_mo3d_loss_bwd`` with given coefficients, saturated logits and soft targets."""
    n, per = 2, 2049
    lg, tg = make_inputs(per, n, True, seed=6)
    coef = torch.tensor([[0.7, -0.3, 0.45, 0.0], [-1.1, 0.2, 0.05, 0.0]], dtype=torch.float32)
    out = torch.empty(n * per, device="cuda")
    lg_dev, tg_dev, coef_dev = lg.cuda(), tg.cuda(), coef.cuda()
    check(_mo3d_bwd(lg_dev, tg_dev, n, per, coef_dev, out), "mo3d_loss_bwd")
    x, y, c = lg.double().view(n, per), tg.double().view(n, per), coef.double()
    p = torch.sigmoid(x)
    want = c[:, 0:1] * (p - y) + (c[:, 1:2] + c[:, 2:3] * y) * p * (1 - p)
    torch.testing.assert_close(out.cpu().double().view(n, per), want, rtol=GRAD_RTOL, atol=GRAD_ATOL * float(want.abs().max()))


@pytest.mark.parametrize("given", ["both", "logits_only", "act_only"])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_loss_head_dlogits(act, given):
    """out = g_logits + g_act * f'(activated), f' from the activated output, written into channels [1, 3) of a 4-channel NaN buffer.
    Bound: 1e-6 of |g_logits| + |g_act f'| per element (the two terms may cancel; that is the data's doing, not the kernel's)."""
    n, ch, S, ctot, c0 = 2, 2, 3 * 5 * 7, 4, 1
    g = torch.Generator().manual_seed(40 + act)
    z = torch.randn(n, ch, S, generator=g) * 2
    z.view(-1)[::17] = 0.0
    av = (z, torch.sigmoid(z), torch.tanh(z), torch.relu(z))[act].contiguous()
    gl, ga = torch.randn(n, ch, S, generator=g), torch.randn(n, ch, S, generator=g)
    use_l, use_a = given != "act_only", given != "logits_only"
    dst = torch.full((n, ctot, S), float("nan"), device="cuda")
    keep = [t.cuda() for t in (gl, ga, av)]
    check(lib.biu_head_dlogits(ptr(keep[0]) if use_l else None, ptr(keep[1]) if use_a else None, ptr(keep[2]), act, n, ch, S, ptr(dst), ctot, c0,
                               stream()), "head_dlogits")
    a64 = av.double()
    d = (torch.ones_like(a64), a64 * (1 - a64), 1 - a64 * a64, (a64 > 0).double())[act]
    t_l, t_a = (gl.double() if use_l else torch.zeros_like(a64)), (ga.double() * d if use_a else torch.zeros_like(a64))
    got = dst.cpu().double()
    assert bool(torch.isnan(got[:, 0]).all()) and bool(torch.isnan(got[:, 3]).all())
    err = (got[:, c0:c0 + ch] - (t_l + t_a)).abs()
    assert bool((err <= 1e-6 * (t_l.abs() + t_a.abs())).all()), float((err / (t_l.abs() + t_a.abs() + 1e-300)).max())
    if act == 3 and use_a and not use_l:
        assert bool((got[:, c0:c0 + ch][av == 0] == 0).all())        # relu'(0) = 0


# --- the single-head criteria as plans of the multi-head loss ------------------------------------------------------------------------
def _value_and_grad(crit, x, t, **kw):
    l = x.clone().requires_grad_(True)
    loss = crit(l, t, **kw)
    (loss * 1.3).backward()
    return loss.detach().cpu(), l.grad.cpu()


@pytest.mark.parametrize("shape", [(3, 2, 2, 3, 4), (3, 1, 1, 3, 5)], ids=["v4", "v1"])
def test_loss_single_head_equals_the_3d_criteria_bit_for_bit(shape):
    """The same kernels now: value and gradient of the three criteria equal those of ``multi_output_unet3d.losses`` bit for bit, with
    16-byte accesses (per % 4 == 0) and with scalar ones."""
    from bio_image_unet_amd import losses as S
    from bio_image_unet_amd.multi_output_unet3d import losses as M
    g = torch.Generator().manual_seed(11)
    x, t = (torch.randn(shape, generator=g) * 3).cuda(), torch.rand(shape, generator=g).cuda()
    assert (x[0].numel() % 4 == 0) == (shape == (3, 2, 2, 3, 4))
    for a, b in ((S.BCEDiceLoss(1, 1), M.BCEDiceLoss(1, 1)), (S.TverskyLoss(0.3, 0.7, 1), M.TverskyLoss(0.3, 0.7, 1)),
                 (S.logcoshTverskyLoss(), M.logcoshTverskyLoss())):
        (la, ga), (lb, gb) = _value_and_grad(a, x, t), _value_and_grad(b, x, t)
        assert np.isfinite(float(la)) and torch.equal(la, lb), (type(a).__name__, float(la), float(lb))
        assert float(ga.abs().max()) > 0 and torch.equal(ga, gb), type(a).__name__


def test_loss_single_head_rank4_equals_its_rank5_view():
    from bio_image_unet_amd import losses as S
    g = torch.Generator().manual_seed(12)
    x, t = (torch.randn(3, 1, 5, 7, generator=g) * 3).cuda(), torch.rand(3, 1, 5, 7, generator=g).cuda()
    for crit in (S.BCEDiceLoss(1, 1), S.TverskyLoss(0.3, 0.7, 1), S.logcoshTverskyLoss()):
        l4, l5 = crit(x, t), crit(x.view(3, 1, 1, 5, 7), t.view(3, 1, 1, 5, 7))
        assert np.isfinite(float(l4)) and torch.equal(l4, l5), type(crit).__name__


@pytest.mark.parametrize("which", ["bcedice", "tversky"])
@pytest.mark.parametrize("n,per", [(2, 5), (3, 4096 + 4)])
def test_loss_time_term_is_a_table_term(n, per, which):
    """``time_weight`` as the K_PAIRSL1 term of the plan: value and gradient against the float64 torch composition, three launches each way
    (fwd, pair fwd, finish; coef, bwd, pair bwd).  At n = 3, per = 4100 both terms have more than one block row."""
    from bio_image_unet_amd import losses as S
    from bio_image_unet_amd.multi_output_unet3d import losses as M
    from oracle import unet_oracle as O
    if per > 4096:
        assert lib.biu_mo3d_loss_blocks(n * per) > 1 and lib.biu_pair_smooth_l1_blocks((n - 1) * per) > 1
    lg, tg = make_inputs(per, n, True, seed=21)
    crit, ref_fn = ((S.BCEDiceLoss(1, 1), lambda l, t: O.bce_dice_loss(l, t, 1, 1)) if which == "bcedice" else
                    (S.TverskyLoss(0.3, 0.7, 1), lambda l, t: O.tversky_loss(l, t, 0.3, 0.7, 1)))
    l = lg.cuda().requires_grad_(True)
    before = M.launches
    loss = crit(l, tg.cuda(), time_weight=0.1)
    assert M.launches - before == 3
    (loss * 1.3).backward()
    assert M.launches - before == 6
    lr, tr = lg.double().requires_grad_(True), tg.double()
    ref = ref_fn(lr, tr) + 0.1 * torch.nn.functional.smooth_l1_loss(lr[1:], lr[:-1])
    (ref * 1.3).backward()
    dv, dg = deviation(float(loss.detach()), l.grad.cpu().double(), float(ref.detach()), lr.grad)
    print(f"time term {which:8s} n {n} per {per}: loss {float(loss.detach()):.8f} ref {float(ref.detach()):.8f} value dev {dv:.2e} grad excess {dg:.2e}")
    assert dv <= VALUE_RTOL, (float(loss.detach()), float(ref.detach()))
    assert dg <= GRAD_ATOL, dg


def test_loss_time_term_of_a_batch_of_one_is_nan():
    from bio_image_unet_amd import losses as S
    lg, tg = make_inputs(5, 1, True, seed=22)
    for crit in (S.BCEDiceLoss(1, 1), S.TverskyLoss(0.3, 0.7, 1)):
        assert torch.isnan(crit(lg.cuda(), tg.cuda(), time_weight=0.1))
        assert np.isfinite(float(crit(lg.cuda(), tg.cuda())))


def test_loss_dice_smooth_reaches_the_kernels():
    """``SoftDiceLoss.smooth`` is p2 of the BCE-Dice term: 0.5 against float64 (and away from the value at smooth = 1)."""
    from bio_image_unet_amd import losses as S
    from oracle import unet_oracle as O
    g = torch.Generator().manual_seed(23)
    lg, tg = torch.randn(2, 1, 3, 4, generator=g) * 3, torch.rand(2, 1, 3, 4, generator=g)
    crit = S.BCEDiceLoss(0.3, 0.7)
    crit.dice.smooth = 0.5
    l = lg.cuda().requires_grad_(True)
    loss = crit(l, tg.cuda())
    (loss * 1.3).backward()
    lr, tr = lg.double().requires_grad_(True), tg.double()
    ref = 0.3 * torch.nn.functional.binary_cross_entropy_with_logits(lr, tr) + 0.7 * O.soft_dice_loss(lr, tr, 0.5)
    (ref * 1.3).backward()
    dv, dg = deviation(float(loss.detach()), l.grad.cpu().double(), float(ref.detach()), lr.grad)
    print(f"dice smooth 0.5: loss {float(loss.detach()):.8f} ref {float(ref.detach()):.8f} value dev {dv:.2e} grad excess {dg:.2e}")
    assert abs(float(ref.detach()) - float(O.bce_dice_loss(lr, tr, 0.3, 0.7).detach())) > 1e-3          # the smooth matters at this size
    assert dv <= VALUE_RTOL and dg <= GRAD_ATOL, (dv, dg)
