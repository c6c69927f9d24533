"""The in-situ checker's own formulas (tests/insitu.py) against torch autograd in float64: the checker is the only reference for the
span, copy, deep-supervision and eval-backward paths, so what it expects is pinned here -- small random tensors, no engine, no GPU.
Every expectation comes from the functions the hooks call; nothing is re-implemented."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests import insitu as I

TOL = 1e-10            # float64 against float64: rounding of a few hundred terms of O(1)
SLOPE = float(torch.tensor(I.LRELU, dtype=torch.float32))      # the slope as the engine's fp32 transform vector holds it
FP32_TOL = 1e-5        # the checker's fp32 element tolerance (InSitu.close: 1e-5 * rms): what "tells apart" has to exceed by far


def _rand(*shape, seed):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_bilinear_is_align_corners_true():
    a = _rand(2, 3, 1, 3, 5, seed=1)
    got = I.resample_ref("bilinear", a, (2, 1, 6, 10))
    assert got.shape == (2, 3, 1, 6, 10)
    true = F.interpolate(a.squeeze(2), scale_factor=2, mode="bilinear", align_corners=True).unsqueeze(2)
    false = F.interpolate(a.squeeze(2), scale_factor=2, mode="bilinear", align_corners=False).unsqueeze(2)
    assert float((got - true).abs().max()) <= TOL
    rms = float(true.pow(2).mean().sqrt())
    assert float((got - false).abs().max()) > 1e3 * FP32_TOL * rms, "the two conventions must be far apart at this size"
    # the adjoint the backward hook takes from autograd is that of the same op
    av = a.clone().requires_grad_(True)
    g = _rand(2, 3, 1, 6, 10, seed=2)
    (gx,) = torch.autograd.grad(I.resample_ref("bilinear", av, (2, 1, 6, 10)), av, g)
    bv = a.squeeze(2).clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.interpolate(bv, scale_factor=2, mode="bilinear", align_corners=True), bv, g.squeeze(2))
    assert float((gx.squeeze(2) - ref).abs().max()) <= TOL


def test_trilinear_keeps_align_corners_false():
    a = _rand(1, 2, 2, 3, 4, seed=3)
    got = I.resample_ref("trilinear", a, (1, 4, 6, 8))
    assert float((got - F.interpolate(a, scale_factor=2, mode="trilinear", align_corners=False)).abs().max()) <= TOL


def _bn_problem(seed):
    n, cin, c, h, w = 2, 3, 4, 5, 6
    x = _rand(n, cin, h, w, seed=seed)
    wt = (_rand(c, cin, 3, 3, seed=seed + 1) * 0.3).requires_grad_(True)
    b = _rand(c, seed=seed + 2).requires_grad_(True)
    gamma = (_rand(c, seed=seed + 3).abs() + 0.5) * torch.tensor([1.0, -1.0, 1.0, 1.0], dtype=torch.float64)      # one negative scale
    gamma.requires_grad_(True)
    beta = _rand(c, seed=seed + 4).requires_grad_(True)
    rm = _rand(c, seed=seed + 5) * 0.3
    rv = _rand(c, seed=seed + 6).abs() + 0.5
    da = _rand(n, c, h, w, seed=seed + 7)
    return x, wt, b, gamma, beta, rm, rv, da


def _checker_side(y, da, gamma, beta, mean, invstd, batch_stats):
    """What bwd_ConvBlockNode_post computes: dz from the consumer transform (dact), then bn_bwd_expect."""
    scale = (gamma * invstd).float()
    shift = (beta - mean * gamma * invstd).float()
    fac, _ = I.dact(y.unsqueeze(2), (scale, shift, torch.full_like(scale, SLOPE)))
    return I.bn_bwd_expect(da.unsqueeze(2) * fac, y.unsqueeze(2), mean, invstd, gamma, batch_stats)


def test_eval_batchnorm_backward_equals_autograd_and_differs_from_train_form():
    x, wt, b, gamma, beta, rm, rv, da = _bn_problem(10)
    eps = 1e-5
    y = F.conv2d(x, wt, b, padding=1)
    y.retain_grad()
    out = F.leaky_relu(F.batch_norm(y, rm, rv, gamma, beta, training=False, eps=eps), SLOPE)
    out.backward(da)
    ex = _checker_side(y.detach(), da, gamma.detach(), beta.detach(), rm, torch.rsqrt(rv + eps), False)
    for got, want, what in ((ex["dy"].squeeze(2), y.grad, "dy"), (ex["dgamma"], gamma.grad, "dgamma"), (ex["dbeta"], beta.grad, "dbeta"),
                            (ex["dbias"], b.grad, "conv dbias")):
        assert float((got - want).abs().max()) <= TOL * (1 + float(want.abs().max())), what
    assert float(b.grad.abs().max()) > 0.1          # a live number, not rounding noise
    # the batch-statistics formula on the same operands is another function: the check can tell the two apart
    tr = _checker_side(y.detach(), da, gamma.detach(), beta.detach(), rm, torch.rsqrt(rv + eps), True)
    assert float((tr["dy"] - ex["dy"]).abs().max()) > 1e3 * FP32_TOL * float(ex["dy"].pow(2).mean().sqrt())
    assert float((tr["dbias"] - ex["dbias"]).abs().max()) > 1e3 * 1e-4 * float(ex["dbias"].abs().max())


def test_train_batchnorm_backward_equals_autograd_with_zero_conv_bias_gradient():
    x, wt, b, gamma, beta, _, _, da = _bn_problem(20)
    eps = 1e-5
    y = F.conv2d(x, wt, b, padding=1)
    y.retain_grad()
    out = F.leaky_relu(F.batch_norm(y, None, None, gamma, beta, training=True, eps=eps), SLOPE)
    out.backward(da)
    yd = y.detach()
    mean, var = yd.mean(dim=(0, 2, 3)), yd.var(dim=(0, 2, 3), unbiased=False)
    ex = _checker_side(yd, da, gamma.detach(), beta.detach(), mean, torch.rsqrt(var + eps), True)
    for got, want, what in ((ex["dy"].squeeze(2), y.grad, "dy"), (ex["dgamma"], gamma.grad, "dgamma"), (ex["dbeta"], beta.grad, "dbeta")):
        assert float((got - want).abs().max()) <= TOL * (1 + float(want.abs().max())), what
    assert int(torch.count_nonzero(ex["dbias"])) == 0
    assert float(b.grad.abs().max()) <= 1e-12, "autograd's conv bias gradient behind a batch-statistics BatchNorm is rounding noise"


def test_span_accumulates_leaf_by_leaf():
    """A row buffer of three leaves A | B | C whose gradient memory starts as garbage.  Reader 1 (a deep-supervision head) reads A alone;
    reader 2 reads the parts (span(A, B), C) of a concatenation: A was written, B is zero-filled because A was, C is fresh."""
    n, h, w = 2, 3, 4
    wa, wb, wc = 2, 3, 2
    leaves = [_rand(n, c, 1, h, w, seed=30 + i).requires_grad_(True) for i, c in enumerate((wa, wb, wc))]
    A, Bl, Cl = leaves
    k1 = _rand(n, wa, 1, h, w, seed=40)
    k2 = _rand(n, wa + wb + wc, 1, h, w, seed=41)
    total = (A * k1).sum() + (torch.cat([A, Bl, Cl], 1) * k2).sum()               # the sum of the readers
    ga, gb, gc = torch.autograd.grad(total, leaves)
    buf = torch.full((n, wa + wb + wc, 1, h, w), float("nan"), dtype=torch.float64)
    flags = [False, False, False]
    # reader 1 writes A
    before = I.span_before(flags[:1], [wa], buf[:, :wa])
    assert before is None
    buf[:, :wa] = I.accumulated(k1, before)
    flags[0] = True
    # reader 2: first part span(A, B), second part C
    b0 = I.span_before(flags[:2], [wa, wb], buf[:, :wa + wb])
    assert b0 is not None and torch.equal(b0[:, :wa], k1) and int(torch.count_nonzero(b0[:, wa:])) == 0
    b1 = I.span_before(flags[2:], [wc], buf[:, wa + wb:])
    assert b1 is None
    buf[:, :wa + wb] = I.accumulated(k2[:, :wa + wb], b0)
    buf[:, wa + wb:] = I.accumulated(k2[:, wa + wb:], b1)
    assert torch.isfinite(buf).all(), "a leaf nobody had written leaked its garbage into the expectation"
    for got, want in ((buf[:, :wa], ga), (buf[:, wa:wa + wb], gb), (buf[:, wa + wb:], gc)):
        assert float((got - want).abs().max()) <= TOL
    # the snapshot is a copy: the buffer's later writes do not reach it
    assert torch.equal(b0[:, :wa], k1)


def test_heads_are_grouped_and_differentiated_per_trunk():
    """Two trunks: x1 with one sigmoid head, x2 with two stacked heads (tanh 1 channel, relu 2 channels), listed interleaved."""
    n, c, h, w = 2, 5, 3, 4
    x1 = _rand(n, c, 1, h, w, seed=50).requires_grad_(True)
    x2 = _rand(n, c, 1, h, w, seed=51).requires_grad_(True)
    t1, t2 = object(), object()
    spec = [(t2, x2, 2, 1), (t1, x1, 1, 1), (t2, x2, 3, 2)]              # (trunk Act, its T(x), activation code, channels)
    fn = {1: torch.sigmoid, 2: torch.tanh, 3: F.relu}
    heads, live, loss = [], [], 0
    for i, (t, x, act, co) in enumerate(spec):
        wt = _rand(co, c, seed=60 + i).requires_grad_(True)
        b = _rand(co, seed=70 + i).requires_grad_(True)
        out = fn[act](torch.einsum("ncdhw,oc->nodhw", x, wt) + b.view(1, -1, 1, 1, 1))
        ga = _rand(*out.shape, seed=80 + i)
        loss = loss + (out * ga).sum()
        hd = SimpleNamespace(xin=t, act=act, w=wt, b=b, x=x)
        heads.append(hd)
        live.append((hd, I.head_dlogits(act, None, ga, out.detach())))
    groups = I.group_by_trunk(live)
    assert [[h.act for h, _ in g] for g in groups] == [[2, 3], [1]]
    earlier = _rand(n, c, 1, h, w, seed=90)              # a gradient trunk x1 already held
    for grp in groups:
        x = grp[0][0].x
        before = earlier if x is x1 else None
        dx, per = I.head_group_expect(x.detach(), [(hd.w.detach(), dl) for hd, dl in grp], before)
        (gx,) = torch.autograd.grad(loss, x, retain_graph=True)
        assert float((dx - I.accumulated(gx, before)).abs().max()) <= TOL
        for (hd, _), (dw, db) in zip(grp, per):
            gw, gb = torch.autograd.grad(loss, (hd.w, hd.b), retain_graph=True)
            assert float((dw - gw).abs().max()) <= TOL and float((db - gb).abs().max()) <= TOL
