"""The 2-D multi-output networks on the GPU: the bilinear x2 (align_corners=True) kernel against PyTorch, and MultiOutputUnet /
MultiOutputNestedUNet / _3Levels against the fp64 functional oracle (tests/mo2d_oracle.py) on the engine's own branch decisions."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bio_image_unet_amd as B  # noqa: E402
from bio_image_unet_amd import engine as E  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402
from tests import mo2d_oracle as M  # noqa: E402
from tests.gpu_util import DT, XF, Dev, assert_close, check, lib, stream  # noqa: E402

REL = 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# the op
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 8, 1, 1), (2, 7, 2, 2), (1, 1, 3, 5), (2, 130, 5, 3), (1, 64, 64, 64), (2, 8, 3, 64), (1, 130, 2, 1)]


def _pad(c):
    return (c + 7) // 8 * 8 + 8


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_bilinear_up_vs_torch(shape, pitched, dtype):
    """biu_bilinear_up_fwd / _bwd against F.interpolate(bilinear, align_corners=True) on the CPU and its autograd adjoint: a random
    transform with negative scales, pitched slices (vector path with a scalar tail for 130 channels) or dense rows, accumulate 0 / 1;
    the backward repeats bit for bit and nothing outside the slices is touched."""
    n, c, h, w = shape
    code = DT[dtype][1]
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, c, h, w, generator=g)
    kw = dict(pitch=_pad(c), c0=8) if pitched else {}
    xd = Dev(x, dtype=dtype, **kw)
    od = Dev(shape=(n, c, 1, 2 * h, 2 * w), dtype=dtype, **kw)
    xf = XF(c, seed=c)
    xa = xf.apply(xd.ref()).squeeze(2).requires_grad_(True)
    ref = F.interpolate(xa, scale_factor=2, mode="bilinear", align_corners=True)
    check(lib.biu_bilinear_up_fwd(xd.a(), xf.x(), od.a(), code, stream()), "bilinear_up_fwd")
    torch.cuda.synchronize()
    assert_close(od.get(squeeze2d=True), ref.detach(), dtype, "bilinear fwd")
    if pitched:
        assert torch.isnan(od.buf[..., :8].float()).all() and torch.isnan(od.buf[..., 8 + c:].float()).all(), "wrote outside its slice"
    gout = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    gd = Dev(gout, dtype=dtype, **kw)
    ref.backward(gd.ref().squeeze(2))
    dxd = Dev(shape=(n, c, 1, h, w), dtype=dtype, **kw)
    check(lib.biu_bilinear_up_bwd(gd.a(), dxd.a(), 0, code, stream()), "bilinear_up_bwd")
    torch.cuda.synchronize()
    assert_close(dxd.get(squeeze2d=True), xa.grad, dtype, "bilinear bwd")
    first = dxd.buf.clone()
    check(lib.biu_bilinear_up_bwd(gd.a(), dxd.a(), 0, code, stream()), "bilinear_up_bwd (again)")
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.uint8) if first.dtype == torch.bfloat16 else first.view(torch.int32),
                       dxd.buf.view(torch.uint8) if first.dtype == torch.bfloat16 else dxd.buf.view(torch.int32)), "backward not reproducible"
    if pitched:
        assert torch.isnan(dxd.buf[..., :8].float()).all() and torch.isnan(dxd.buf[..., 8 + c:].float()).all(), "wrote outside its slice"
    base = torch.randn(n, c, h, w, generator=g)
    acc = Dev(base, dtype=dtype, **kw)
    check(lib.biu_bilinear_up_bwd(gd.a(), acc.a(), 1, code, stream()), "bilinear_up_bwd(acc)")
    torch.cuda.synchronize()
    assert_close(acc.get(squeeze2d=True), acc_ref(base, dtype) + xa.grad, dtype, "bilinear bwd accumulate")


def acc_ref(base, dtype):
    return base.to(DT[dtype][0]).float()


def test_bilinear_up_refuses_bad_shapes():
    x = Dev(torch.randn(1, 4, 3, 3))
    o = Dev(shape=(1, 4, 1, 6, 7))
    assert lib.biu_bilinear_up_fwd(x.a(), None, o.a(), DT["f32"][1], stream()) != 0
    assert lib.biu_bilinear_up_bwd(o.a(), x.a(), 0, DT["f32"][1], stream()) != 0
    v = Dev(shape=(1, 4, 2, 3, 3))
    vo = Dev(shape=(1, 4, 2, 6, 6))
    assert lib.biu_bilinear_up_fwd(v.a(), None, vo.a(), DT["f32"][1], stream()) != 0


# ---------------------------------------------------------------------------------------------------------------------------------
# whole networks
# ---------------------------------------------------------------------------------------------------------------------------------
HEADS3 = {"a": {"channels": 1, "activation": "sigmoid", "weight": 0.5}, "b": {"channels": 2, "activation": None},
          "c": {"channels": 1, "activation": "tanh", "weight": 2.0}}
HEADS2 = {"a": {"channels": 1, "activation": "sigmoid"}, "b": {"channels": 2, "activation": "relu", "weight": 0.5}}

# kind -> (class, ctor kwargs, input shape, levels)
CASES = {
    "nested_f32": (B.MultiOutputNestedUNet, dict(in_channels=1, output_heads=HEADS3, n_filter=32), (2, 1, 128, 128), 4),
    "nested_ds_f16": (B.MultiOutputNestedUNet, dict(in_channels=1, output_heads=HEADS2, n_filter=16, deep_supervision=True,
                                                    dilation=(1, 2, 1, 1, 2)), (2, 1, 64, 64), 4),
    "nested3_ds_f16": (B.MultiOutputNestedUNet_3Levels, dict(in_channels=2, output_heads=HEADS2, n_filter=16, deep_supervision=True,
                                                             dilation=(2, 1, 1, 1)), (2, 2, 32, 48), 3),
    "mo2d_f32": (B.MultiOutputUnet, dict(in_channels=1, output_heads=HEADS3, n_filter=32), (2, 1, 64, 64), 4),
}


def _problem(kind, seed=0):
    cls, kw, shape, levels = CASES[kind]
    torch.manual_seed(seed)
    m = cls(**kw)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(shape, generator=g)
    tg = {name: torch.rand((shape[0], cfg["channels"]) + shape[2:], generator=g) for name, cfg in kw["output_heads"].items()}
    return cls, kw, levels, sd, x, tg


def _loss(out, tg, kw, levels):
    return M.weighted_mse(out, tg, kw["output_heads"], deep_supervision=kw.get("deep_supervision", False), levels=levels)


def _oracle(cls, kw, levels, sd, x, training, cat_paths=None):
    heads = kw["output_heads"]
    if cls is B.MultiOutputUnet:
        return M.mo2d_forward(sd, x, heads, training=training)
    return M.nested_forward(sd, x, heads, levels=levels, deep_supervision=kw.get("deep_supervision", False),
                            train_mode=kw.get("train_mode", True), dilation=kw.get("dilation", False), training=training, cat_paths=cat_paths)


def _oracle_run(cls, kw, levels, sd, x, tg, dt, cat_paths=None):
    osd = O.clone_state({k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}, requires_grad=True)
    out = _oracle(cls, kw, levels, osd, x.to(dt), True, cat_paths)
    loss = _loss(out, {k: v.to(dt) for k, v in tg.items()}, kw, levels)
    return out, loss, O.grads_of(loss, osd), osd


def _hip_run(cls, kw, sd, x, tg, levels, dtype):
    m = cls(**kw)
    m.load_state_dict(sd)
    m.cuda().train()
    if dtype == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    out = m(x.cuda())
    loss = _loss(out, {k: v.cuda() for k, v in tg.items()}, kw, levels)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    return m, {k: v.detach().cpu() for k, v in out.items()}, float(loss), grads


def relerr(got, want):
    return float((got.double() - want.double()).abs().max()) / (float(want.abs().max()) + 1e-12)


def _grad_errors(grads, truth):
    gscale = max(float(v.abs().max()) for v in truth.values())
    out = {}
    for k, want in truth.items():
        got, want = grads[k].double(), want.double()
        e = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-2 * gscale)
        l2 = float((got - want).norm() / (want.norm() + 1e-3 * gscale * want.numel() ** 0.5))
        cos = float((got * want).sum() / (got.norm() * want.norm() + 1e-300))
        out[k] = (e, l2, cos)
    return out


def _dead(k):
    """Conv biases in front of a train-mode BatchNorm: their true gradient is exactly 0."""
    return k.endswith((".conv1.bias", ".conv2.bias", ".0.bias"))


def _engine(m):
    return list(m._engines.values())[-1][-1]


@pytest.mark.parametrize("kind", list(CASES))
def test_midsize_fp32_vs_oracle(kind):
    """fp32 engine against the fp64 oracle on the branch the engine took (as test_gpu_models.test_midsize_fp32_vs_oracle): outputs,
    loss, every parameter gradient, BatchNorm buffers and the eval forward within 1e-3.  The F = 32 nested case must read every
    concatenation through the two-source kernels (no x_r_j copied); narrow rows take the copy path."""
    from tests import insitu
    cls, kw, levels, sd, x, tg = _problem(kind)
    m, outs, loss, grads = _hip_run(cls, kw, sd, x, tg, levels, "f32")
    eng = _engine(m)
    paths = getattr(eng, "cat_paths", None)
    if kind == "nested_f32":
        assert paths and set(paths.values()) == {"two-source"}, paths
        assert not any(isinstance(nd, E.CopyNode) for nd in eng.nodes)
    if kind == "nested_ds_f16":
        assert paths["conv0_1"] == "copy" and "two-source" in paths.values(), paths
    q = insitu.extract_decisions(eng)
    with O.record_decisions() as rq:
        f_outs, f_loss, _, _ = _oracle_run(cls, kw, levels, sd, x, tg, torch.float32)
    for k, (d, t) in insitu.decision_mismatch(q, rq).items():
        assert d <= 1e-4 * t + 2, f"{k}: {d} of {t} decisions differ from the free-running fp32 oracle"
    with O.forced_decisions(q):
        t_outs, t_loss, t_grads, osd = _oracle_run(cls, kw, levels, sd, x, tg, torch.float64)
    assert list(outs) == list(t_outs)
    for k, want in t_outs.items():
        assert relerr(outs[k], want) < REL, f"{k} rel err vs fp64 {relerr(outs[k], want)}"
        assert relerr(outs[k], f_outs[k].detach()) < REL, f"{k} rel err vs fp32 {relerr(outs[k], f_outs[k].detach())}"
    assert abs(loss - float(t_loss)) < REL * max(1.0, abs(float(t_loss)))
    assert set(grads) == set(t_grads), set(grads) ^ set(t_grads)
    mine = _grad_errors(grads, t_grads)
    gmax = max(float(v.abs().max()) for v in t_grads.values())
    for k, (e, l2, cos) in mine.items():
        if _dead(k):
            continue
        assert e <= REL, f"grad {k}: err {e} > 1e-3"
        if float(t_grads[k].abs().max()) > 1e-3 * gmax:
            assert cos > 0.99999, f"grad {k}: cosine {cos}"
    msd = m.state_dict()
    for k in sd:
        if "running_" in k:
            torch.testing.assert_close(msd[k].cpu().double(), osd[k].detach(), rtol=REL, atol=REL)
    m.eval()
    with torch.no_grad():
        oe = m(x.cuda())
        re_ = _oracle(cls, kw, levels, {k: v.detach() for k, v in osd.items()}, x.double(), False)
    for k, want in re_.items():
        assert relerr(oe[k].cpu(), want) < REL, f"eval {k}: {relerr(oe[k].cpu(), want)}"


@pytest.mark.parametrize("kind", ["nested_f32", "nested_ds_f16", "mo2d_f32"])
def test_midsize_bf16_vs_oracle(kind):
    """bf16 engine against the fp64 oracle with the bounds of test_gpu_models.test_midsize_bf16_vs_oracle: no further from it than
    the oracle's own bf16-storage emulation (outputs rms <= 1.5x, gradients per parameter L2 <= 1.6x + 0.03)."""
    cls, kw, levels, sd, x, tg = _problem(kind)
    m, outs, loss, grads = _hip_run(cls, kw, sd, x, tg, levels, "bf16")
    t_outs, t_loss, t_grads, _ = _oracle_run(cls, kw, levels, sd, x, tg, torch.float64)
    with O.emulate_bf16():
        e_outs, e_loss, e_grads, _ = _oracle_run(cls, kw, levels, sd, x, tg, torch.float32, getattr(_engine(m), "cat_paths", None))
    for k, want in t_outs.items():
        assert relerr(outs[k], want) < 0.15, f"{k} rel err {relerr(outs[k], want)}"
        d_h = float((outs[k].double() - want).pow(2).mean().sqrt())
        d_e = float((e_outs[k].detach().double() - want).pow(2).mean().sqrt())
        assert d_h <= 1.5 * d_e + 1e-3 * float(want.abs().max()), f"{k}: rms deviation {d_h} vs the emulation's {d_e}"
    assert abs(loss - float(t_loss)) < 5e-2
    mine, emu = _grad_errors(grads, t_grads), _grad_errors(e_grads, t_grads)
    gmax = max(float(v.abs().max()) for v in t_grads.values())
    for k, (e, l2, cos) in mine.items():
        if _dead(k):
            continue
        assert l2 <= 1.6 * emu[k][1] + 0.03, f"grad {k}: L2 error {l2} vs the bf16 emulation's {emu[k][1]}"
        if float(t_grads[k].abs().max()) > 1e-3 * gmax:
            assert cos >= min(0.99, emu[k][2] - 0.05), f"grad {k}: cosine {cos} vs the emulation's {emu[k][2]}"


@pytest.mark.parametrize("cls", [B.MultiOutputNestedUNet, B.MultiOutputNestedUNet_3Levels])
def test_train_mode_false_equals_last_level(cls):
    """deep supervision without train_mode: the reference's keys (one per head), bit-equal to the last-level outputs of a train_mode
    model with the same weights."""
    torch.manual_seed(3)
    a = cls(1, HEADS2, 16, deep_supervision=True).cuda()
    b = cls(1, HEADS2, 16, deep_supervision=True, train_mode=False).cuda()
    b.load_state_dict(a.state_dict())
    x = torch.rand(2, 1, 32, 32, device="cuda")
    with torch.no_grad():
        oa, ob = a(x), b(x)
    L = a.levels
    assert list(oa) == sum(([f"{n}_{l}" for l in range(1, L + 1)] + [n] for n in HEADS2), [])
    assert all(oa[n] is oa[f"{n}_{L}"] for n in HEADS2)
    assert list(ob) == list(HEADS2)
    for n in HEADS2:
        assert torch.equal(ob[n], oa[f"{n}_{L}"]), n


def test_bf16_step_reproducible():
    """Two identical bf16 steps: loss and outputs repeat bit for bit; gradients agree to fp32 rounding (within 2.5e-7 of the net's largest
    gradient, README "reproducible": the weight-gradient sums of the first layer are accumulated with float atomics; measured 1.2e-7 of
    that tensor's own maximum for conv0_0.conv1.weight of this network)."""
    cls, kw, levels, sd, x, tg = _problem("nested_ds_f16")
    runs = [_hip_run(cls, kw, sd, x, tg, levels, "bf16") for _ in range(2)]
    (_, o1, l1, g1), (_, o2, l2, g2) = runs
    assert l1 == l2
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    gmax = max(float(v.abs().max()) for v in g1.values())
    for k in g1:
        assert float((g1[k] - g2[k]).abs().max()) <= 2.5e-7 * gmax, k


def test_trainer_step_clip_adam():
    """What the reference trainer does with network=MultiOutputNestedUNet (train.py:31-32, 157-186): construct with its keywords,
    init_weights, the deep-supervision loss, clip_grad_norm_(1.0) and torch Adam -- the clipped norm and the updated weights match
    the oracle's."""
    from bio_image_unet_amd.utils import init_weights
    torch.manual_seed(5)
    m = B.MultiOutputNestedUNet(n_filter=16, in_channels=1, output_heads=HEADS2, dilation=False, deep_supervision=True)
    m.apply(init_weights)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.cuda().train()
    x = torch.rand(2, 1, 32, 32)
    tg = {n: torch.rand(2, c["channels"], 32, 32) for n, c in HEADS2.items()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    out = m(x.cuda())
    assert m.deep_supervision
    loss = M.weighted_mse(out, {k: v.cuda() for k, v in tg.items()}, HEADS2, deep_supervision=True, levels=4)
    opt.zero_grad()
    loss.backward()
    norm = float(torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=1.0))
    opt.step()
    kw = dict(output_heads=HEADS2, deep_supervision=True)
    from tests import insitu
    with O.forced_decisions(insitu.extract_decisions(_engine(m))):       # on the engine's own LeakyReLU / max-pool branch
        _, o_loss, o_grads, _ = _oracle_run(B.MultiOutputNestedUNet, kw, 4, sd, x, tg, torch.float64)
    upd, o_norm = O.adam_step({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, o_grads, lr=1e-3, clip=1.0)
    assert abs(float(loss) - float(o_loss)) < REL * max(1.0, abs(float(o_loss)))
    assert abs(norm - float(o_norm)) < 1e-3 * float(o_norm)
    msd = m.state_dict()
    for k, want in upd.items():
        if _dead(k):
            continue
        live = o_grads[k].abs() > 1e-3 * float(o_grads[k].abs().max())       # Adam's first step is ~lr * sign(g): compare where g is no tie
        d = (msd[k].cpu().double() - sd[k].double()) - (want - sd[k].double())
        assert float(d[live].abs().max()) < 1e-4, k


def test_bad_extent_raises():
    m = B.MultiOutputNestedUNet(1, HEADS2, 8).cuda()
    with pytest.raises(RuntimeError):
        m(torch.rand(1, 1, 40, 48, device="cuda"))
    u = B.MultiOutputUnet(1, HEADS2, 8).cuda()
    with pytest.raises(ValueError):
        u(torch.rand(1, 1, 40, 48, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's own numbers (tests/golden/make_golden_mo2d.py)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mo2d_f2", "nested_f2", "nested_f2_ds", "nested3_f4_ds"])
def test_golden_train_step_fp32(case):
    """As test_gpu_models.test_golden_train_step_fp32: outputs, loss, every gradient (1e-3 of its scale + 1e-5 of the net's), BatchNorm
    buffers, eval forward, the fused clip + Adam kernels against the reference's clip_grad_norm_ + torch Adam, and the second forward."""
    from bio_image_unet_amd.optim import Adam
    from tests import mo2d_golden as MG
    from tests.golden_util import load_case
    g = load_case(case)
    m = MG.build(g["meta"]).cuda()
    m.load_state_dict(g["sd"])
    m.train()
    x = g["in"]["x"].cuda()
    tg = {k: v.cuda() for k, v in MG.targets(g).items()}
    outs = m(x)
    assert list(outs) == list(g["train"])
    for k, v in g["train"].items():
        assert relerr(outs[k].detach().cpu(), v) < REL, f"train.{k}"
    loss = MG.loss(g, outs, tg)
    assert abs(float(loss) - float(g["loss"])) < REL * max(1.0, abs(float(g["loss"])))
    loss.backward()
    gscale = max(float(v.abs().max()) for v in g["grad"].values())
    off = []
    for k, p in m.named_parameters():
        want = g["grad"][k]
        got = p.grad.cpu() if p.grad is not None else torch.zeros_like(want)
        if float((got - want).abs().max()) > REL * float(want.abs().max()) + 1e-5 * gscale:
            off.append(k)
    if off:
        # A LeakyReLU / max-pool decision within fp32 rounding of its boundary may fall the other way than in the reference's CPU run (the
        # narrow first blocks of these F = 2 nets sum the whole gradient through a few such decisions).  Then the engine's decisions differ
        # from the free-running fp32 oracle's in a handful of elements only, and on the engine's own branch every such gradient is within
        # the bound of the fp64 oracle.
        from tests import insitu
        q = insitu.extract_decisions(_engine(m))
        with O.record_decisions() as rq, torch.no_grad():
            MG.forward(g, O.clone_state(g["sd"]), g["in"]["x"], True)
        flips = insitu.decision_mismatch(q, rq)
        assert sum(d for d, _ in flips.values()) > 0, f"gradients {off} off the reference's with identical decisions"
        for kind, (d, t) in flips.items():
            assert d <= 1e-4 * t + 2, f"{kind}: {d} of {t} decisions differ"
        with O.forced_decisions(q):
            osd = O.clone_state({k: (v.double() if v.is_floating_point() else v) for k, v in g["sd"].items()}, requires_grad=True)
            tl = MG.loss(g, MG.forward(g, osd, g["in"]["x"].double(), True), {k: v.double() for k, v in MG.targets(g).items()})
            tgr = O.grads_of(tl, osd)
        params = dict(m.named_parameters())
        for k in off:
            got, want = params[k].grad.cpu().double(), tgr[k]
            tol = REL * float(want.abs().max()) + 1e-5 * gscale
            assert float((got - want).abs().max()) <= tol, f"grad.{k}: {float((got - want).abs().max())} > {tol} on the engine's branch"
    sd_now = m.state_dict()
    for k, v in g["sd1"].items():
        torch.testing.assert_close(sd_now[k].cpu(), v, rtol=REL, atol=1e-5, msg=lambda s: f"sd1.{k}: {s}")
    m.eval()
    with torch.no_grad():
        oe = m(x)
    for k, v in g["eval"].items():
        assert relerr(oe[k].cpu(), v) < REL, f"eval.{k}"
    m.train()
    opt = Adam(m.parameters(), lr=1e-3)
    if g["gradnorm"] is not None:
        norm = opt.clip_grad_norm_(1.0)
        assert abs(float(norm) - float(g["gradnorm"])) < REL * float(g["gradnorm"]), (float(norm), float(g["gradnorm"]))
    opt.step()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        want, g0 = g["adam1"][k], g["grad"][k]
        solid = g0.abs() > 20 * (2 * REL * float(g0.abs().max()) + 1e-5 * gscale)
        got = p.detach().cpu()
        assert float((got - want).abs().max()) <= 2.0e-3 + 1e-6, f"adam1.{k}: an entry moved by more than 2 lr"
        if solid.any():
            assert float((got - want)[solid].abs().max()) <= 2e-5, f"adam1.{k}: {float((got - want)[solid].abs().max())}"
    sd_ref = {k: v.clone() for k, v in m.state_dict().items()}
    sd_ref.update(g["adam1"])
    m.load_state_dict(sd_ref)
    with torch.no_grad():
        loss2 = MG.loss(g, m(x), tg)
    assert abs(float(loss2) - float(g["loss2"])) < REL * max(1.0, abs(float(g["loss2"])))
    sd_now = m.state_dict()
    for k, v in g["sd2"].items():
        torch.testing.assert_close(sd_now[k].cpu(), v, rtol=REL, atol=1e-5, msg=lambda s: f"sd2.{k}: {s}")
