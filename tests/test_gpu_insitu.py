"""Whole-network steps verified kernel call by kernel call on the operands the engine actually holds (tests/insitu.py):
the sharp form of network parity -- ~1 ulp of the storage type per call, in fp32 AND bf16 -- that a comparison of final
gradients cannot give (discrete LeakyReLU / max-pool decisions, chaotic bf16 rounding; see profiles/r02_bf16_error_budget.md).

Shapes are the MFMA widths of the BASELINE configs at reduced extent: cfg2 (Unet F=64, 2 outputs), cfg3 (Siam 'max' F=32),
cfg4 (UNet3D F=32), cfg5 (MultiOutputUnet3D, 3 heads, both up-sampling modes; F=32 keeps the 16-channel layers of cfg4 and
the stacked-head backward), plus Siam 'concat' (two-source bottleneck join, copy join and its backward).

The 2-D multi-output family at the smallest extents that keep ragged MFMA tiles and a multi-voxel bottleneck: MultiOutputUnet and
U-Net++ (MultiOutputNestedUNet, _3Levels) with their pitched prefix sources (Buf.span), the bilinear up-sampling inside the graph, the
copy path of the narrow rows, dilated blocks on the direct kernels and deep supervision (one head backward per trunk, spans whose
leaves are written only in part when the prefix gradient arrives).  Every case also runs as an eval-mode backward where listed
(EVAL_BWD): running statistics as constants, live conv-bias gradients, the folded decoder's ConvT-bias chain through dy_sum.
Measured: profiles/r12_insitu_mo2d.txt."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import bio_image_unet_amd as B  # noqa: E402
from bio_image_unet_amd import engine as E  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402
from tests import insitu  # noqa: E402
from tests import mo2d_oracle as M  # noqa: E402

HEADS = {"seg": {"channels": 1, "activation": "sigmoid"}, "flow": {"channels": 2, "activation": None},
         "dist": {"channels": 1, "activation": "tanh"}}

HEADS5 = {"seg": {"channels": 1, "activation": "sigmoid"}, "flow": {"channels": 2, "activation": None},
          "dist": {"channels": 1, "activation": "sigmoid"}}          # bench.HEADS5: cfg5 as benchmarked

HEADS_DS = {"seg": {"channels": 1, "activation": "sigmoid"}, "flow": {"channels": 2, "activation": "relu", "weight": 0.5}}


def _init_like(module, seed):
    """state_dict with the module's own (PyTorch default + Kaiming-normal Conv2d) initialisation under a fixed seed."""
    from bio_image_unet_amd.utils import init_weights
    torch.manual_seed(seed)
    for mod in module.modules():
        if hasattr(mod, "reset_parameters"):
            mod.reset_parameters()
    module.apply(init_weights)
    return {k: v.clone() for k, v in module.state_dict().items()}


CASES = {
    "unet2d_f16": (lambda: B.Unet(1, 1, 16), lambda: O.init_unet2d(1, 1, 16, seed=3), (2, 1, 64, 64), 1),
    "cfg2_unet2d_f64_o2": (lambda: B.Unet(1, 2, 64), lambda: O.init_unet2d(1, 2, 64, seed=4), (2, 1, 64, 64), 1),
    "cfg3_siam_max_f32": (lambda: B.Siam_UNet(32, "max"), lambda: O.init_unet2d(1, 1, 32, seed=5, init_weights=False), (2, 1, 64, 64), 2),
    "siam_concat_f16": (lambda: B.Siam_UNet(16, "concat"), lambda: O.init_unet2d(1, 1, 16, seed=6, init_weights=False, siam_mode="concat"), (2, 1, 64, 64), 2),
    "attention_f16": (lambda: B.AttentionUnet(1, 1, 16), lambda: _init_like(B.AttentionUnet(1, 1, 16), 10), (2, 1, 64, 64), 1),
    "unet_v0_f16": (lambda: B.Unet_v0(16), lambda: _init_like(B.Unet_v0(16), 11), (2, 1, 64, 64), 1),
    "cfg4_unet3d_f32": (lambda: B.UNet3D(1, 1, 32), lambda: O.init_unet3d(1, 1, 32, seed=7), (2, 1, 16, 32, 32), 1),
    "cfg5_mo3d_f32_interp": (lambda: B.MultiOutputUnet3D(1, HEADS, 32, True), lambda: O.init_mo3d(1, HEADS, 32, True, seed=8), (1, 1, 16, 32, 32), 1),
    "cfg5_mo3d_f32_convT": (lambda: B.MultiOutputUnet3D(1, HEADS, 32, False), lambda: O.init_mo3d(1, HEADS, 32, False, seed=9), (1, 1, 16, 32, 32), 1),
    # cfg5 at its stated width: base 64 (3-D layers of 512 / 768 input channels), heads and activations of bench.py
    "cfg5_mo3d_f64_interp": (lambda: B.MultiOutputUnet3D(1, HEADS5, 64, True), lambda: O.init_mo3d(1, HEADS5, 64, True, seed=12), (1, 1, 16, 32, 32), 1),
    "cfg5_mo3d_f64_convT": (lambda: B.MultiOutputUnet3D(1, HEADS5, 64, False), lambda: O.init_mo3d(1, HEADS5, 64, False, seed=13), (1, 1, 16, 32, 32), 1),
}

# the 2-D multi-output family: name -> (class, ctor kwargs, input shape, levels); the loss is the reference trainer's weighted MSE over
# every head and, with deep supervision, every level (tests/mo2d_oracle.weighted_mse), so that every output key carries gradient
MO2D = {
    "nested_f32w_o3": (B.MultiOutputNestedUNet, dict(in_channels=1, output_heads=HEADS, n_filter=32), (2, 1, 64, 48), 4),
    "nested_ds_f16_dil": (B.MultiOutputNestedUNet, dict(in_channels=1, output_heads=HEADS_DS, n_filter=16, deep_supervision=True,
                                                       dilation=(1, 2, 1, 1, 2)), (2, 1, 32, 48), 4),
    "nested3_ds_f16_c2": (B.MultiOutputNestedUNet_3Levels, dict(in_channels=2, output_heads=HEADS_DS, n_filter=16, deep_supervision=True,
                                                                dilation=(2, 1, 1, 1)), (1, 2, 24, 40), 3),
    "mo2d_f32w_o3": (B.MultiOutputUnet, dict(in_channels=1, output_heads=HEADS, n_filter=32), (2, 1, 48, 64), 4),
}
for _i, (_k, (_cls, _kw, _shape, _lv)) in enumerate(MO2D.items()):
    CASES[_k] = (lambda c=_cls, kw=_kw: c(**kw), lambda c=_cls, kw=_kw, i=_i: _init_like(c(**kw), 20 + i), _shape, 1)

EVAL_BWD = ["cfg4_unet3d_f32", "cfg5_mo3d_f32_interp", "siam_concat_f16", "nested_ds_f16_dil"]


def _loss(case, outs):
    if case in MO2D:
        _, kw, _, levels = MO2D[case]
        tg = {k: torch.rand_like(outs[k]) for k in kw["output_heads"]}
        return M.weighted_mse(outs, tg, kw["output_heads"], deep_supervision=kw.get("deep_supervision", False), levels=levels)
    if isinstance(outs, dict):
        tg = {k: torch.rand_like(v) for k, v in outs.items()}
        return sum(((outs[k] - tg[k]) ** 2).mean() * w for k, w in (("seg", 1.0), ("flow", 0.5), ("dist", 0.25)))
    y = (torch.rand_like(outs[1]) > 0.5).float()
    return O.bce_dice_loss(outs[1], y) + 0.05 * outs[0].mean()          # both outputs carry gradient


def _assert_paths(case, eng, chk):
    """The path a case is about, so that a dispatch change cannot silently empty it."""
    copies = [n for n in eng.nodes if isinstance(n, E.CopyNode)]
    if case == "nested_f32w_o3":
        assert set(eng.cat_paths.values()) == {"two-source"} and not copies, eng.cat_paths
    if case == "nested_ds_f16_dil":
        assert eng.cat_paths["conv0_1"] == "copy" and "two-source" in eng.cat_paths.values() and copies, eng.cat_paths
        assert chk.head_groups == 4, chk.head_groups
    if case == "nested3_ds_f16_c2":
        assert chk.head_groups == 3, chk.head_groups
    if case in ("nested_ds_f16_dil", "nested3_ds_f16_c2"):
        assert chk.partial_spans, "no span was found written only in part when its prefix gradient was written"
        assert any(isinstance(n, E.ConvBlockNode) and n.dil == 2 for n in eng.nodes)


def _report(tag, case, dtype, chk, seconds, capsys):
    w, rep = chk.rep.worst(), chk.rep
    line = (f"[insitu{tag} {case} {dtype}] {len(rep.rows)} checks, {rep.n_elem} elements, {rep.n_out} beyond 1x tolerance "
            f"({rep.n_out / max(rep.n_elem, 1):.2e}) in {len(rep.outliers)} checks; worst: {w[0]} / {w[1]} = {w[2]:.3f}x tolerance, {w[3]:.6f} within; "
            f"{seconds:.1f} s")
    with capsys.disabled():
        print("\n" + line)
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "insitu_outliers.txt"), "a") as f:
        f.write(line + "\n")
        for lab, what, no, n, dev in sorted(rep.outliers, key=lambda r: -r[4])[:8]:
            f.write(f"    {lab:28s} {what:22s} {no} of {n} beyond 1x, worst {dev:.2f}x\n")
    return line


# measured (profiles/r03_insitu_outliers.txt): fp32 0 of 2.4e8 elements over all networks; bf16 0 everywhere except Unet_v0 (70 of 3.9e6 =
# 1.8e-5 at 1.2-1.5x: tensors whose gradient has two writers / the 1-channel block, where an intermediate bf16 rounding of the engine
# and of the checker's float64 model fall on different sides of a rounding boundary)
# (profiles/r12_insitu_mo2d.txt: the 1-channel block's share was the checker's own data-gradient predicate, since corrected -- Unet_v0 15 of
# 3.9e6; the U-Net++ prefixes, gradients with up to five writers, reach 8.0e-6 of a step at 1.1-1.6x.  The bounds stay as they were.)
OUTLIER_FRAC = {"f32": 2e-6, "bf16": 1e-4}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_every_kernel_call_of_a_train_step(case, dtype, capsys):
    t0 = time.perf_counter()
    mk, init, shape, nin = CASES[case]
    torch.manual_seed(0)
    m = mk().cuda()
    m.load_state_dict(init())
    if dtype == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    m.train()
    xs = [torch.rand(*shape).cuda() for _ in range(nin)]
    chk = insitu.attach(m, xs, dtype == "bf16")
    loss = _loss(case, m(*xs))
    loss.backward()
    torch.cuda.synchronize()
    rep = chk.rep
    line = _report("", case, dtype, chk, time.perf_counter() - t0, capsys)
    assert len(rep.rows) > 100
    assert not chk.failures, "\n".join(chk.failures[:20]) + "\n" + rep.table()
    # over the whole step: elements beyond their tolerance are the rare ones whose decision / rounding boundary lies inside the
    # kernel's own rounding (each check already needs 99.9 % within 1x and nothing beyond 64x); bounded here so that a drift shows
    assert rep.n_out <= OUTLIER_FRAC[dtype] * rep.n_elem, line
    _assert_paths(case, chk.eng, chk)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_kernel_call_of_an_eval_forward(dtype):
    """Eval mode: running statistics, no statistics epilogue -- the other form of every forward kernel."""
    torch.manual_seed(1)
    m = B.UNet3D(1, 1, 32).cuda()
    sd = O.init_unet3d(1, 1, 32, seed=7)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.randn_like(sd[k]) * 0.1
        if k.endswith("running_var"):
            sd[k] = torch.rand_like(sd[k]) + 0.5
    m.load_state_dict(sd)
    if dtype == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    m.eval()
    x = torch.rand(1, 1, 16, 32, 32).cuda()
    chk = insitu.attach(m, [x], dtype == "bf16")
    with torch.no_grad():
        m(x)
    assert len(chk.rep.rows) > 30
    assert not chk.failures, "\n".join(chk.failures[:20])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", EVAL_BWD)
def test_every_kernel_call_of_an_eval_backward(case, dtype, capsys):
    """``model.eval(); loss.backward()`` (frozen-BatchNorm fine-tuning): the running statistics are constants, so dy = gamma * invstd * dz
    (biu_bn_bwd_finalize_eval), the conv bias gradient is live, no reader reduces BatchNorm sums on the way and the folded decoder's
    ConvT-bias chain rule takes sum_v dy from ``dy_sum`` -- the other form of every backward kernel call."""
    t0 = time.perf_counter()
    mk, init, shape, nin = CASES[case]
    torch.manual_seed(1)
    m = mk().cuda()
    sd = init()
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.randn_like(sd[k]) * 0.1
        if k.endswith("running_var"):
            sd[k] = torch.rand_like(sd[k]) + 0.5
    m.load_state_dict(sd)
    if dtype == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    m.eval()
    xs = [torch.rand(*shape).cuda() for _ in range(nin)]
    chk = insitu.attach(m, xs, dtype == "bf16")
    loss = _loss(case, m(*xs))
    loss.backward()
    torch.cuda.synchronize()
    rep = chk.rep
    line = _report(" eval-bwd", case, dtype, chk, time.perf_counter() - t0, capsys)
    blocks = [n for n in chk.eng.nodes if isinstance(n, E.ConvBlockNode)]
    assert blocks and not any(n.batch_stats for n in blocks), "a block normalised with batch statistics in eval mode"
    assert any(n.conv.bias is not None and n.conv.bias.grad is not None and bool(n.conv.bias.grad.ne(0).any()) for n in blocks), \
        "every conv bias gradient is zero: the eval-mode backward did not run"
    assert any(r[1] == "conv dbias (eval)" for r in rep.rows) and not any(r[1] == "conv dbias == 0" for r in rep.rows)
    assert len(rep.rows) > 100
    assert not chk.failures, "\n".join(chk.failures[:20]) + "\n" + rep.table()
    assert rep.n_out <= OUTLIER_FRAC[dtype] * rep.n_elem, line
    if case == "nested_ds_f16_dil":
        _assert_paths(case, chk.eng, chk)
