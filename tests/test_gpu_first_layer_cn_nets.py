"""Whole networks with 2 to 4 input channels, every kernel call checked on the operands the engine holds (tests/insitu.py, as
tests/test_gpu_insitu.py runs it): one training step in bf16 and in fp32 of a 2-D U-Net with three input channels, a 3-D U-Net with two and
a 3-D multi-output U-Net with four.  Their first block runs on the first-layer kernels (the 16-channel one of the 2-D net on csrc/biu_c1.hip in
bf16, the 8-channel ones of the 3-D nets and everything in fp32 on csrc/biu_special.hip); the in-situ model holds it to fp32 weights times the stored input.  A step that asks for the gradient of the input still gets it:
the first layer's data gradient stays on the any-shape kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bio_image_unet_amd as B  # noqa: E402
from bio_image_unet_amd import engine as E  # noqa: E402
from bio_image_unet_amd._lib import lib  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402
from tests import insitu  # noqa: E402
from tests.test_gpu_insitu import HEADS, OUTLIER_FRAC, _loss  # noqa: E402

CASES = {
    "unet2d_c3_f16": (lambda: B.Unet(3, 1, 16), lambda: O.init_unet2d(3, 1, 16, seed=31), (2, 3, 32, 32)),
    "unet3d_c2_f16": (lambda: B.UNet3D(2, 1, 16), lambda: O.init_unet3d(2, 1, 16, seed=32), (1, 2, 16, 32, 32)),
    "mo3d_c4_f16": (lambda: B.MultiOutputUnet3D(4, HEADS, 16, True), lambda: O.init_mo3d(4, HEADS, 16, True, seed=33), (1, 4, 16, 32, 32)),
}


def _model(case, dtype):
    mk, init, shape = CASES[case]
    torch.manual_seed(0)
    m = mk().cuda()
    m.load_state_dict(init())
    if dtype == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    m.train()
    return m, torch.rand(*shape).cuda()


def _first_block(eng):
    return next(n for n in eng.nodes if isinstance(n, E.ConvBlockNode))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_every_kernel_call_of_a_train_step(case, dtype):
    m, x = _model(case, dtype)
    chk = insitu.attach(m, [x], dtype == "bf16")
    nd = _first_block(chk.eng)
    assert nd.xin.c == CASES[case][2][1] and nd.y.c == (16 if len(CASES[case][2]) == 4 else 8)      # (the 3-D nets open with n_filter / 2)
    assert lib.biu_conv_first_ok(nd.xin.a(), nd.y.a(), nd.kd, nd.kh, nd.kw, nd.dil, chk.eng.dtype) == 1, "the first block is not on the first-layer kernels"
    _loss(case, m(x)).backward()
    torch.cuda.synchronize()
    rep = chk.rep
    assert len(rep.rows) > 100
    assert not chk.failures, "\n".join(chk.failures[:20]) + "\n" + rep.table()
    assert rep.n_out <= OUTLIER_FRAC[dtype] * rep.n_elem, f"{rep.n_out} of {rep.n_elem} elements beyond 1x tolerance"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_step_that_asks_for_the_input_gradient_still_gets_it(dtype):
    """requires_grad on the input: the first-layer kernels have no data gradient, the any-shape one writes it.  Every call of the step is
    checked in situ; in fp32 the gradient is also held to the eager float64 network within 1e-3 of its largest element (the bound the
    parity tests of this suite put on an fp32 step), in bf16 (chaotic against another rounding of the activations) it has to be there."""
    m, x = _model("unet2d_c3_f16", dtype)
    x.requires_grad_(True)
    chk = insitu.attach(m, [x], dtype == "bf16")
    out = m(x)
    torch.manual_seed(5)
    tgt = (torch.rand_like(out[1]) > 0.5).float()
    O.bce_dice_loss(out[1], tgt).backward()
    torch.cuda.synchronize()
    assert not chk.failures, "\n".join(chk.failures[:20])
    g = x.grad
    assert g is not None and g.shape == x.shape and torch.isfinite(g).all() and float(g.abs().max()) > 0
    if dtype == "f32":
        sd = O.clone_state({k: (v.double() if v.is_floating_point() else v) for k, v in CASES["unet2d_c3_f16"][1]().items()})
        xr = x.detach().cpu().double().requires_grad_(True)
        _, logits = O.unet2d_forward(sd, xr, training=True)
        O.bce_dice_loss(logits, tgt.cpu().double()).backward()
        err = float((g.cpu().double() - xr.grad).abs().max() / xr.grad.abs().max())
        print(f"input gradient: {err:.3e} of the largest element")
        assert err < 1e-3
