"""Pin tests/mo2d_oracle.py to vectors the reference's own multi_output_unet code produced (tests/golden/make_golden_mo2d.py): train
forward, loss, every gradient, BatchNorm buffers, eval forward, clip + Adam step and the second forward, with the bounds of
tests/test_oracle_golden.py; and the HIP classes carry exactly the fixtures' state_dict keys."""
import pytest
import torch

from oracle import unet_oracle as O
from tests import mo2d_golden as MG
from tests.golden_util import load_case

RTOL, ATOL = 1e-5, 1e-6


@pytest.mark.parametrize("case", MG.CASES)
def test_mo2d_oracle_matches_reference_vectors(case):
    torch.set_num_threads(4)
    g = load_case(case)
    tg = MG.targets(g)
    sd = O.clone_state(g["sd"], requires_grad=True)
    outs = MG.forward(g, sd, g["in"]["x"], True)
    assert list(outs) == list(g["train"])
    for k, v in g["train"].items():
        torch.testing.assert_close(outs[k].detach(), v, rtol=RTOL, atol=ATOL, msg=lambda m: f"train.{k}: {m}")
    loss = MG.loss(g, outs, tg)
    torch.testing.assert_close(loss.detach(), g["loss"], rtol=RTOL, atol=ATOL)
    grads = O.grads_of(loss, sd)
    assert set(grads) == set(g["grad"])
    gscale = max(float(v.abs().max()) for v in g["grad"].values())
    for k, v in g["grad"].items():
        scale = float(v.abs().max())
        torch.testing.assert_close(grads[k], v, rtol=1e-4, atol=1e-5 * scale + 1e-6 * gscale, msg=lambda m: f"grad.{k}: {m}")
    for k, v in g["sd1"].items():
        torch.testing.assert_close(sd[k].detach(), v, rtol=RTOL, atol=ATOL, msg=lambda m: f"sd1.{k}: {m}")
    with torch.no_grad():
        outs_e = MG.forward(g, sd, g["in"]["x"], False)
    for k, v in g["eval"].items():
        torch.testing.assert_close(outs_e[k], v, rtol=RTOL, atol=ATOL, msg=lambda m: f"eval.{k}: {m}")
    clip = 1.0 if g["gradnorm"] is not None else None
    new, norm = O.adam_step(sd, grads, lr=1e-3, clip=clip)
    if clip is not None:
        torch.testing.assert_close(norm, g["gradnorm"], rtol=1e-4, atol=0)
    assert set(new) == set(g["adam1"])
    for k, v in g["adam1"].items():
        solid = g["grad"][k].abs() > 1e-4 * gscale
        torch.testing.assert_close(new[k][solid], v[solid], rtol=1e-5, atol=2e-6, msg=lambda m: f"adam1.{k}: {m}")
        assert float((new[k] - v).abs().max()) <= 2.0e-3 + 1e-6, f"adam1.{k}: an entry moved by more than 2 lr"
    sd2 = O.clone_state({**{k: v for k, v in sd.items() if not O.is_param(k)}, **g["adam1"]}, requires_grad=False)
    with torch.no_grad():
        loss2 = MG.loss(g, MG.forward(g, sd2, g["in"]["x"], True), tg)
    torch.testing.assert_close(loss2, g["loss2"], rtol=RTOL, atol=ATOL)
    for k, v in g["sd2"].items():
        torch.testing.assert_close(sd2[k], v, rtol=RTOL, atol=ATOL, msg=lambda m: f"sd2.{k}: {m}")


@pytest.mark.parametrize("case", MG.CASES)
def test_hip_classes_carry_the_fixture_keys(case):
    g = load_case(case)
    m = MG.build(g["meta"])
    sd = m.state_dict()
    assert list(sd) == list(g["sd"])
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in g["sd"].items())
    m.load_state_dict(g["sd"])
