"""CPU-side checks of the 2-D multi-output networks (no GPU): the reference's state_dict schema, the constructor contract of the
reference trainer, the CPU refusal, and the functional oracle (tests/mo2d_oracle.py) against the same networks built from plain
torch.nn modules in the reference's structure."""
import pytest
import torch
import torch.nn.functional as F

import bio_image_unet_amd as B
from bio_image_unet_amd import multi_output_unet as MO
from tests import mo2d_oracle as M

HEADS = {"a": {"channels": 1, "activation": "sigmoid"}, "b": {"channels": 2, "activation": None}, "c": {"channels": 1, "activation": "tanh"}}


def _expected_keys(levels, in_channels, f, heads, deep_supervision):
    """The reference's registration order (multi_output_nested_unet.py:58-118): blocks column by column, then the heads."""
    nb = [f << r for r in range(levels + 1)]
    blocks = [(f"conv{r}_0", in_channels if r == 0 else nb[r - 1], nb[r]) for r in range(levels + 1)]
    blocks += [(f"conv{r}_{j}", nb[r] * j + nb[r + 1], nb[r]) for j in range(1, levels + 1) for r in range(levels + 1 - j)]
    keys = []
    for name, cin, cout in blocks:
        for i, ci in ((1, cin), (2, cout)):
            keys += [(f"{name}.conv{i}.weight", (cout, ci, 3, 3)), (f"{name}.conv{i}.bias", (cout,))]
            keys += [(f"{name}.bn{i}.{k}", s) for k, s in (("weight", (cout,)), ("bias", (cout,)), ("running_mean", (cout,)),
                                                              ("running_var", (cout,)), ("num_batches_tracked", ()))]
    for name, cfg in heads.items():
        for key in ([f"{name}_{l}" for l in range(1, levels + 1)] if deep_supervision else [name]):
            keys += [(f"output_layers.{key}.weight", (cfg["channels"], f, 1, 1)), (f"output_layers.{key}.bias", (cfg["channels"],))]
    return keys


@pytest.mark.parametrize("cls,levels", [(B.MultiOutputNestedUNet, 4), (B.MultiOutputNestedUNet_3Levels, 3)])
@pytest.mark.parametrize("ds", [False, True])
def test_nested_state_dict_schema(cls, levels, ds):
    m = cls(2, HEADS, 4, deep_supervision=ds)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _expected_keys(levels, 2, 4, HEADS, ds)
    assert [k for k, _ in m.named_children()][:2] == ["pool", "up"] and list(m._modules)[-1] == "output_layers"
    assert list(m.conv1_1._modules) == ["relu", "conv1", "bn1", "conv2", "bn2", "dropout"]
    m.load_state_dict(cls(2, HEADS, 4, deep_supervision=ds).state_dict())


def test_multi_output_unet_schema_and_kwargs():
    m = B.MultiOutputUnet(**{"in_channels": 1, "output_heads": HEADS, "n_filter": 4, "dilation": 2, "deep_supervision": True})
    assert m.deep_supervision is False
    keys = list(m.state_dict())
    u = B.Unet(1, 1, 4)
    body = [k for k in u.state_dict() if not k.startswith("final")]
    assert keys[:len(body)] == body
    assert keys[len(body):] == [f"output_layers.{n}.{p}" for n in HEADS for p in ("weight", "bias")]
    assert m.encode1[0].dilation == (1, 1)


def test_constructor_defaults():
    m = B.MultiOutputNestedUNet()
    assert m.dilation == (1, 1, 1, 1, 1) and not m.deep_supervision and m.train_mode
    assert list(m.output_heads) == ["default"] and m.conv0_0.conv1.out_channels == 32
    m3 = B.MultiOutputNestedUNet_3Levels(n_filter=8, in_channels=1, output_heads=HEADS, dilation=False, deep_supervision=True)
    assert m3.dilation == (1, 1, 1, 1) and not hasattr(m3, "conv4_0")
    d = B.MultiOutputNestedUNet(n_filter=4, dilation=(1, 2, 1, 1, 2))
    assert d.conv1_0.conv1.dilation == (2, 2) and d.conv1_0.conv2.dilation == (2, 2) and d.conv4_0.conv2.padding == (2, 2)
    assert d.conv1_1.conv1.dilation == (1, 1)
    assert MO.MultiOutputNestedUNet is B.MultiOutputNestedUNet and MO.MultiOutputUnet is B.MultiOutputUnet
    assert MO.MultiOutputNestedUNet_3Levels is B.MultiOutputNestedUNet_3Levels


@pytest.mark.parametrize("cls", [B.MultiOutputUnet, B.MultiOutputNestedUNet, B.MultiOutputNestedUNet_3Levels])
def test_cpu_input_refused(cls):
    m = cls(1, HEADS, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.rand(1, 1, 32, 32))


# ------------------------------------------------------------------------------------------------------------------------------------
# the oracle against torch.nn modules in the reference's structure (what the reference forward computes)
# ------------------------------------------------------------------------------------------------------------------------------------
def _ref_nested_forward(m, x, levels, heads, ds, train_mode):
    """The reference's forward (multi_output_nested_unet.py:116-156), written as module calls on the HIP model's own containers."""
    up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)
    blk = lambda name, t: _run_vgg(getattr(m, name), t)
    X = {(0, 0): blk("conv0_0", x)}
    for k in range(1, levels + 1):
        X[(k, 0)] = blk(f"conv{k}_0", F.max_pool2d(X[(k - 1, 0)], 2, 2))
        for j in range(1, k + 1):
            r = k - j
            X[(r, j)] = blk(f"conv{r}_{j}", torch.cat([X[(r, i)] for i in range(j)] + [up(X[(r + 1, j - 1)])], 1))
    act = {"sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu}
    out = {}
    for name, cfg in heads.items():
        f = act.get(cfg.get("activation"), lambda t: t)
        if ds and train_mode:
            for l in range(1, levels + 1):
                out[f"{name}_{l}"] = f(m.output_layers[f"{name}_{l}"](X[(0, l)]))
            out[name] = out[f"{name}_{levels}"]
        else:
            out[name] = f(m.output_layers[f"{name}_{levels}" if ds else name](X[(0, levels)]))
    return out


def _run_vgg(b, t):
    t = F.leaky_relu(b.bn1(b.conv1(t)), 0.1)
    return F.leaky_relu(b.bn2(b.conv2(t)), 0.1)


@pytest.mark.parametrize("cls,levels,ds,dil", [(B.MultiOutputNestedUNet, 4, False, False), (B.MultiOutputNestedUNet, 4, True, (1, 2, 1, 1, 2)),
                                               (B.MultiOutputNestedUNet_3Levels, 3, True, (2, 1, 1, 1))])
def test_nested_oracle_matches_module_forward(cls, levels, ds, dil):
    """mo2d_oracle.nested_forward (the functional form the GPU tests compare against) equals the reference structure run with torch.nn
    modules in fp64: outputs, the trainer's deep-supervision loss, every gradient and the BatchNorm running statistics."""
    torch.manual_seed(0)
    m = cls(2, HEADS, 4, deep_supervision=ds, dilation=dil).double().train()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.rand(2, 2, 32, 48, dtype=torch.float64)
    tg = {n: torch.rand(2, c["channels"], 32, 48, dtype=torch.float64) for n, c in HEADS.items()}
    want = _ref_nested_forward(m, x, levels, HEADS, ds, True)
    wl = M.weighted_mse(want, tg, HEADS, deep_supervision=ds, levels=levels)
    wl.backward()
    from oracle import unet_oracle as O
    osd = O.clone_state(sd, requires_grad=True)
    got = M.nested_forward(osd, x, HEADS, levels=levels, deep_supervision=ds, dilation=dil)
    gl = M.weighted_mse(got, tg, HEADS, deep_supervision=ds, levels=levels)
    assert list(got) == list(want)
    for k in want:
        torch.testing.assert_close(got[k], want[k], rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(gl, wl, rtol=1e-10, atol=1e-12)
    grads = O.grads_of(gl, osd)
    for k, p in m.named_parameters():
        torch.testing.assert_close(grads[k], p.grad, rtol=1e-8, atol=1e-12, msg=lambda s, k=k: f"{k}: {s}")
    for k, v in m.state_dict().items():
        if "running_" in k:
            torch.testing.assert_close(osd[k], v, rtol=1e-10, atol=1e-12)


def test_mo2d_oracle_matches_module_forward():
    torch.manual_seed(1)
    m = B.MultiOutputUnet(1, HEADS, 4).double().train()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.rand(2, 1, 32, 48, dtype=torch.float64)

    def blk(s, t):
        return F.leaky_relu(s[1](s[0](t)), 0.1)
    e, skips, t = x, [], x
    for lvl in range(4):
        t = blk(getattr(m, f"encode{2 * lvl + 2}"), blk(getattr(m, f"encode{2 * lvl + 1}"), t))
        skips.append(t)
        t = F.max_pool2d(t, 2, 2)
    t = blk(m.middle_conv2, blk(m.middle_conv1, t))
    for lvl, skip in zip((1, 2, 3, 4), reversed(skips)):
        t = torch.cat([getattr(m, f"up{lvl}")(t), skip], 1)
        t = blk(getattr(m, f"decode{2 * lvl}"), blk(getattr(m, f"decode{2 * lvl - 1}"), t))
    act = {"sigmoid": torch.sigmoid, "tanh": torch.tanh}
    want = {n: act.get(c["activation"], lambda v: v)(m.output_layers[n](t)) for n, c in HEADS.items()}
    from oracle import unet_oracle as O
    got = M.mo2d_forward(O.clone_state(sd), x, HEADS)
    for k in want:
        torch.testing.assert_close(got[k], want[k], rtol=1e-10, atol=1e-12)
