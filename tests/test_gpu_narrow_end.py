"""The 16-channel end of a step without its dead traffic: a one-channel head that does not store its data gradient
(``biu_head_bwd_bnred`` with dx = NULL), the trunk's weight gradient that rebuilds it in its loader (``biu_conv_bwd_weight_bn_rank1``), and a
train step that takes this path against one that has it switched off (BIU_DISABLE=headrank1).  Each new entry point is compared with the
calls it replaces on the same inputs, through the C ABI."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DT, XF, Dev, check, lib, ptr, stream  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------
# 1. one-channel head backward without its data gradient
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, (8, 8, 32)), (1, (10, 24, 40))], ids=["2x8x8x32", "1x10x24x40"])
def test_head_bwd_bnred_without_dx_gives_the_same_sums(case):
    """C = 16, cout = 1, bf16: dw, dbias, the number of partial rows and the rows themselves are, bit for bit, those of the call that stores
    dx (the BatchNorm-backward sums are taken from the value rounded to the storage type either way; no atomics anywhere)."""
    n, sp = case
    c, cout, code = 16, 1, DT["bf16"][1]
    xf = XF(c, seed=3)
    xd = Dev(rnd(n, c, *sp, seed=1), dtype="bf16")
    w = (rnd(cout, c, seed=2) * 0.3).cuda()
    dl = rnd(n, cout, *sp, seed=4).cuda().contiguous()
    mean, invstd = (rnd(c, seed=8) * 0.1).cuda(), (rnd(c, seed=9).abs() + 0.5).cuda()
    wsz = lib.biu_head_bwd_workspace(c)
    ws = torch.empty(wsz, dtype=torch.uint8, device="cuda")
    nfl = 1024 * c * 2
    got = []
    for store in (True, False):
        dx = Dev(shape=(n, c) + sp, dtype="bf16")
        dw, db = torch.full_like(w, float("nan")), torch.full((cout,), float("nan"), device="cuda")
        part, nb = torch.full((nfl,), float("nan"), device="cuda"), C.c_int(0)
        check(lib.biu_head_bwd_bnred(xd.a(), xf.x(), ptr(w), cout, ptr(dl), dx.a() if store else None, ptr(dw), ptr(db), ptr(ws), wsz,
                                     ptr(mean), ptr(invstd), ptr(part), nfl, C.byref(nb), code, stream()), "head_bwd_bnred")
        got.append((dw.cpu(), db.cpu(), nb.value, part[:nb.value * c * 2].cpu(), dx.buf.float().cpu()))
    (dw_a, db_a, nb_a, part_a, dx_a), (dw_b, db_b, nb_b, part_b, _) = got
    assert nb_a == nb_b and nb_a >= 1 and bool(torch.isfinite(part_a).all()) and bool(torch.isfinite(dx_a).all())
    assert float(dw_a.abs().max()) > 0 and float(part_a.abs().max()) > 0
    assert torch.equal(dw_b.view(torch.int32), dw_a.view(torch.int32)) and torch.equal(db_b.view(torch.int32), db_a.view(torch.int32))
    assert torch.equal(part_b.view(torch.int32), part_a.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------
# 2. weight gradient that rebuilds the head's rank-one data gradient in its loader
# ---------------------------------------------------------------------------------------------------------------
def _probe(mode, tmp_path, tag, env_extra):
    out = str(tmp_path / f"{mode}_{tag}.pt")
    env = dict(os.environ)
    env.pop("BIU_DISABLE", None)
    env.update(env_extra)
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "narrow_end_probe.py"), mode, out], check=True, env=env, timeout=300)
    return torch.load(out)


def test_rank1_weight_gradient_matches_head_plus_fused_weight_gradient(tmp_path):
    """32 -> 16 block, bf16, under BIU_ROLL=always (read once per process: tests/narrow_end_probe.py): 1 x 16x16x32, the smallest shape the
    rolling form takes, and 2 x 16x24x40 with ragged windows in H and W.  dy is bit for bit what biu_head_bwd_bnred +
    biu_conv_bwd_weight_bn leave in the gradient buffer; dW agrees to 1e-6 of its largest entry (the kernels flush with float atomics,
    whose order differs from run to run).  A two-channel head is refused: the predicate says 0 and the call returns BIU_ERR_UNSUPPORTED
    without touching dy."""
    r = _probe("rank1", tmp_path, "roll", {"BIU_ROLL": "always"})
    bad = r["cout2"]
    assert bad["ok"] == 0 and bad["rc"] == -2 and bad["dy_untouched"]
    for name in ("1x16x16x32", "2x16x24x40"):
        c = r[name]
        assert c["ok"] == 1 and c["rc"] == 0, name
        assert bool(torch.isfinite(c["dy_old"].float()).all()) and float(c["dy_old"].float().abs().max()) > 0
        same = torch.equal(c["dy_new"].view(torch.int16), c["dy_old"].view(torch.int16))
        scale = float(c["dw_old"].abs().max())
        d = float((c["dw_new"] - c["dw_old"]).abs().max()) / scale
        print(f"rank-one weight gradient {name}: dy identical {same}, dW differs by {d:.3e} of its scale (bound 1e-6)")
        assert same, name
        assert bool(torch.isfinite(c["dw_new"]).all()) and d <= 1e-6, name


# ---------------------------------------------------------------------------------------------------------------
# 3. a train step with the new path against one with it switched off
# ---------------------------------------------------------------------------------------------------------------
TOKENS = "headrank1"
NEW_CALLS = ("biu_conv_bwd_weight_bn_rank1",)


def _step(disable, tmp_path):
    # at this extent every 3-D block would hand its weight gradient to the side stream (a size rule); 0 keeps the blocks on the calls a
    # full-size volume takes, the fused weight gradient of the last block among them.  Both sides alike.
    env = {"BIU_SIDE_WGRAD_VOX": "0"}
    if disable:
        env["BIU_DISABLE"] = disable
    return _probe("step", tmp_path, "off" if disable else "on", env)


def test_step_with_the_narrow_end_paths_matches_the_step_without(tmp_path):
    """UNet3D(1, 1, 32) bf16, (2, 1, 16, 16, 32), BCEDiceLoss(0.5, 0.5) with time_weight 0.1.  The new path changes no stored value the step
    reads later: loss, outputs and BatchNorm buffers are equal; parameter gradients agree to 1e-5 of each tensor's largest entry (the order
    of the float atomics inside the weight-gradient kernels differs from run to run by that much: bench.py's docstring)."""
    on, off = _step(None, tmp_path), _step(TOKENS, tmp_path)
    for name in NEW_CALLS:
        assert on["calls"].get(name, 0) >= 1, f"{name} did not run with the path on: {sorted(on['calls'])}"
        assert off["calls"].get(name, 0) == 0, f"{name} ran although switched off"
    assert on["calls"].get("biu_conv_bwd_weight_bn", 0) == off["calls"].get("biu_conv_bwd_weight_bn", 0) - 1      # decode6 alone changed its call
    for side in (on, off):
        assert side["calls"].get("biu_head_dlogits", 0) == 0      # the unused `prob` output gets no zero gradient: d logits is used as it is
    assert torch.equal(on["loss"], off["loss"]) and bool(torch.isfinite(on["loss"]))
    assert torch.equal(on["prob"], off["prob"]) and torch.equal(on["logits"], off["logits"])
    assert on["buffers"].keys() == off["buffers"].keys()
    for k in on["buffers"]:
        assert torch.equal(on["buffers"][k], off["buffers"][k]), k
    worst = 0.0
    for k, g_off in off["grads"].items():
        scale = float(g_off.abs().max())
        d = float((on["grads"][k] - g_off).abs().max()) / (scale + 1e-30)
        worst = max(worst, d)
        assert scale > 0 or k.endswith("bias"), k
        assert d <= 1e-5, f"{k}: gradients differ by {d:.3e} of the tensor's scale"
    print(f"narrow-end step: worst parameter-gradient difference {worst:.3e} of its tensor's scale (bound 1e-5)")
