"""Helper of test_gpu_narrow_end, run as a subprocess so that BIU_DISABLE / BIU_ROLL (read once per process) can differ between runs.

  step  OUT   one train-mode forward/backward of UNet3D(1, 1, 32) in bf16 with the 3-D trainer's loss (BCE/dice + time term); everything the
              step produces is dumped together with the number of calls per entry point (``lib.prof``)
  rank1 OUT   ``biu_head_bwd_bnred`` (dx = NULL) + ``biu_conv_bwd_weight_bn_rank1`` against ``biu_head_bwd_bnred`` +
              ``biu_conv_bwd_weight_bn`` on the same inputs of a 32 -> 16 block with a one-channel head; the raw results are dumped"""
import collections
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bio_image_unet_amd as B  # noqa: E402
from bio_image_unet_amd._lib import lib  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]


def step():
    from bio_image_unet_amd.losses import BCEDiceLoss
    from oracle import unet_oracle as O
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(11)
    m = B.UNet3D(1, 1, 32).cuda()
    m.load_state_dict(O.init_unet3d(1, 1, 32, seed=7))
    m.set_compute_dtype(torch.bfloat16)
    m.train()
    shape = (2, 1, 16, 16, 32)
    x = torch.rand(*shape, generator=g).cuda()
    y = (torch.rand(*shape, generator=g) > 0.5).float().cuda()
    lib.prof = []
    prob, logits = m(x)
    loss = BCEDiceLoss(0.5, 0.5)(logits, y, time_weight=0.1)
    loss.backward()
    torch.cuda.synchronize()
    calls = collections.Counter(name for name, _, _, _ in lib.prof)
    lib.prof = None
    return {"loss": loss.detach().cpu(), "prob": prob.detach().cpu(), "logits": logits.detach().cpu(), "calls": dict(calls),
            "buffers": {k: b.detach().cpu() for k, b in m.named_buffers()},
            "grads": {k: p.grad.cpu() for k, p in m.named_parameters()}}


def rank1():
    from tests.gpu_util import DT, XF, Dev, check, ptr, stream

    def rnd(*shape, seed=0):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))

    code = DT["bf16"][1]
    cin, c = 32, 16
    res = {}
    for name, n, sp, head_cout in (("1x16x16x32", 1, (16, 16, 32), 1), ("2x16x24x40", 2, (16, 24, 40), 1), ("cout2", 1, (16, 16, 32), 2)):
        x, xf = Dev(rnd(n, cin, *sp, seed=1), dtype="bf16"), XF(cin, seed=2)
        y, yxf = Dev(rnd(n, c, *sp, seed=3), dtype="bf16"), XF(c, seed=5)
        coef = [t.cuda() for t in (rnd(c, seed=6) * 0.3 + 1.0, rnd(c, seed=7) * 0.05, rnd(c, seed=8) * 0.05)]
        mean, invstd = (rnd(c, seed=9) * 0.1).cuda(), (rnd(c, seed=10).abs() + 0.5).cuda()
        dl = rnd(n, head_cout, *sp, seed=4).cuda().contiguous()
        wh = (rnd(head_cout, c, seed=12) * 0.3).cuda()
        wsz = max(lib.biu_conv_bwd_weight_workspace(cin, c, 3, 3, 3, code), lib.biu_head_bwd_workspace(c), 16)
        ws = torch.empty(wsz, dtype=torch.uint8, device="cuda")
        dy_new = Dev(shape=(n, c) + sp, dtype="bf16")
        ok = lib.biu_conv_bwd_weight_bn_rank1_ok(x.a(), dy_new.a(), y.a(), head_cout, 3, 3, 3, 1, code)
        dw_new = torch.full((c, cin, 3, 3, 3), float("nan"), device="cuda")
        rc = lib.biu_conv_bwd_weight_bn_rank1(x.a(), xf.x(), ptr(dl), ptr(wh), head_cout, dy_new.a(), y.a(), ptr(yxf.d[0]), ptr(yxf.d[1]),
                                              ptr(yxf.d[2]), ptr(coef[0]), ptr(coef[1]), ptr(coef[2]), 3, 3, 3, 1, ptr(dw_new), ptr(ws), wsz, code,
                                              stream())
        torch.cuda.synchronize()
        res[name] = {"ok": ok, "rc": rc, "dy_untouched": bool(torch.isnan(dy_new.buf.float()).all())}
        if head_cout != 1:
            continue
        # today's two calls: the head stores d loss / d a, the block's fused weight gradient loads it back and leaves dy in its place
        da = Dev(shape=(n, c) + sp, dtype="bf16")
        part = torch.zeros(1024 * c * 2, device="cuda")
        nb = C.c_int(0)
        dwh, dbh = torch.empty_like(wh), torch.empty(head_cout, device="cuda")
        check(lib.biu_head_bwd_bnred(y.a(), yxf.x(), ptr(wh), head_cout, ptr(dl), da.a(), ptr(dwh), ptr(dbh), ptr(ws), wsz, ptr(mean),
                                     ptr(invstd), ptr(part), part.numel(), C.byref(nb), code, stream()), "head_bwd_bnred")
        dw_old = torch.full((c, cin, 3, 3, 3), float("nan"), device="cuda")
        check(lib.biu_conv_bwd_weight_bn(x.a(), xf.x(), da.a(), y.a(), ptr(yxf.d[0]), ptr(yxf.d[1]), ptr(yxf.d[2]), ptr(coef[0]), ptr(coef[1]),
                                         ptr(coef[2]), 3, 3, 3, 1, ptr(dw_old), ptr(ws), wsz, code, stream()), "conv_bwd_weight_bn")
        torch.cuda.synchronize()
        res[name].update(dy_old=da.buf.cpu(), dy_new=dy_new.buf.cpu(), dw_old=dw_old.cpu(), dw_new=dw_new.cpu())
    return res


torch.save(step() if mode == "step" else rank1(), out)
