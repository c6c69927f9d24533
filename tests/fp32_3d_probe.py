"""Helper of test_gpu_fp32_products_3d: every fp32 3-D matrix-core op once, seeded, on shapes of the 3-D cases of test_gpu_ops.py, with
its float64 CPU reference and the float64 sum of |products| (the same op on |operands|).  Run as a subprocess: BIU_FP32_PRODUCTS_3D is read
once per process.  Writes {op: (got, ref, absref)} to argv[1]."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tests.gpu_util import DT, XF, Dev, check, lib, ptr, stream  # noqa: E402

code = DT["f32"][1]
out = {}


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def conv3(x, w, b=None):
    return F.conv3d(x, w, b, padding=1)


# ---- 3x3x3 convolution: forward, data gradient, weight gradient.  (3, 1, 48, 48, (5, 7, 9)) of MFMA_CASES, and decode1 of an n_filter = 64
# network (768 -> 64 channels) on a small volume
for tag, n, cin, cout, sp in [("c48", 1, 48, 48, (5, 7, 9)), ("c768", 1, 768, 64, (2, 4, 16))]:
    x = rnd(n, cin, *sp, seed=1)
    w = rnd(cout, cin, 3, 3, 3, seed=2) * (1.0 / (cin * 27) ** 0.5)
    b = rnd(cout, seed=3)
    xf = XF(cin, seed=4)
    xd = Dev(x, pitch=cin + 16, c0=8)
    xa = xf.apply(xd.ref()).double()
    wd, bd = w.cuda(), b.cuda()
    pk = torch.empty(lib.biu_conv_packed_bytes(0, cin, cout, 3, 3, 3, 1, code), dtype=torch.uint8, device="cuda")
    check(lib.biu_conv_pack(0, ptr(wd), cin, cout, 3, 3, 3, code, ptr(pk), stream()), "conv_pack")
    yd = Dev(shape=(n, cout, *sp))
    check(lib.biu_conv_fwd(xd.a(), xf.x(), ptr(wd), ptr(pk), ptr(bd), 3, 3, 3, 1, yd.a(), None, 0, code, stream()), "conv_fwd")
    out[f"conv_fwd_{tag}"] = (yd.get(), conv3(xa, w.double(), b.double()), conv3(xa.abs(), w.double().abs()))
    dyd = Dev(rnd(n, cout, *sp, seed=5))
    dy = dyd.ref().double()
    pk2 = torch.empty(lib.biu_conv_packed_bytes(1, cin, cout, 3, 3, 3, 1, code), dtype=torch.uint8, device="cuda")
    check(lib.biu_conv_pack(1, ptr(wd), cin, cout, 3, 3, 3, code, ptr(pk2), stream()), "conv_pack(dgrad)")
    dxd = Dev(shape=(n, cin, *sp))
    check(lib.biu_conv_bwd_data(dyd.a(), ptr(wd), ptr(pk2), 3, 3, 3, 1, dxd.a(), 0, None, 0, code, stream()), "conv_bwd_data")
    dgrad = lambda g, ww: torch.nn.grad.conv3d_input(xa.shape, ww, g, padding=1)  # noqa: E731
    out[f"conv_dgrad_{tag}"] = (dxd.get(), dgrad(dy, w.double()), dgrad(dy.abs(), w.double().abs()))
    ws = torch.empty(lib.biu_conv_bwd_weight_workspace(cin, cout, 3, 3, 3, code), dtype=torch.uint8, device="cuda")
    dw, db = torch.full_like(wd, float("nan")), torch.empty_like(bd)
    check(lib.biu_conv_bwd_weight(xd.a(), xf.x(), dyd.a(), 3, 3, 3, 1, ptr(dw), ptr(db), ptr(ws), ws.numel(), code, stream()), "conv_bwd_weight")
    wgrad = lambda a_, g: torch.nn.grad.conv3d_weight(a_, w.shape, g, padding=1)  # noqa: E731
    out[f"conv_wgrad_{tag}"] = (dw.cpu(), wgrad(xa, dy), wgrad(xa.abs(), dy.abs()))

# ---- ConvTranspose3d k2 s2: forward, data gradient, weight gradient  ((3, 1, 64, 64, (4, 8, 16)) of CONVT_MFMA_CASES)
n, cin, cout, sp = 1, 64, 64, (4, 8, 16)
x = rnd(n, cin, *sp, seed=1)
w = rnd(cin, cout, 2, 2, 2, seed=2) * (1.0 / cin ** 0.5)
b = rnd(cout, seed=3)
xf = XF(cin, seed=4)
xd = Dev(x, pitch=cin + 8, c0=8)
xa = xf.apply(xd.ref()).double()
wd, bd = w.cuda(), b.cuda()
hi = tuple(2 * s for s in sp)
pk = torch.empty(lib.biu_convt_packed_bytes(0, cin, cout, 2, code), dtype=torch.uint8, device="cuda")
check(lib.biu_convt_pack(0, ptr(wd), cin, cout, 2, code, ptr(pk), stream()), "convt_pack")
yd = Dev(shape=(n, cout, *hi))
check(lib.biu_convt_fwd(xd.a(), xf.x(), ptr(wd), ptr(pk), ptr(bd), 2, yd.a(), code, stream()), "convt_fwd")
ct = lambda a_, ww, bb=None: F.conv_transpose3d(a_, ww, bb, stride=2)  # noqa: E731
out["convt_fwd"] = (yd.get(), ct(xa, w.double(), b.double()), ct(xa.abs(), w.double().abs()))
gd = Dev(rnd(n, cout, *hi, seed=5))
g = gd.ref().double()
pk1 = torch.empty(lib.biu_convt_packed_bytes(1, cin, cout, 2, code), dtype=torch.uint8, device="cuda")
check(lib.biu_convt_pack(1, ptr(wd), cin, cout, 2, code, ptr(pk1), stream()), "convt_pack(dgrad)")
dxd = Dev(shape=(n, cin, *sp))
check(lib.biu_convt_bwd_data(gd.a(), ptr(wd), ptr(pk1), 2, dxd.a(), 0, code, stream()), "convt_bwd_data")
out["convt_dgrad"] = (dxd.get(), F.conv3d(g, w.double(), stride=2), F.conv3d(g.abs(), w.double().abs(), stride=2))
ws = torch.empty(lib.biu_convt_bwd_weight_workspace(cin, cout, 2, code), dtype=torch.uint8, device="cuda")
dw, db = torch.full_like(wd, float("nan")), torch.empty_like(bd)
check(lib.biu_convt_bwd_weight(xd.a(), xf.x(), gd.a(), 2, ptr(dw), ptr(db), ptr(ws), ws.numel(), code, stream()), "convt_bwd_weight")
ctw = lambda a_, gg: torch.nn.grad.conv3d_weight(gg, (cin, cout, 2, 2, 2), a_, stride=2)  # noqa: E731   (dW[ci][co][k] = sum_v x[v][ci] g[2v+k][co])
out["convt_wgrad"] = (dw.cpu(), ctw(xa, g), ctw(xa.abs(), g.abs()))

# ---- nearest up-sampling folded into the 3x3x3 conv: forward, data gradient, weight gradient  ((1, 32, 32, (4, 8, 16)) of UPCONV_CASES)
n, cin, cout, sp = 1, 32, 32, (4, 8, 16)
x = rnd(n, cin, *sp, seed=1)
w = rnd(cout, cin, 3, 3, 3, seed=2) * (1.0 / (cin * 27) ** 0.5)
b = rnd(cout, seed=3)
xf = XF(cin, seed=4)
xd = Dev(x, pitch=cin + 16, c0=8)
xa = xf.apply(xd.ref()).double()
up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
hi = tuple(2 * s for s in sp)
wd, bd = w.cuda(), b.cuda()
yd = Dev(shape=(n, cout, *hi))
pk = torch.empty(lib.biu_upconv_packed_bytes(0, cin, cout, code), dtype=torch.uint8, device="cuda")
check(lib.biu_upconv_pack(0, ptr(wd), cin, cout, code, ptr(pk), stream()), "upconv_pack")
nfl = lib.biu_upconv_fwd_stats_floats(xd.a(), yd.a())
part = torch.empty(nfl, device="cuda")
nblk = C.c_int(0)
check(lib.biu_upconv_fwd(xd.a(), xf.x(), ptr(pk), ptr(bd), yd.a(), ptr(part), nfl, C.byref(nblk), code, stream()), "upconv_fwd")
# (the folded weights sum up to 8 fine taps: |W'| <= the sum of |w| over them, so the |.| reference of the unfolded op bounds the folded one)
out["upconv_fwd"] = (yd.get(), conv3(up(xa), w.double(), b.double()), conv3(up(xa.abs()), w.double().abs()))
gd = Dev(rnd(n, cout, *hi, seed=5))
g = gd.ref().double()
pk1 = torch.empty(lib.biu_upconv_packed_bytes(1, cin, cout, code), dtype=torch.uint8, device="cuda")
check(lib.biu_upconv_pack(1, ptr(wd), cin, cout, code, ptr(pk1), stream()), "upconv_pack(dgrad)")
dxd = Dev(shape=(n, cin, *sp))
check(lib.biu_upconv_bwd_data(gd.a(), ptr(pk1), dxd.a(), 0, code, stream()), "upconv_bwd_data")
down = lambda t: F.avg_pool3d(t, 2) * 8  # noqa: E731   (adjoint of nearest up-sampling)
dgu = lambda gg, ww: down(torch.nn.grad.conv3d_input((n, cin, *hi), ww, gg, padding=1))  # noqa: E731
out["upconv_dgrad"] = (dxd.get(), dgu(g, w.double()), dgu(g.abs(), w.double().abs()))
ws = torch.empty(lib.biu_upconv_bwd_weight_workspace(cin, cout, code), dtype=torch.uint8, device="cuda")
dw = torch.full_like(wd, float("nan"))
check(lib.biu_upconv_bwd_weight_bn(xd.a(), xf.x(), gd.a(), None, None, None, None, None, None, None, ptr(dw), ptr(ws), ws.numel(), code, stream()),
      "upconv_bwd_weight")
wgu = lambda a_, gg: torch.nn.grad.conv3d_weight(up(a_), w.shape, gg, padding=1)  # noqa: E731
out["upconv_wgrad"] = (dw.cpu(), wgu(xa, g), wgu(xa.abs(), g.abs()))

torch.cuda.synchronize()
torch.save({k: tuple(t.detach().cpu() for t in v) for k, v in out.items()}, sys.argv[1])
