"""First-layer kernels with 2 to 4 input channels through the C ABI (csrc/biu_c1.hip on the matrix cores for bf16, csrc/biu_special.hip
on the vector ALUs for fp32), against float64 references that share no kernel with them.

Shapes sit at the edges of the bricks (16x32 forward / 8x32 weight gradient in 2-D, 2x8x32 / 1x8x32 in 3-D): one where no extent is a
multiple of a brick (W % 4 != 0 also takes the one-voxel fp32 forward), one where every extent is; 48 output channels are a 32-piece
plus a 16-piece, 8 and 24 are what the matrix-core form does not take (the 3-D networks open with n_filter / 2 = 8 at n_filter = 16).  The input is a channel slice of pitch Cin and Cin + 8, with and without a per-channel input transform.

Bounds.  A = conv(|T(x)|, |w|) + |b| is the sum of the magnitudes that enter an output element.
  bf16 forward: 2^-8 |want| (the store rounding, half an ulp, doubled) + 2^-15 A (fp32 accumulation of <= 109 terms plus the 2^-17
                residue of the two-term weight split).  A weight rounded once to bf16 (2^-9 per product) does not meet it: shown below.
  fp32 forward: 2^-20 A.
  statistics:   rel 2^-17, of the sum and of the sum of squares.  The bias of every output channel is drawn away from zero on the side of
                the channel's own mean (fwd_case), so that no channel's sum cancels and the relative bound means something.
  gradients:    the tolerances of run_conv_bwd_weight_bn(..., torch_ref=True) in tests/test_gpu_ops.py."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.gpu_util import DT, Dev, check, lib, ptr, stream  # noqa: E402
from tests.gpu_util import biu_xform  # noqa: E402
from tests.test_gpu_ops import run_conv_bwd_weight_bn, run_conv_fwd_stats_and_dgrad_bnred  # noqa: E402

SHAPES = {"2d-ragged": (2, (19, 37)), "2d-aligned": (1, (32, 64)), "3d-ragged": (2, (3, 10, 37)), "3d-aligned": (1, (4, 16, 64))}
WALK = (1, (96, 96, 96))                      # 1728 forward bricks: every block of the 3 x CU-count grid walks more than two
CINS, COUTS, DTYPES = [2, 3, 4], [16, 32, 48, 8, 24], ["bf16", "f32"]     # (8, 24: no multiple of 16, bf16 stays on the vector ALUs as well)
VARIANTS = [(pitch8, use_xf) for pitch8 in (False, True) for use_xf in (False, True)]


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def q(t, dtype):
    """t as the device stores it."""
    return t.bfloat16().float() if dtype == "bf16" else t.float()


class Xf:
    """Per-channel transform T(x) = lrelu(scale * x + shift, slope), negative scales included."""

    def __init__(self, c):
        self.scale = rnd(c, seed=41) * 0.5 + 1.0
        self.scale[::3] *= -1
        self.shift = rnd(c, seed=42) * 0.3
        self.slope = torch.full((c,), 0.1)
        self.d = [t.cuda() for t in (self.scale, self.shift, self.slope)]
        self.s = biu_xform(*[t.data_ptr() for t in self.d])

    def apply64(self, x):
        shp = (1, -1) + (1,) * (x.dim() - 2)
        t = x.double() * self.scale.double().view(shp) + self.shift.double().view(shp)
        return torch.where(t > 0, t, t * self.slope.double().view(shp))


def conv64(x, w, b, nd):
    return (F.conv3d if nd == 3 else F.conv2d)(x, w, b, padding=1)


def u5(t, nd):
    return t.unsqueeze(2) if nd == 2 else t


def s5(t, nd):
    return t.squeeze(2) if nd == 2 else t


@functools.lru_cache(maxsize=4)
def fwd_case(n, sp, cin, cout, dtype, use_xf):
    """Operands and the float64 references of one forward case, computed once and shared by the pitch variants: the stored input, T of it in
    float64, the fp32 weights, want, A, and what a kernel that rounded its weights once to bf16 would store."""
    nd = len(sp)
    x = q(rnd(n, cin, *sp, seed=1), dtype)
    w = rnd(cout, cin, *([3] * nd), seed=2)                                      # weights of O(1)
    xf = Xf(cin) if use_xf else None
    tx = xf.apply64(x) if use_xf else x.double()
    # bias of O(1) on the side of the channel's mean without it: |sum over the voxels| >= the voxel count, no cancellation in the statistics
    m0 = conv64(tx, w.double(), None, nd).transpose(0, 1).flatten(1).mean(1)
    b = (torch.where(m0 < 0, -1.0, 1.0) * (1.0 + rnd(cout, seed=3).abs().double())).float()
    want = conv64(tx, w.double(), b.double(), nd)
    A = conv64(tx.abs(), w.double().abs(), b.double().abs(), nd)
    once = conv64(tx, w.bfloat16().double(), b.double(), nd).float().bfloat16().double()
    return x, w, b, xf, u5(want, nd), u5(A, nd), u5(once, nd)


def fwd_bound(want, A, dtype):
    return 2.0 ** -8 * want.abs() + 2.0 ** -15 * A if dtype == "bf16" else 2.0 ** -20 * A


def run_fwd(n, sp, cin, cout, dtype, pitch8, use_xf):
    nd, code = len(sp), DT[dtype][1]
    kd = 3 if nd == 3 else 1
    x, w, b, xf, want, A, _ = fwd_case(n, sp, cin, cout, dtype, use_xf)
    xd = Dev(x, dtype=dtype, pitch=cin + 8 if pitch8 else cin)
    wd, bd = w.cuda(), b.cuda()
    rows = []
    for rep in range(2):
        yd = Dev(shape=tuple(want.shape), dtype=dtype)
        assert lib.biu_conv_first_ok(xd.a(), yd.a(), kd, 3, 3, 1, code) == 1
        nfl = lib.biu_conv_fwd_stats_floats(yd.a(), kd)
        part = torch.full((nfl,), float("nan"), device="cuda")
        nblk = C.c_int(0)
        check(lib.biu_conv_fwd_stats(xd.a(), C.byref(xf.s) if use_xf else None, ptr(wd), None, ptr(bd), kd, 3, 3, 1, yd.a(), ptr(part), nfl,
                                     C.byref(nblk), None, 0, code, stream()), "conv_fwd_stats")
        assert nblk.value > 0
        rows.append((yd.buf.clone(), part[:nblk.value * cout * 2].clone()))
    got = yd.get().double()
    dev = ((got - want).abs() / fwd_bound(want, A, dtype)).max()
    print(f"fwd {sp} cin {cin} cout {cout} {dtype} pitch8 {pitch8} xf {use_xf}: worst {float(dev):.3f} x bound, {nblk.value} statistics rows")
    assert torch.isfinite(got).all() and float(dev) <= 1.0
    # statistics of the values as stored
    sums = rows[1][1].view(nblk.value, cout, 2).double().sum(0).cpu()
    red = (0, 2, 3, 4)
    s1, s2 = got.sum(dim=red), (got * got).sum(dim=red)
    d1, d2 = ((sums[:, 0] - s1).abs() / s1.abs()).max(), ((sums[:, 1] - s2).abs() / s2).max()
    print(f"    statistics: sum {float(d1) * 2 ** 17:.3f}, sum of squares {float(d2) * 2 ** 17:.3f} (x 2^-17)")
    assert float(d1) <= 2.0 ** -17 and float(d2) <= 2.0 ** -17
    assert torch.equal(rows[0][0], rows[1][0]) and torch.equal(rows[0][1], rows[1][1]), "two launches differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_and_statistics(shape, cin, cout, dtype):
    n, sp = SHAPES[shape]
    for pitch8, use_xf in VARIANTS:
        run_fwd(n, sp, cin, cout, dtype, pitch8, use_xf)


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_bf16_bound_tells_split_weights_from_weights_rounded_once(shape, cin, cout):
    """The same bound, applied to the output of a float64 convolution with bf16-rounded weights (stored in bf16): violated."""
    n, sp = SHAPES[shape]
    _, _, _, _, want, A, once = fwd_case(n, sp, cin, cout, "bf16", False)
    dev = ((once - want).abs() / fwd_bound(want, A, "bf16")).max()
    assert float(dev) > 1.0, f"weights rounded once stay within the bound ({float(dev):.3f}x): it cannot tell the split from them"


def run_wgrad(n, sp, cin, cout, dtype, pitch8, use_xf):
    nd, code = len(sp), DT[dtype][1]
    kd = 3 if nd == 3 else 1
    osp = (1, *sp) if nd == 2 else sp
    xf = Xf(cin) if use_xf else None
    xd = Dev(rnd(n, cin, *sp, seed=1), dtype=dtype, pitch=cin + 8 if pitch8 else cin)
    xa = q(xf.apply64(xd.ref()).float(), dtype).double() if use_xf else xd.ref().double()     # T(x) as staged
    xfp = C.byref(xf.s) if use_xf else None
    wshape = (cout, cin) + (3,) * nd
    wzero = torch.zeros(wshape, dtype=torch.float64)
    wsz = lib.biu_conv_first_workspace(cin, cout, kd, code)
    assert wsz > 0 and lib.biu_conv_bwd_weight_workspace(cin, cout, kd, 3, 3, code) == 0
    ws = torch.empty(wsz, dtype=torch.uint8, device="cuda")

    def torch_dw(dy):
        return torch.ops.aten.convolution_backward(s5(dy.double(), nd), s5(xa, nd), wzero, None, [1] * nd, [1] * nd, [1] * nd, False, [0] * nd, 1,
                                                   [False, True, False])[1]

    def close(got, ref, what, rtol, atol):
        err = ((got.double() - ref).abs() / (atol + rtol * ref.abs())).max()
        print(f"    {what}: worst {float(err):.4f} x tolerance")
        assert torch.isfinite(got).all() and float(err) <= 1.0, what

    print(f"wgrad {sp} cin {cin} cout {cout} {dtype} pitch8 {pitch8} xf {use_xf}")
    # plain call (+ dbias)
    dyd = Dev(rnd(n, cout, *osp, seed=5), dtype=dtype)
    dws = []
    for rep in range(2):
        dw, db = torch.full(wshape, float("nan"), device="cuda"), torch.full((cout,), float("nan"), device="cuda")
        check(lib.biu_conv_bwd_weight(xd.a(), xfp, dyd.a(), kd, 3, 3, 1, ptr(dw), ptr(db), ptr(ws), ws.numel(), code, stream()), "conv_bwd_weight")
        dws.append(dw)
    gw = torch_dw(dyd.get())
    tw = (1e-3, 2e-4) if dtype == "f32" else (1e-2, 1e-2)
    close(dw.cpu(), gw, "dw (plain)", tw[0], tw[1] * float(gw.abs().max()))
    gb = dyd.get().double().sum(dim=(0, 2, 3, 4))
    close(db.cpu(), gb, "dbias", tw[0], tw[1] * float(gb.abs().max()))
    assert torch.equal(dws[0], dws[1]), "two launches of the plain weight gradient differ"
    # fused call: da -> dy in place (formula of biu_bn_bwd_apply on the stored operands), dw of the dy it stored
    yd = Dev(rnd(n, cout, *osp, seed=3), dtype=dtype)
    da0 = rnd(n, cout, *osp, seed=4)
    sc, sh, sl = rnd(cout, seed=51) * 0.5 + 1.0, rnd(cout, seed=52) * 0.3, torch.full((cout,), 0.1)
    sc[::3] *= -1
    cA, cB, cC = rnd(cout, seed=6) * 0.3 + 1.0, rnd(cout, seed=7) * 0.05, rnd(cout, seed=8) * 0.05
    dv = [t.cuda() for t in (sc, sh, sl, cA, cB, cC)]
    dws = []
    for rep in range(2):
        da = Dev(da0, dtype=dtype)
        dw = torch.full(wshape, float("nan"), device="cuda")
        check(lib.biu_conv_bwd_weight_bn(xd.a(), xfp, da.a(), yd.a(), *[ptr(t) for t in dv], kd, 3, 3, 1, ptr(dw), ptr(ws), ws.numel(), code, stream()),
              "conv_bwd_weight_bn")
        dws.append((dw, da.buf.clone()))
    v = (1, -1, 1, 1, 1)
    yr, dar = yd.ref().double(), Dev(da0, dtype=dtype).ref().double()
    tt = sc.double().view(v) * yr + sh.double().view(v)
    dy_ref = cA.double().view(v) * dar * torch.where(tt > 0, torch.ones_like(tt), sl.double().view(v).expand_as(tt)) + cB.double().view(v) * yr + cC.double().view(v)
    t = (1e-5, 1e-5) if dtype == "f32" else (2e-2, 2e-2)
    close(da.get(), dy_ref, "da -> dy (formula)", *t)
    gw = torch_dw(da.get())
    tw = (2e-4, 2e-4) if dtype == "f32" else (2e-2, 2e-2)
    close(dw.cpu(), gw, "dw (fused)", tw[0], tw[1] * float(gw.abs().max()))
    assert torch.equal(dws[0][0], dws[1][0]) and torch.equal(dws[0][1], dws[1][1]), "two launches of the fused weight gradient differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_weight_gradients(shape, cin, cout, dtype):
    n, sp = SHAPES[shape]
    for pitch8, use_xf in VARIANTS:
        run_wgrad(n, sp, cin, cout, dtype, pitch8, use_xf)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_second_opinion_of_the_per_kernel_suite(shape, cin, dtype, monkeypatch):
    """The bodies of tests/test_gpu_ops.py with 2 to 4 input channels: the forward with statistics and the plain forward, and the fused weight
    gradient against the separate pass and torch.  That helper sizes its scratch with biu_conv_bwd_weight_workspace alone (0 here), so as
    it stands its weight gradients are those of a caller that did not ask biu_conv_first_workspace: the any-shape kernels, which must stay
    right.  Run again with the query answering as a caller that asks both, the same body reaches the first-layer weight gradients."""
    n, sp = SHAPES[shape]
    run_conv_fwd_stats_and_dgrad_bnred((n, cin, 16, sp), dtype, parts=("fwd",))
    run_conv_bwd_weight_bn((len(sp), n, cin, 16, sp), dtype, torch_ref=True, reps=1)
    old = lib.biu_conv_bwd_weight_workspace
    asked = []

    def both(ci, co, kd, kh, kw, code):
        asked.append(lib.biu_conv_first_workspace(ci, co, kd, code))
        return max(old(ci, co, kd, kh, kw, code), asked[-1])

    monkeypatch.setattr(lib, "biu_conv_bwd_weight_workspace", both, raising=False)
    run_conv_bwd_weight_bn((len(sp), n, cin, 16, sp), dtype, torch_ref=True)
    assert asked and min(asked) > 0


@pytest.mark.parametrize("kernel", ["forward", "weight gradients"])
def test_a_block_walks_more_than_two_bricks(kernel):
    n, sp = WALK
    if kernel == "forward":
        run_fwd(n, sp, 2, 16, "bf16", False, False)
    else:
        run_wgrad(n, sp, 2, 16, "bf16", False, False)
