"""Helper of test_gpu_fp32_product_probes.  Run as a subprocess (the fp32 product modes are process-wide and latched on first use) with
BIU_FP32_PRODUCTS and BIU_FP32_PRODUCTS_3D set to the same mode; writes {"probe": ..., "dense": ..., "stats": ..., "aux": ...} to argv[1]
and prints one line per probed op.

1. Single-product probes.  One operand of every launch is one-hot, the other dense, the transform the identity and the bias zero, so every
   output element is exactly ONE product of two fp32 values or exactly zero: the stored fp32 result is the kernel's product itself (all other
   contributions are exact zeros, so accumulation order, split-K atomics and the input-channel split's reduce add nothing).  Values are
   full-mantissa fp32 in [0.25, 4) (tests/fp32_split.operands); the reference is the float64 product (exact).  The non-zero positions move over
   NSETS weight sets so that every tap, every position inside a 16-channel chunk, two or more chunks and every 32-channel output tile carry
   products; the record counts them.
2. Dense float64 bounds of the 2-D launches, as tests/fp32_3d_probe.py has them for 3-D: a real transform, pitched channel slices, a bias;
   (got, float64 reference, float64 sum of |products|) per launch."""
import ctypes as C
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tests.fp32_split import operands  # noqa: E402
from tests.gpu_util import DT, XF, Dev, check, lib, ptr, stream  # noqa: E402

code = DT["f32"][1]
NSETS = 3
probe, dense, stats, aux = {}, {}, {}, {}


def u8(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")


def shape5(n, c, sp):
    return (n, c, 1, *sp) if len(sp) == 2 else (n, c, *sp)


def pack_conv(kind, wd, cin, cout, kd):
    nb = lib.biu_conv_packed_bytes(kind, cin, cout, kd, 3, 3, 1, code)
    assert nb > 0, f"conv {cin} -> {cout} kd {kd}: not served by the matrix-core kernels"
    pk = u8(nb)
    check(lib.biu_conv_pack(kind, ptr(wd), cin, cout, kd, 3, 3, code, ptr(pk), stream()), "conv_pack")
    return pk


def pack_convt(kind, wd, cin, cout, kd):
    nb = lib.biu_convt_packed_bytes(kind, cin, cout, kd, code)
    assert nb > 0, f"convt {cin} -> {cout} kd {kd}: not served by the matrix-core kernels"
    pk = u8(nb)
    check(lib.biu_convt_pack(kind, ptr(wd), cin, cout, kd, code, ptr(pk), stream()), "convt_pack")
    return pk


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. single-product probes
# ----------------------------------------------------------------------------------------------------------------------------------------
def picks(rows, K, T, s):
    """Reduction channel and tap of the one non-zero weight of each of `rows` one-hot rows in weight set s.  7 is odd and prime to every K
    used: 16 consecutive rows cover the 16 positions of a chunk, 9 (27) consecutive rows every tap."""
    j = torch.arange(rows) + s * rows
    return (7 * j + s) % K, j % T


def voxels(c, nvox, s):
    """Flat voxel (within the batch) of the one non-zero value of each of c channels in set s."""
    j = torch.arange(c) + s * c
    return (11 * j + 5 * s) % nvox


def record(name, got, ref, eligible, ch_dims=(1,), taps=None, red=None, rows_alive=None, extra=None):
    """Fold one launch (one weight set) into the record of op `name`.  got: fp32 CPU; ref: float64, exactly one product or zero.  ch_dims: the
    dimensions of `got` that kernels tile by 32 channels (the output channels; both channel dimensions of a weight gradient)."""
    r = probe.setdefault(name, dict(worst=0.0, median=[], products=0, zeros=0, zeros_bad=0, negzero=0, nonfinite=0, eligible=eligible, sha=hashlib.sha256(),
                                    taps=set(), pos=set(), chunks=set(), tiles=set(), ntiles=0, launches=0, extra_ok=True))
    nz = ref != 0
    bad = (got != 0) & ~nz                                   # (a NaN left in the buffer counts: NaN != 0)
    r["nonfinite"] += int((~torch.isfinite(got)).sum())
    r["zeros"] += int((~nz).sum())
    r["zeros_bad"] += int(bad.sum())
    r["negzero"] += int((torch.signbit(got) & (got == 0) & ~nz).sum())
    e = ((got.double() - ref).abs() / ref.abs())[nz]
    e = torch.nan_to_num(e, nan=float("inf"))
    r["products"] += int(nz.sum())
    r["worst"] = max(r["worst"], float(e.max()))
    r["median"].append(float(e.median()))
    r["sha"].update(got.contiguous().numpy().tobytes())
    r["launches"] += 1
    r["ntiles"] = 0
    alive = None
    for d in ch_dims:
        nch = got.shape[d]
        al = nz.movedim(d, 0).reshape(nch, -1).any(1)
        alive = al if alive is None else alive
        r["ntiles"] += (nch + 31) // 32
        r["tiles"] |= {(d, t) for t in (torch.nonzero(al).flatten() // 32).tolist()}
    if rows_alive is None:
        rows_alive = alive
    if taps is not None:
        r["taps"] |= set(taps[rows_alive].tolist())
    if red is not None:
        r["pos"] |= set((red[rows_alive] % 16).tolist())
        r["chunks"] |= set((red[rows_alive] // 16).tolist())
    if extra is not None:
        r["extra_ok"] = r["extra_ok"] and bool(extra)


def conv_nd(nd):
    return (F.conv2d, torch.nn.grad.conv2d_input, torch.nn.grad.conv2d_weight) if nd == 2 else (F.conv3d, torch.nn.grad.conv3d_input, torch.nn.grad.conv3d_weight)


def onehot_x(n, c, sp, s, seed):
    """(n, c, *sp) zero but for one voxel per channel; returns it and the flat voxel index per channel."""
    nv = n * math.prod(sp)
    v = voxels(c, nv, s)
    x = torch.zeros(nv, c)
    x[v, torch.arange(c)] = operands(c, seed=seed)
    return x.view(n, *sp, c).movedim(-1, 1).contiguous(), v


def probe_conv(tag, nd, n, cin, cout, sp, *, split_ws=False, variants=True):
    """3x3(x3) convolution cin -> cout: forward, data gradient and weight gradient (and, variants: _fwd_stats, _bnred, _bn)."""
    kd, T = (1, 9) if nd == 2 else (3, 27)
    conv, conv_in, conv_w = conv_nd(nd)
    sq = nd == 2
    el = lambda K: K >= 16 and K % 16 == 0          # noqa: E731   (biu.h: launches with < 16 or a non-multiple of 16 reduction channels stay exact)
    zb = torch.zeros(cout, device="cuda")
    for s in range(NSETS):
        seed = 1000 * s + 17
        # ---- forward: w[co] non-zero at one (ci, tap)
        x = operands(n, cin, *sp, seed=seed + 1)
        xd = Dev(x)
        ci, tap = picks(cout, cin, T, s)
        w = torch.zeros(cout, cin, T)
        w[torch.arange(cout), ci, tap] = operands(cout, seed=seed + 2)
        w = w.view(cout, cin, *([3] * nd))
        wd = w.cuda()
        pk = pack_conv(0, wd, cin, cout, kd)
        ref = conv(x.double(), w.double(), padding=1)
        yd = Dev(shape=shape5(n, cout, sp))
        ws, need = None, 0
        if split_ws:
            need = lib.biu_conv_split_workspace(cin, yd.a(), None, kd, 3, 3, 1, code)
            assert need > 0, f"{tag}: this shape is meant to split over its input channels"
            ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
        check(lib.biu_conv_fwd(xd.a(), None, ptr(wd), ptr(pk), ptr(zb), kd, 3, 3, 1, yd.a(), ptr(ws), need, code, stream()), "conv_fwd")
        used = None if ws is None else not bool((ws == 0x5A).all())
        record(f"conv_fwd[{tag}]", yd.get(squeeze2d=sq), ref, el(cin), taps=tap, red=ci, extra=used)
        if variants:
            yd2 = Dev(shape=shape5(n, cout, sp))
            nfl = lib.biu_conv_fwd_stats_floats(yd2.a(), kd)
            part = torch.empty(nfl, device="cuda")
            nblk = C.c_int(0)
            check(lib.biu_conv_fwd_stats(xd.a(), None, ptr(wd), ptr(pk), ptr(zb), kd, 3, 3, 1, yd2.a(), ptr(part), nfl, C.byref(nblk), None, 0, code, stream()),
                  "conv_fwd_stats")
            record(f"conv_fwd_stats[{tag}]", yd2.get(squeeze2d=sq), ref, el(cin), taps=tap, red=ci)
        # ---- data gradient: w non-zero at one (co, tap) per ci
        dy = operands(n, cout, *sp, seed=seed + 3)
        dyd = Dev(dy)
        co, tap = picks(cin, cout, T, s)
        w = torch.zeros(cout, cin, T)
        w[co, torch.arange(cin), tap] = operands(cin, seed=seed + 4)
        w = w.view(cout, cin, *([3] * nd))
        wd = w.cuda()
        pk = pack_conv(1, wd, cin, cout, kd)
        ref = conv_in((n, cin, *sp), w.double(), dy.double(), padding=1)
        dxd = Dev(shape=shape5(n, cin, sp))
        ws, need = None, 0
        if split_ws:
            need = lib.biu_conv_split_workspace(cout, dxd.a(), None, kd, 3, 3, 1, code)
            assert need > 0, f"{tag}: the data gradient of this shape is meant to split"
            ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
        check(lib.biu_conv_bwd_data(dyd.a(), ptr(wd), ptr(pk), kd, 3, 3, 1, dxd.a(), 0, ptr(ws), need, code, stream()), "conv_bwd_data")
        used = None if ws is None else not bool((ws == 0x5A).all())
        record(f"conv_dgrad[{tag}]", dxd.get(squeeze2d=sq), ref, el(cout), taps=tap, red=co, extra=used)
        if variants:
            dxd2 = Dev(shape=shape5(n, cin, sp))
            yup = Dev(operands(n, cin, *sp, seed=seed + 5))
            one, zero = torch.ones(cin, device="cuda"), torch.zeros(cin, device="cuda")
            nfl = lib.biu_bwd_data_bnred_floats(dxd2.a(), kd, 0)
            part = torch.empty(nfl, device="cuda")
            nblk = C.c_int(0)
            check(lib.biu_conv_bwd_data_bnred(dyd.a(), ptr(wd), ptr(pk), kd, 3, 3, 1, dxd2.a(), yup.a(), ptr(one), ptr(zero), ptr(one), ptr(zero), ptr(one),
                                              ptr(part), nfl, C.byref(nblk), None, 0, code, stream()), "conv_bwd_data_bnred")
            record(f"conv_dgrad_bnred[{tag}]", dxd2.get(squeeze2d=sq), ref, el(cout), taps=tap, red=co)
        # ---- weight gradient: x non-zero at one voxel per channel (every dw element is one product, or zero where the tap leaves the tensor)
        x, vox = onehot_x(n, cin, sp, s, seed + 6)
        xd = Dev(x)
        ref = conv_w(x.double(), (cout, cin, *([3] * nd)), dy.double(), padding=1)
        wsz = lib.biu_conv_bwd_weight_workspace(cin, cout, kd, 3, 3, code)
        wsb = u8(wsz)
        dw = torch.full((cout, cin, *([3] * nd)), float("nan"), device="cuda")
        check(lib.biu_conv_bwd_weight(xd.a(), None, dyd.a(), kd, 3, 3, 1, ptr(dw), None, ptr(wsb), wsz, code, stream()), "conv_bwd_weight")
        alive_taps = torch.nonzero((ref != 0).reshape(cout * cin, T).any(0)).flatten()
        record(f"conv_wgrad[{tag}]", dw.cpu(), ref, True, ch_dims=(0, 1), taps=alive_taps, red=vox, rows_alive=slice(None))
        if variants:
            # the BatchNorm backward fused into the loader, made the identity: dy = 1 * da * T'(.) + 0 * y + 0 with slope 1 (the entry point takes
            # no NULL y); da must come back bit-identical
            dad = Dev(dy)
            yy = Dev(operands(n, cout, *sp, seed=seed + 7))
            one, zero = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
            dw2 = torch.full_like(dw, float("nan"))
            check(lib.biu_conv_bwd_weight_bn(xd.a(), None, dad.a(), yy.a(), ptr(one), ptr(zero), ptr(one), ptr(one), ptr(zero), ptr(zero), kd, 3, 3, 1,
                                             ptr(dw2), ptr(wsb), wsz, code, stream()), "conv_bwd_weight_bn")
            record(f"conv_wgrad_bn[{tag}]", dw2.cpu(), ref, True, ch_dims=(0, 1), taps=alive_taps, red=vox, rows_alive=slice(None),
                   extra=torch.equal(dad.buf, dyd.buf))


def probe_cat(tag, n, c0, c1, cout, sp):
    """The two-source forms of the 2-D convolution: (x0 | x1) -> y, dy -> (dx0 | dx1), weight gradient with y = NULL."""
    cin, T = c0 + c1, 9
    zb = torch.zeros(cout, device="cuda")
    for s in range(NSETS):
        seed = 1000 * s + 517
        x = operands(n, cin, *sp, seed=seed + 1)
        d0, d1 = Dev(x[:, :c0]), Dev(x[:, c0:])
        ci, tap = picks(cout, cin, T, s)
        w = torch.zeros(cout, cin, T)
        w[torch.arange(cout), ci, tap] = operands(cout, seed=seed + 2)
        w = w.view(cout, cin, 3, 3)
        wd = w.cuda()
        pk = pack_conv(0, wd, cin, cout, 1)
        yd = Dev(shape=shape5(n, cout, sp))
        assert lib.biu_conv_cat_ok(d0.a(), d1.a(), yd.a(), 1, 3, 3, 1, code) == 1
        check(lib.biu_conv_fwd_cat(d0.a(), None, d1.a(), None, ptr(wd), ptr(pk), ptr(zb), 1, 3, 3, 1, yd.a(), None, 0, None, None, 0, code, stream()), "conv_fwd_cat")
        record(f"conv_fwd_cat[{tag}]", yd.get(squeeze2d=True), F.conv2d(x.double(), w.double(), padding=1), True, taps=tap, red=ci)
        dy = operands(n, cout, *sp, seed=seed + 3)
        dyd = Dev(dy)
        co, tap = picks(cin, cout, T, s)
        w = torch.zeros(cout, cin, T)
        w[co, torch.arange(cin), tap] = operands(cin, seed=seed + 4)
        w = w.view(cout, cin, 3, 3)
        wd = w.cuda()
        pk = pack_conv(1, wd, cin, cout, 1)
        g0, g1 = Dev(shape=shape5(n, c0, sp)), Dev(shape=shape5(n, c1, sp))
        check(lib.biu_conv_bwd_data_cat(dyd.a(), ptr(wd), ptr(pk), 1, 3, 3, 1, g0.a(), 0, g1.a(), 0, None, 0, code, stream()), "conv_bwd_data_cat")
        got = torch.cat([g0.get(squeeze2d=True), g1.get(squeeze2d=True)], 1)
        record(f"conv_dgrad_cat[{tag}]", got, torch.nn.grad.conv2d_input((n, cin, *sp), w.double(), dy.double(), padding=1), True, taps=tap, red=co)
        x, vox = onehot_x(n, cin, sp, s, seed + 6)
        d0, d1 = Dev(x[:, :c0]), Dev(x[:, c0:])
        ref = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), dy.double(), padding=1)
        wsz = lib.biu_conv_bwd_weight_workspace(cin, cout, 1, 3, 3, code)
        wsb = u8(wsz)
        dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
        check(lib.biu_conv_bwd_weight_cat(d0.a(), None, d1.a(), None, dyd.a(), None, None, None, None, None, None, None, 1, 3, 3, 1, ptr(dw), ptr(wsb), wsz, code,
                                          stream()), "conv_bwd_weight_cat")
        alive_taps = torch.nonzero((ref != 0).reshape(cout * cin, T).any(0)).flatten()
        record(f"conv_wgrad_cat[{tag}]", dw.cpu(), ref, True, ch_dims=(0, 1), taps=alive_taps, red=vox, rows_alive=slice(None))


def probe_convt(tag, nd, n, cin, cout, sp):
    """ConvTranspose k2 s2 cin -> cout on the coarse extent sp: forward, data gradient, weight gradient."""
    kd, A = (1, 4) if nd == 2 else (2, 8)
    sq = nd == 2
    ct = F.conv_transpose2d if nd == 2 else F.conv_transpose3d
    cv = F.conv2d if nd == 2 else F.conv3d
    cw = torch.nn.grad.conv2d_weight if nd == 2 else torch.nn.grad.conv3d_weight
    hi = tuple(2 * e for e in sp)
    zb = torch.zeros(cout, device="cuda")
    el = lambda K: K >= 16 and K % 16 == 0          # noqa: E731
    for s in range(NSETS):
        seed = 1000 * s + 317
        # ---- forward: w non-zero at one ci per (co, a) -- every output element is one product
        x = operands(n, cin, *sp, seed=seed + 1)
        xd = Dev(x)
        ci, _ = picks(cout * A, cin, 1, s)
        w = torch.zeros(cin, cout, A)
        rows = torch.arange(cout * A)
        w[ci, rows // A, rows % A] = operands(cout * A, seed=seed + 2)
        w = w.view(cin, cout, *([2] * nd))
        wd = w.cuda()
        pk = pack_convt(0, wd, cin, cout, kd)
        yd = Dev(shape=shape5(n, cout, hi))
        check(lib.biu_convt_fwd(xd.a(), None, ptr(wd), ptr(pk), ptr(zb), kd, yd.a(), code, stream()), "convt_fwd")
        record(f"convt_fwd[{tag}]", yd.get(squeeze2d=sq), ct(x.double(), w.double(), stride=2), el(cin), taps=rows % A, red=ci, rows_alive=slice(None))
        # ---- data gradient: w non-zero at one (co, a) per ci
        g = operands(n, cout, *hi, seed=seed + 3)
        gd = Dev(g)
        co, a = picks(cin, cout, A, s)
        w = torch.zeros(cin, cout, A)
        w[torch.arange(cin), co, a] = operands(cin, seed=seed + 4)
        w = w.view(cin, cout, *([2] * nd))
        wd = w.cuda()
        pk = pack_convt(1, wd, cin, cout, kd)
        dxd = Dev(shape=shape5(n, cin, sp))
        check(lib.biu_convt_bwd_data(gd.a(), ptr(wd), ptr(pk), kd, dxd.a(), 0, code, stream()), "convt_bwd_data")
        record(f"convt_dgrad[{tag}]", dxd.get(squeeze2d=sq), cv(g.double(), w.double(), stride=2), el(cout) and kd == 1, taps=a, red=co)
        # ---- weight gradient: x non-zero at one voxel per channel
        x, vox = onehot_x(n, cin, sp, s, seed + 6)
        xd = Dev(x)
        ref = cw(g.double(), (cin, cout, *([2] * nd)), x.double(), stride=2)
        wsz = lib.biu_convt_bwd_weight_workspace(cin, cout, kd, code)
        wsb = u8(wsz)
        dw = torch.full((cin, cout, *([2] * nd)), float("nan"), device="cuda")
        check(lib.biu_convt_bwd_weight(xd.a(), None, gd.a(), kd, ptr(dw), None, ptr(wsb), wsz, code, stream()), "convt_bwd_weight")
        record(f"convt_wgrad[{tag}]", dw.cpu(), ref, True, ch_dims=(0, 1), taps=torch.arange(A), red=vox, rows_alive=slice(None))


# 2-D 3x3: the four forms of the split launch -- one / two 32-channel output tiles per block (odd / even tile count: 96 and 64 channels)
# crossed with W % 32 == 0 or not --, forward and data gradient each (the data gradient's output tiles are cin's)
probe_conv("64-96@24x40", 2, 1, 64, 96, (24, 40))
probe_conv("64-96@32x32", 2, 1, 64, 96, (32, 32), variants=False)
probe_conv("96-64@24x40", 2, 1, 96, 64, (24, 40), variants=False)
probe_conv("96-64@32x32", 2, 1, 96, 64, (32, 32))
# 24 reduction channels: the forward stays on the exact kernel in every mode (its data gradient, 32 reduction channels, does not)
probe_conv("24-32@20x28", 2, 1, 24, 32, (20, 28), variants=False)
# the input-channel split with a caller workspace
probe_conv("256-256@16x16,ksplit", 2, 1, 256, 256, (16, 16), split_ws=True, variants=False)
probe_cat("128|64-64@24x40", 1, 128, 64, 64, (24, 40))
# ConvTranspose2d: forward tiles are cout's, data-gradient tiles cin's (one and two per block either way); weight gradient CA = cin > 32 and <= 32
probe_convt("64-32@16x16", 2, 2, 64, 32, (16, 16))
probe_convt("32-64@10x36", 2, 1, 32, 64, (10, 36))
# 3-D
probe_conv("3d,48-48@5x7x9", 3, 1, 48, 48, (5, 7, 9), variants=False)
probe_convt("3d,64-64@4x8x16", 3, 1, 64, 64, (4, 8, 16))


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. dense float64 bounds of the 2-D launches
# ----------------------------------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def dense_conv(tag, n, cin, cout, sp, *, full=True, split_ws=False):
    x = rnd(n, cin, *sp, seed=1)
    w = rnd(cout, cin, 3, 3, seed=2) * (1.0 / (cin * 9) ** 0.5)
    b = rnd(cout, seed=3)
    xf = XF(cin, seed=4)
    xd = Dev(x, pitch=cin + 16, c0=8)
    xa = xf.apply(xd.ref().squeeze(2)).double()
    wd, bd = w.cuda(), b.cuda()
    W = w.double()
    pk = pack_conv(0, wd, cin, cout, 1)
    yd = Dev(shape=shape5(n, cout, sp), pitch=cout + 8, c0=8)
    ws, need = None, 0
    if split_ws:
        need = lib.biu_conv_split_workspace(cin, yd.a(), None, 1, 3, 3, 1, code)
        assert need > 0
        ws = u8(need)
    check(lib.biu_conv_fwd(xd.a(), xf.x(), ptr(wd), ptr(pk), ptr(bd), 1, 3, 3, 1, yd.a(), ptr(ws), need, code, stream()), "conv_fwd")
    yref, yabs = F.conv2d(xa, W, b.double(), padding=1), F.conv2d(xa.abs(), W.abs(), padding=1)
    dense[f"conv_fwd[{tag}]"] = (yd.get(squeeze2d=True), yref, yabs)
    assert torch.isnan(yd.buf[..., :8]).all(), "conv_fwd wrote outside its channel slice"
    if full:
        yd2 = Dev(shape=shape5(n, cout, sp), pitch=cout + 8, c0=8)
        nfl = lib.biu_conv_fwd_stats_floats(yd2.a(), 1)
        part = torch.full((nfl,), float("nan"), device="cuda")
        nblk = C.c_int(0)
        check(lib.biu_conv_fwd_stats(xd.a(), xf.x(), ptr(wd), ptr(pk), ptr(bd), 1, 3, 3, 1, yd2.a(), ptr(part), nfl, C.byref(nblk), None, 0, code, stream()),
              "conv_fwd_stats")
        got = yd2.get(squeeze2d=True)
        dense[f"conv_fwd_stats[{tag}]"] = (got, yref, yabs)
        stats[f"conv_fwd_stats[{tag}]"] = (part[:nblk.value * cout * 2].view(nblk.value, cout, 2).double().sum(0).cpu(), got)
    dyd = Dev(rnd(n, cout, *sp, seed=5), pitch=cout + 8, c0=0)
    dy = dyd.ref().squeeze(2).double()
    pk1 = pack_conv(1, wd, cin, cout, 1)
    dxd = Dev(shape=shape5(n, cin, sp), pitch=cin + 8, c0=0)
    ws, need = None, 0
    if split_ws:
        need = lib.biu_conv_split_workspace(cout, dxd.a(), None, 1, 3, 3, 1, code)
        assert need > 0
        ws = u8(need)
    check(lib.biu_conv_bwd_data(dyd.a(), ptr(wd), ptr(pk1), 1, 3, 3, 1, dxd.a(), 0, ptr(ws), need, code, stream()), "conv_bwd_data")
    dg = lambda g_, w_: torch.nn.grad.conv2d_input((n, cin, *sp), w_, g_, padding=1)          # noqa: E731
    gref, gabs = dg(dy, W), dg(dy.abs(), W.abs())
    dense[f"conv_dgrad[{tag}]"] = (dxd.get(squeeze2d=True), gref, gabs)
    if full:
        # accumulate onto what dx holds (that term is one more exact summand of the reference and of the sum of magnitudes)
        base = dxd.get(squeeze2d=True)
        check(lib.biu_conv_bwd_data(dyd.a(), ptr(wd), ptr(pk1), 1, 3, 3, 1, dxd.a(), 1, None, 0, code, stream()), "conv_bwd_data(accumulate)")
        dense[f"conv_dgrad_acc[{tag}]"] = (dxd.get(squeeze2d=True), gref + base.double(), gabs + base.double().abs())
        dxd2 = Dev(shape=shape5(n, cin, sp), pitch=cin + 8, c0=0)
        yup = Dev(rnd(n, cin, *sp, seed=6), pitch=cin + 8, c0=8)
        uxf = XF(cin, seed=7)
        md, isd = (rnd(cin, seed=8) * 0.2).cuda(), (rnd(cin, seed=9).abs() + 0.5).cuda()
        nfl = lib.biu_bwd_data_bnred_floats(dxd2.a(), 1, 0)
        part = torch.empty(nfl, device="cuda")
        nblk = C.c_int(0)
        check(lib.biu_conv_bwd_data_bnred(dyd.a(), ptr(wd), ptr(pk1), 1, 3, 3, 1, dxd2.a(), yup.a(), ptr(uxf.d[0]), ptr(uxf.d[1]), ptr(uxf.d[2]), ptr(md), ptr(isd),
                                          ptr(part), nfl, C.byref(nblk), None, 0, code, stream()), "conv_bwd_data_bnred")
        dense[f"conv_dgrad_bnred[{tag}]"] = (dxd2.get(squeeze2d=True), gref, gabs)
    if split_ws:
        return
    wsz = lib.biu_conv_bwd_weight_workspace(cin, cout, 1, 3, 3, code)
    wsb = u8(wsz)
    dw, db = torch.full_like(wd, float("nan")), torch.empty_like(bd)
    check(lib.biu_conv_bwd_weight(xd.a(), xf.x(), dyd.a(), 1, 3, 3, 1, ptr(dw), ptr(db), ptr(wsb), wsz, code, stream()), "conv_bwd_weight")
    wg = lambda a_, g_: torch.nn.grad.conv2d_weight(a_, w.shape, g_, padding=1)          # noqa: E731
    dense[f"conv_wgrad[{tag}]"] = (dw.cpu(), wg(xa, dy), wg(xa.abs(), dy.abs()))
    if full:
        # BatchNorm + LeakyReLU backward in the loader: da -> dy in place, dw w.r.t. the dy it stored
        yxf = XF(cout, seed=9)
        coef = [t.cuda() for t in ((rnd(cout, seed=10) * 0.3 + 1.0), rnd(cout, seed=11) * 0.05, rnd(cout, seed=12) * 0.05)]
        da0 = rnd(n, cout, *sp, seed=13)
        dad = Dev(da0, pitch=cout + 8, c0=0)
        check(lib.biu_conv_bwd_weight_bn(xd.a(), xf.x(), dad.a(), yd.a(), ptr(yxf.d[0]), ptr(yxf.d[1]), ptr(yxf.d[2]), ptr(coef[0]), ptr(coef[1]), ptr(coef[2]),
                                         1, 3, 3, 1, ptr(dw), ptr(wsb), wsz, code, stream()), "conv_bwd_weight_bn")
        yr = yd.get(squeeze2d=True)
        shp = (1, -1, 1, 1)
        tt = yxf.scale.view(shp) * yr + yxf.shift.view(shp)
        dy_ref = coef[0].cpu().view(shp) * da0 * torch.where(tt > 0, torch.ones_like(tt), yxf.slope.view(shp).expand_as(tt)) + coef[1].cpu().view(shp) * yr + \
            coef[2].cpu().view(shp)
        stored = dad.get(squeeze2d=True)
        aux[f"conv_wgrad_bn[{tag}] dy"] = (stored, dy_ref)
        dense[f"conv_wgrad_bn[{tag}]"] = (dw.cpu(), wg(xa, stored.double()), wg(xa.abs(), stored.double().abs()))


def dense_cat(tag, n, c0, c1, cout, sp):
    cin = c0 + c1
    x0, x1 = rnd(n, c0, *sp, seed=1), rnd(n, c1, *sp, seed=2)
    w = rnd(cout, cin, 3, 3, seed=3) * (1.0 / (cin * 9) ** 0.5)
    b = rnd(cout, seed=4)
    xf0 = XF(c0, seed=5)
    d0, d1 = Dev(x0), Dev(x1)
    xa = torch.cat([xf0.apply(d0.ref().squeeze(2)), d1.ref().squeeze(2)], 1).double()
    wd, bd = w.cuda(), b.cuda()
    W = w.double()
    pk0, pk1 = pack_conv(0, wd, cin, cout, 1), pack_conv(1, wd, cin, cout, 1)
    yd = Dev(shape=shape5(n, cout, sp))
    assert lib.biu_conv_cat_ok(d0.a(), d1.a(), yd.a(), 1, 3, 3, 1, code) == 1
    nfl = lib.biu_conv_fwd_stats_floats(yd.a(), 1)
    part = torch.full((nfl,), float("nan"), device="cuda")
    nblk = C.c_int(0)
    check(lib.biu_conv_fwd_cat(d0.a(), xf0.x(), d1.a(), None, ptr(wd), ptr(pk0), ptr(bd), 1, 3, 3, 1, yd.a(), ptr(part), nfl, C.byref(nblk), None, 0, code, stream()),
          "conv_fwd_cat")
    got = yd.get(squeeze2d=True)
    dense[f"conv_fwd_cat[{tag}]"] = (got, F.conv2d(xa, W, b.double(), padding=1), F.conv2d(xa.abs(), W.abs(), padding=1))
    stats[f"conv_fwd_cat[{tag}]"] = (part[:nblk.value * cout * 2].view(nblk.value, cout, 2).double().sum(0).cpu(), got)
    gd = Dev(rnd(n, cout, *sp, seed=7))
    g = gd.ref().squeeze(2).double()
    base1 = rnd(n, c1, *sp, seed=8)
    g0, g1 = Dev(shape=shape5(n, c0, sp)), Dev(base1)
    check(lib.biu_conv_bwd_data_cat(gd.a(), ptr(wd), ptr(pk1), 1, 3, 3, 1, g0.a(), 0, g1.a(), 1, None, 0, code, stream()), "conv_bwd_data_cat")
    dg = lambda g_, w_: torch.nn.grad.conv2d_input((n, cin, *sp), w_, g_, padding=1)          # noqa: E731
    gref, gabs = dg(g, W), dg(g.abs(), W.abs())
    gref[:, c0:] += base1.double()
    gabs[:, c0:] += base1.double().abs()
    dense[f"conv_dgrad_cat[{tag}]"] = (torch.cat([g0.get(squeeze2d=True), g1.get(squeeze2d=True)], 1), gref, gabs)
    wsz = lib.biu_conv_bwd_weight_workspace(cin, cout, 1, 3, 3, code)
    wsb = u8(wsz)
    dw = torch.full_like(wd, float("nan"))
    check(lib.biu_conv_bwd_weight_cat(d0.a(), xf0.x(), d1.a(), None, gd.a(), None, None, None, None, None, None, None, 1, 3, 3, 1, ptr(dw), ptr(wsb), wsz, code,
                                      stream()), "conv_bwd_weight_cat")
    wg = lambda a_, g_: torch.nn.grad.conv2d_weight(a_, w.shape, g_, padding=1)          # noqa: E731
    dense[f"conv_wgrad_cat[{tag}]"] = (dw.cpu(), wg(xa, g), wg(xa.abs(), g.abs()))


def dense_convt(tag, n, cin, cout, sp):
    x = rnd(n, cin, *sp, seed=1)
    w = rnd(cin, cout, 2, 2, seed=2) * (1.0 / cin ** 0.5)
    b = rnd(cout, seed=3)
    xf = XF(cin, seed=4)
    xd = Dev(x, pitch=cin + 8, c0=8)
    xa = xf.apply(xd.ref().squeeze(2)).double()
    wd, bd = w.cuda(), b.cuda()
    W = w.double()
    hi = tuple(2 * e for e in sp)
    pk = pack_convt(0, wd, cin, cout, 1)
    yd = Dev(shape=shape5(n, cout, hi), pitch=cout + 32, c0=0)
    check(lib.biu_convt_fwd(xd.a(), xf.x(), ptr(wd), ptr(pk), ptr(bd), 1, yd.a(), code, stream()), "convt_fwd")
    ct = lambda a_, w_, b_=None: F.conv_transpose2d(a_, w_, b_, stride=2)          # noqa: E731
    dense[f"convt_fwd[{tag}]"] = (yd.get(squeeze2d=True), ct(xa, W, b.double()), ct(xa.abs(), W.abs()))
    assert torch.isnan(yd.buf[..., cout:]).all(), "convt_fwd wrote outside its channel slice"
    gd = Dev(rnd(n, cout, *hi, seed=5))
    g = gd.ref().squeeze(2).double()
    pk1 = pack_convt(1, wd, cin, cout, 1)
    dxd = Dev(shape=shape5(n, cin, sp))
    check(lib.biu_convt_bwd_data(gd.a(), ptr(wd), ptr(pk1), 1, dxd.a(), 0, code, stream()), "convt_bwd_data")
    dense[f"convt_dgrad[{tag}]"] = (dxd.get(squeeze2d=True), F.conv2d(g, W, stride=2), F.conv2d(g.abs(), W.abs(), stride=2))
    wsz = lib.biu_convt_bwd_weight_workspace(cin, cout, 1, code)
    wsb = u8(wsz)
    dw, db = torch.full_like(wd, float("nan")), torch.empty_like(bd)
    check(lib.biu_convt_bwd_weight(xd.a(), xf.x(), gd.a(), 1, ptr(dw), ptr(db), ptr(wsb), wsz, code, stream()), "convt_bwd_weight")
    cw = lambda a_, g_: torch.nn.grad.conv2d_weight(g_, (cin, cout, 2, 2), a_, stride=2)          # noqa: E731   (dW[ci][co][k] = sum_v x[v][ci] g[2v+k][co])
    dense[f"convt_wgrad[{tag}]"] = (dw.cpu(), cw(xa, g), cw(xa.abs(), g.abs()))


dense_conv("64-96@24x40", 2, 64, 96, (24, 40))
dense_conv("96-64@32x32", 1, 96, 64, (32, 32), full=False)
dense_conv("256-256@16x16,ksplit", 1, 256, 256, (16, 16), full=False, split_ws=True)
dense_cat("128|64-64@24x40", 1, 128, 64, 64, (24, 40))
dense_convt("64-32@16x16", 2, 64, 32, (16, 16))
dense_convt("32-64@10x36", 1, 32, 64, (10, 36))

torch.cuda.synchronize()
mode = os.environ.get("BIU_FP32_PRODUCTS", "?")
lg = lambda v: f"2^{math.log2(v):7.2f}" if v > 0 and math.isfinite(v) else f"{v:9.3g}"          # noqa: E731
for name, r in probe.items():
    r["sha"] = r["sha"].hexdigest()
    r["median"] = max(r["median"])
    print(f"{mode:7s} {name:36s} {'split' if r['eligible'] else 'exact'}  worst {lg(r['worst'])}  median {lg(r['median'])}  products {r['products']:7d}  "
          f"zeros {r['zeros']:6d} (wrong {r['zeros_bad']}, -0 {r['negzero']})  taps {len(r['taps']):2d}  positions {len(r['pos']):2d}  chunks {len(r['chunks']):3d}  "
          f"tiles {len(r['tiles'])}  launches {r['launches']}")
torch.save(dict(probe=probe, dense={k: tuple(t.detach().cpu() for t in v) for k, v in dense.items()},
                stats={k: tuple(t.detach().cpu() for t in v) for k, v in stats.items()},
                aux={k: tuple(t.detach().cpu() for t in v) for k, v in aux.items()}), sys.argv[1])
