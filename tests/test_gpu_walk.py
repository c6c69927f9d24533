"""Value tests of the persistent convolution kernels at shapes where a block WALKS several bricks.

Every MFMA convolution launch is persistent: about one block per CU, block b runs bricks b, b + g, b + 2g, ...  The cases of
tests/test_gpu_ops.py have fewer bricks than blocks, so there every block runs one brick and stops; the hand-over from one brick to the next
(activation prefetch, weight-slab flip, the dead prefetch of a block that stops a round early, both walk orders, BatchNorm statistics and
weight gradients that accumulate across bricks, da -> dy rewritten brick after brick) runs at benchmark size only.  Here tests/walk_geometry.py
picks, from the CU count of the device, the smallest extents with at least three full rounds plus a ragged last one (two for the first layer),
and the bodies of the op tests (tests/test_gpu_ops.py: run_*) run on them against a float64 CPU reference with the tolerances they use there.

Each case asserts its precondition as a failure, never a skip.  Where the C ABI hands out the blocks per column (bn_nblk / nblk) and the
float64 reference of the larger shape stays inside the budget, the precondition is the brick-free one -- no brick of any kernel form holds more
than 1024 voxels, so ceil(voxels / 1024) >= 3 * rows walks whatever brick the kernel takes, and rows < ceil(voxels / 1024) -- with nothing of
the mirror table in it.  Where that shape is past the budget (the 512- and 256-voxel bricks ask for two and four times the voxels: the 2- and
4-column 3-D cases, k_conv16_pipe in 3-D, the folded decoder level) the bricks are COUNTED WITH THE TABLE'S BRICK and the reported rows must
equal the table's grid; where the API reports nothing (weight gradients, biu_convt_fwd, biu_upconv_bwd_data, biu_conv_bwd_data_cat) both come
from the table.  The `WALK` line of each case says which (`bound=`); its bricks, blocks per column and rounds are always the table's.
tools/walk_rounds.py collects those lines into profiles/r10_walk_rounds.txt.

What does not fit the 15 GMAC reference budget and has no case (the arithmetic; g = blocks per column on 256 CUs):
  * biu_foldt_fwd in its rolling-window form: it exists for 64 -> (cup + 32) -> 32 channels on bf16 only (fold_plan, and roll_plan's accumulate
    form for the skip half); its statistics come from k_conv_roll's launch, g = 256 items of 8 x 32 x (depth >= 4) voxels: with the narrowest
    up half, cup = 16, 3 * 256 * 1024 voxels * 27 taps * 48 * 32 = 32.6 GMAC.  (k_conv_roll itself walks in the roll-* cases; the brick form of
    the level walks here.)
  * a walking biu_foldt_bwd_data / biu_foldt_bwd_weight_bn: their launches have ONE column of g = 256 blocks on the coarse tensor, in bricks of
    512 voxels (256 in the fp32 weight gradient).  Even at 256 voxels a brick, 3 * 256 * 256 coarse voxels * 8 fine * 27 taps *
    (cup + cskip >= 32) * 32 = 43 GMAC for the reference of the level.  Both are compositions of launches that do walk here against a
    reference: biu_mfma_conv / biu_mfma_wgrad on the skip half (the conv and weight-gradient cases) and biu_mfma_upconv_dgrad /
    biu_mfma_upconv_wgrad on the coarse half (upconv-dgrad-*, upconv-wgrad-*, with the 8-tap reference).  The foldt-brick-form cases run both, in
    one launch and in phases, on the shape whose FORWARD walks.
  * the two-source forward in 3-D: tests/walk_geometry.py, _cat_specs.

k_convt_all (bf16 ConvTranspose up to 64 channels) caps its grid at a quarter of its tiles, so its cases in tests/test_gpu_ops.py already walk
at least four tiles per block; it has no case here."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import test_gpu_ops as ops
from tests import walk_geometry as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ids(family):
    return [s.id for s in G.SPECS if s.family == family]


def _walks_from_rows(c, rows, what, rounds=3):
    """The precondition from what the launch reported.  c.free: brick-free -- `rows` blocks per column and the voxels of the tensor the launch
    walks, nothing of the table.  Otherwise (the brick-free shape is past the reference budget) the bricks are counted with the table's brick,
    and the table's grid must be what the launch reports."""
    if c.free:
        least = -(-c.n * math.prod(c.sp) // 1024)                            # no brick of any kernel form holds more than 1024 voxels
        assert rows < least, f"{c.id} {what}: {rows} blocks per column for at least {least} bricks -- nothing walks"
        assert least >= rounds * rows, f"{c.id} {what}: at least {least} bricks on {rows} blocks per column are not {rounds} full rounds"
        return
    assert rows == c.g, f"{c.id} {what}: the launch reports {rows} blocks per column, tests/walk_geometry.py mirrors {c.g}"
    assert rows < c.nbricks, f"{c.id} {what}: {rows} blocks for {c.nbricks} bricks (counted with the table's brick) -- nothing walks"
    assert rounds * rows < c.nbricks and c.nbricks % rows != 0 and c.nbricks % rows <= rows / 2, \
        f"{c.id} {what}: {c.nbricks} bricks (counted with the table's brick) on {rows} blocks is not {rounds} full rounds plus a ragged one"


def _walks_from_table(c, rounds=3):
    assert c.g < c.nbricks and G.walks(c.nbricks, c.g, rounds), f"{c.id}: {c.nbricks} bricks on {c.g} blocks is not {rounds} full rounds plus a ragged one"


def _report(c, rec, source):
    dev = rec.get("dev", {})
    worst = max(dev.items(), key=lambda kv: kv[1]) if dev else ("-", float("nan"))
    print(f"WALK {c.id:34s} {c.row:18s} n={c.n} sp={'x'.join(map(str, c.sp)):14s} cols={c.cols:2d} bricks={c.nbricks:5d} blocks/col={c.g:4d} "
          f"rounds={c.rounds} order={c.order:7s} blocks-from={source:5s} bound={'voxels' if c.free and source == 'api' else 'table':6s} "
          f"worst={worst[1]:.3f} ({worst[0]})")


def check_conv_walk(spec):
    """k_conv_pipe, k_conv16_pipe and k_conv_roll through biu_conv_fwd_stats, biu_conv_fwd, biu_conv_bwd_data (plain, accumulate) and
    biu_conv_bwd_data_bnred."""
    c = G.build(spec, _cus())
    rec = {}
    try:
        ops.run_conv_fwd_stats_and_dgrad_bnred((c.n, spec.cin, spec.cout, c.sp), spec.dtype, F64, rec, red_like="roll" if spec.family == "roll" else "brick")
    finally:
        _report(c, rec, "api")
    if "fwd" in spec.launch:
        _walks_from_rows(c, rec["rows_fwd"], "biu_conv_fwd_stats")
    if "dgrad" in spec.launch:
        _walks_from_rows(c, rec["rows_bnred"], "biu_conv_bwd_data_bnred")
    return rec


@pytest.mark.parametrize("sid", _ids("conv") + _ids("roll"))
def test_conv_walk(sid):
    check_conv_walk(G.SPEC_BY_ID[sid])


@pytest.mark.parametrize("sid", _ids("split"))
def test_conv_walk_under_split_fp32_products_3d(sid, tmp_path):
    """fp32 3x3x3 as bf16x3 / bf16x6 products (biu_set_fp32_products_3d).  The mode is latched by the first fp32 3-D call of a process, so the
    case runs in a child that sets it first (and asks for the default again in a `finally`; the library may refuse that once latched)."""
    out = str(tmp_path / "rec.json")
    env = dict(os.environ)
    env.pop("BIU_FP32_PRODUCTS_3D", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "walk_probe.py"), sid, out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.load(open(out))
    # The child asserts the walk brick-free (ceil(voxels / 1024) >= 3 * rows), so it holds for the split kernels' bricks (4 x 8 x 16 and
    # 4 x 4 x 16) as for the exact kernel's; that the mode was in force there is biu_set_fp32_products_3d's return value, checked before the
    # first convolution.  Here only: three output tiles have three columns in either kernel.
    assert rec["rows_fwd"] == G.build(G.SPEC_BY_ID[sid], _cus()).g


@pytest.mark.parametrize("sid", _ids("wgrad") + _ids("wgrad_bn"))
def test_weight_gradient_walk(sid):
    """k_wgrad_pipe (brick and paired-tap forms) and k_wgrad_roll (3-D, its 16-channel form, 2-D over a batch of 8) through
    biu_conv_bwd_weight and biu_conv_bwd_weight_bn; the fused form's da -> dy against biu_bn_bwd_apply's formula on every voxel.  The API
    reports no grid for these: the precondition comes from the table."""
    spec = G.SPEC_BY_ID[sid]
    c = G.build(spec, _cus())
    _walks_from_table(c)
    rec = {}
    case = (spec.nd, c.n, spec.cin, spec.cout, c.sp)
    try:
        if spec.family == "wgrad":
            ops.run_conv_mfma_fwd_dgrad(case, spec.dtype, F64, rec)
        else:
            ops.run_conv_bwd_weight_bn(case, spec.dtype, F64, rec, torch_ref=True, reps=1)
    finally:
        _report(c, rec, "table")


@pytest.mark.parametrize("sid", _ids("cat"))
def test_two_source_walk(sid):
    """biu_conv_fwd_cat, biu_conv_bwd_data_cat and biu_conv_bwd_weight_cat (plain and BatchNorm-fused) on k_conv_pipe / k_wgrad_pipe, each with
    the launch its spec names walking; the calls behind that launch in forward -> data gradient -> weight gradient order are left out."""
    spec = G.SPEC_BY_ID[sid]
    c = G.build(spec, _cus())
    if spec.launch != "fwd":
        _walks_from_table(c)
    rec = {}
    try:
        ops.run_conv_cat_forms((spec.nd, c.n, 64, 32, spec.cout, c.sp), spec.dtype, F64, rec, upto=spec.launch)
    finally:
        _report(c, rec, "api" if spec.launch == "fwd" else "table")
    if spec.launch == "fwd":
        _walks_from_rows(c, rec["rows_fwd"], "biu_conv_fwd_cat")


@pytest.mark.parametrize("sid", _ids("convt"))
def test_convtranspose_walk(sid):
    """ConvTranspose k2 s2 on k_conv_pipe (fp32; bf16 off k_convt_all's channel counts) through biu_convt_fwd, biu_convt_bwd_data and
    biu_convt_bwd_data_bnred."""
    spec = G.SPEC_BY_ID[sid]
    c = G.build(spec, _cus())
    _walks_from_table(c)
    rec = {}
    case = (spec.nd, c.n, spec.cin, spec.cout, c.sp)
    try:
        ops.run_convtranspose_mfma(case, spec.dtype, F64, rec)
        if spec.launch == "dgrad":
            ops.run_convt_bwd_data_bnred(case, spec.dtype, rec)
    finally:
        _report(c, rec, "api" if spec.launch == "dgrad" else "table")
    if spec.launch == "dgrad":
        _walks_from_rows(c, rec["rows_bnred"], "biu_convt_bwd_data_bnred")


@pytest.mark.parametrize("sid", _ids("upconv"))
def test_upconv_walk(sid):
    """Nearest x2 folded into the 3x3x3 convolution: biu_upconv_fwd with statistics (eight parity columns per output tile) and
    biu_upconv_bwd_data (plain, accumulate) on the same tensors; the launch the spec names walks.  The data-gradient cases take the 8-tap
    reference: 769 coarse bricks are 2.8 M fine voxels."""
    spec = G.SPEC_BY_ID[sid]
    c = G.build(spec, _cus())
    rec = {}
    if spec.launch == "dgrad":
        _walks_from_table(c)
    try:
        ops.run_upconv_fwd((c.n, spec.cin, spec.cout, c.sp), spec.dtype, F64, rec, folded=spec.launch == "dgrad")
    finally:
        _report(c, rec, "api" if spec.launch == "fwd" else "table")
    assert "upconv_bwd_data" in rec["dev"]                                  # (the helper leaves the data gradient out where no kernel serves it)
    if spec.launch == "fwd":
        assert rec["rows_fwd"] % 8 == 0                                     # one row per block and parity class
        _walks_from_rows(c, rec["rows_fwd"] // 8, "biu_upconv_fwd")


@pytest.mark.parametrize("sid", _ids("upconv_wgrad"))
def test_upconv_weight_gradient_walk(sid):
    """biu_upconv_bwd_weight_bn: k_wgrad_pipe per parity class on the coarse grid, da -> dy rewritten on the fine one brick after brick --
    against biu_bn_bwd_apply's formula on every fine voxel and torch's weight gradient of the stored dy (8-tap reference), besides the
    unfolded device path the op test compares with."""
    spec = G.SPEC_BY_ID[sid]
    c = G.build(spec, _cus())
    _walks_from_table(c)
    rec = {}
    try:
        ops.run_upconv_bwd_weight((c.n, spec.cin, spec.cout, c.sp), spec.dtype, F64, rec, torch_ref=True, reps=1)
    finally:
        _report(c, rec, "table")


@pytest.mark.parametrize("sid", _ids("foldt"))
def test_folded_decoder_level_walk(sid):
    """biu_foldt_fwd in its brick form (the up half's launch on the coarse tensor walks; its epilogue carries the statistics of the finished
    output), then biu_foldt_bwd_data and biu_foldt_bwd_weight_bn, in one launch and in phases, on the same tensors."""
    spec = G.SPEC_BY_ID[sid]
    c = G.build(spec, _cus())
    o = spec.opts
    rec = {}
    try:
        ops.run_foldt((c.n, o["cl"], o["cup"], o["cs"], spec.cout, c.sp), spec.dtype, F64, rec)
    finally:
        _report(c, rec, "api")
    assert rec["form"] == 0                                                 # (the rolling-window form: see the head of this file)
    assert rec["rows_fwd"] % 8 == 0
    _walks_from_rows(c, rec["rows_fwd"] // 8, "biu_foldt_fwd")


@pytest.mark.parametrize("sid", _ids("rank1"))
def test_rank_one_weight_gradient_walk(sid):
    """biu_conv_bwd_weight_bn_rank1 (k_wgrad_roll's fused 16-channel form; da is not read but rebuilt as bf16(dlogits[v] * w_head[c])): the dy
    it stores against biu_bn_bwd_apply's formula on that da, its dW against torch's weight gradient of the stored dy.  Tolerances: those of
    the fused weight gradient (ops.run_conv_bwd_weight_bn)."""
    from tests.gpu_util import DT, XF, Dev, check, lib, ptr, stream
    spec = G.SPEC_BY_ID[sid]
    c = G.build(spec, _cus())
    _walks_from_table(c)
    code = DT["bf16"][1]
    n, cin, co, sp = c.n, spec.cin, spec.cout, c.sp
    x, xf = Dev(ops.rnd(n, cin, *sp, seed=1), dtype="bf16"), XF(cin, seed=2)
    y, yxf = Dev(ops.rnd(n, co, *sp, seed=3), dtype="bf16"), XF(co, seed=5)
    cA, cB, cC = ops.rnd(co, seed=6) * 0.3 + 1.0, ops.rnd(co, seed=7) * 0.05, ops.rnd(co, seed=8) * 0.05
    coef = [t.cuda() for t in (cA, cB, cC)]
    dl, wh = ops.rnd(n, 1, *sp, seed=4), ops.rnd(1, co, seed=12) * 0.3
    dld, whd = dl.cuda().contiguous(), wh.cuda()
    wsz = max(lib.biu_conv_bwd_weight_workspace(cin, co, 3, 3, 3, code), 16)
    ws = torch.empty(wsz, dtype=torch.uint8, device="cuda")
    dy = Dev(shape=(n, co) + tuple(sp), dtype="bf16")                       # (dense, as the engine's: what biu_conv_bwd_weight_bn_rank1_ok takes)
    assert lib.biu_conv_bwd_weight_bn_rank1_ok(x.a(), dy.a(), y.a(), 1, 3, 3, 3, 1, code) == 1
    dw = torch.full((co, cin, 3, 3, 3), float("nan"), device="cuda")
    rec = {}
    try:
        check(lib.biu_conv_bwd_weight_bn_rank1(x.a(), xf.x(), ptr(dld), ptr(whd), 1, dy.a(), y.a(), ptr(yxf.d[0]), ptr(yxf.d[1]), ptr(yxf.d[2]), ptr(coef[0]),
                                               ptr(coef[1]), ptr(coef[2]), 3, 3, 3, 1, ptr(dw), ptr(ws), wsz, code, stream()), "conv_bwd_weight_bn_rank1")
        shp = (1, -1, 1, 1, 1)
        dar = (dl * wh.view(shp)).bfloat16().to(F64)                        # fp32 product, rounded to the storage type
        yr = y.ref().to(F64)
        tt = yxf.scale.to(F64).view(shp) * yr + yxf.shift.to(F64).view(shp)
        dy_ref = cA.to(F64).view(shp) * dar * torch.where(tt > 0, torch.ones_like(tt), yxf.slope.to(F64).view(shp).expand_as(tt)) + \
            cB.to(F64).view(shp) * yr + cC.to(F64).view(shp)
        got_dy = dy.get()
        ops.close(got_dy, dy_ref, rec, "rank1 da -> dy (formula)", rtol=2e-2, atol=2e-2)
        xa = xf.apply(x.ref()).bfloat16().to(F64)
        gw = torch.ops.aten.convolution_backward(got_dy.to(F64), xa, torch.zeros(co, cin, 3, 3, 3, dtype=F64), None, [1] * 3, [1] * 3, [1] * 3, False,
                                                 [0] * 3, 1, [False, True, False])[1]
        ops.close(dw.cpu(), gw, rec, "rank1 dw (torch)", rtol=2e-2, atol=2e-2 * float(gw.abs().max()))
    finally:
        _report(c, rec, "table")


@pytest.mark.parametrize("sid", _ids("c1m"))
def test_first_layer_walk(sid):
    """The first layer on the matrix cores (biu_c1m_*: bf16, one input channel, 3 blocks per CU): forward with statistics, and the weight
    gradient plain and BatchNorm-fused.  Two full rounds plus a ragged one."""
    spec = G.SPEC_BY_ID[sid]
    c = G.build(spec, _cus())
    rec = {}
    if spec.launch == "fwd":
        try:
            ops.run_conv_fwd_stats_and_dgrad_bnred((c.n, 1, spec.cout, c.sp), spec.dtype, F64, rec, red_like="brick", parts=("fwd",))
        finally:
            _report(c, rec, "api")
        _walks_from_rows(c, rec["rows_fwd"], "biu_conv_fwd_stats", rounds=2)
    else:
        _walks_from_table(c, rounds=2)
        try:
            ops.run_conv_bwd_weight_bn((spec.nd, c.n, 1, spec.cout, c.sp), spec.dtype, F64, rec, torch_ref=True, reps=1)
        finally:
            _report(c, rec, "table")
