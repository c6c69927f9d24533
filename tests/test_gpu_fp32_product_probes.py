"""Per-product accuracy of the split fp32 product modes (include/biu.h: biu_set_fp32_products, biu_set_fp32_products_3d), 2-D and 3-D.

tests/fp32_product_probe.py runs once per mode in a child process (the modes are process-wide and latched), BIU_FP32_PRODUCTS and
BIU_FP32_PRODUCTS_3D set alike.  Its single-product probes arrange the operands of every launch -- 3x3 / 3x3x3 convolution and ConvTranspose
k2 s2, forward, data gradient and weight gradient, in the launch forms the 2-D kernels have -- so that each output element is exactly one
product of two full-mantissa fp32 values or exactly zero.  Per op and mode:
  * every output that must be zero is +0.0 (border taps in the padding, tile tails, planes that do not pair);
  * max |got - ref| / |ref| <= tests/fp32_split.BOUND[mode] against the float64 product: 2^-22 bf16x6, 2^-14 bf16x3 (the c of
    tests/test_gpu_fp32_products_3d.py), 2^-23 exact.  tests/test_fp32_split_host.py proves on the same operand generator that a product with
    any single term missing exceeds these bounds at least 4 x (worst) and for most single products (median).  Measured
    (profiles/r11_fp32_product_probes.txt): exact worst 2^-24.0 (the fp32 MFMA rounds a single product to nearest), bf16x3 2^-15.2, bf16x6
    2^-22.6 -- the latter above the 2^-23.4 of a round-to-nearest restatement of the six-term sum: the pipe's accumulator costs the rest;
  * launches that stay exact by rule (fewer than 16 or a non-multiple of 16 reduction channels; the ConvTranspose3d data gradient) hold the exact
    bound in every mode and are bit-identical across the three children; split-eligible launches are not bit-identical to the exact child's;
  * the probes reached every tap, every position of a 16-channel chunk, two or more chunks and every 32-channel tile, with at least
    MIN_PRODUCTS single products per op.
The same child runs every split-eligible 2-D launch on dense operands (real transform, pitched slices, bias) against float64 within
(c + 2^-16) * sum|a||w|, bf16x6 also within tests/gpu_util.tol("f32"), and the BatchNorm partial sums of the forward's epilogue against the
float64 sums of the stored output."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests.fp32_split import BOUND, MIN_PRODUCTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODES = ("exact", "bf16x3", "bf16x6")
# taps per kernel (the reduction position of a weight gradient is a voxel, not a channel: its positions and chunks count voxels)
TAPS = {"conv": 9, "conv3d": 27, "convt": 4, "convt3d": 8}


def _env(mode):
    env = dict(os.environ)
    env.pop("BIU_DISABLE", None)
    env["BIU_FP32_PRODUCTS"] = mode
    env["BIU_FP32_PRODUCTS_3D"] = mode
    return env


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    d = tmp_path_factory.mktemp("fp32_product_probes")
    res = {}
    for mode in MODES:
        out = str(d / f"{mode}.pt")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fp32_product_probe.py"), out], env=_env(mode), cwd=ROOT, capture_output=True, text=True,
                           timeout=240)
        print(r.stdout)
        assert r.returncode == 0, f"{mode} child failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
        res[mode] = torch.load(out)
    return res


def _ntaps(op):
    kind = "convt" if op.startswith("convt") else "conv"
    return TAPS[kind + ("3d" if "[3d," in op else "")]


def _lg(v):
    return f"2^{math.log2(v):.2f}" if v > 0 and math.isfinite(v) else str(v)


@pytest.mark.timeout(900)
def test_single_products_are_within_the_bound_and_zeros_are_zero(children):
    ops = list(children["exact"]["probe"])
    assert len(ops) >= 39
    for mode in MODES:
        assert list(children[mode]["probe"]) == ops
        for op, r in children[mode]["probe"].items():
            what = f"{mode} {op}"
            assert r["nonfinite"] == 0, f"{what}: {r['nonfinite']} non-finite outputs"
            assert r["zeros_bad"] == 0, f"{what}: {r['zeros_bad']} of {r['zeros']} outputs that must be zero are not"
            assert r["negzero"] == 0, f"{what}: {r['negzero']} outputs that must be +0.0 are -0.0"
            assert r["extra_ok"], f"{what}: the caller's workspace was not used / da was not written back unchanged"
            bound = BOUND[mode] if r["eligible"] else BOUND["exact"]
            assert r["worst"] <= bound, f"{what}: worst single product errs by {_lg(r['worst'])}, bound {_lg(bound)} (median {_lg(r['median'])})"


@pytest.mark.timeout(900)
def test_probes_cover_every_tap_chunk_position_and_tile(children):
    for op, r in children["bf16x6"]["probe"].items():
        assert r["launches"] >= 3 and r["products"] >= MIN_PRODUCTS, f"{op}: {r['products']} products in {r['launches']} launches"
        assert r["taps"] == set(range(_ntaps(op))), f"{op}: taps {sorted(r['taps'])}"
        assert len(r["tiles"]) == r["ntiles"], f"{op}: 32-channel tiles {sorted(r['tiles'])} of {r['ntiles']}"
        if r["eligible"]:
            assert r["pos"] == set(range(16)), f"{op}: positions {sorted(r['pos'])}"
            assert len(r["chunks"]) >= 2, f"{op}: chunks {sorted(r['chunks'])}"
    # the launch forms: one and two output tiles per block (odd / even tile count) x W % 32, both ways; the exact-by-rule launches
    p = children["bf16x6"]["probe"]
    for tag in ("64-96@24x40", "64-96@32x32", "96-64@24x40", "96-64@32x32"):
        assert p[f"conv_fwd[{tag}]"]["eligible"] and p[f"conv_dgrad[{tag}]"]["eligible"]
    assert not p["conv_fwd[24-32@20x28]"]["eligible"] and p["conv_dgrad[24-32@20x28]"]["eligible"]
    assert not p["convt_dgrad[3d,64-64@4x8x16]"]["eligible"] and p["convt_fwd[3d,64-64@4x8x16]"]["eligible"]


@pytest.mark.timeout(900)
def test_split_launches_ran_and_exact_launches_stayed_exact(children):
    ex = children["exact"]["probe"]
    for mode in ("bf16x3", "bf16x6"):
        for op, r in children[mode]["probe"].items():
            if r["eligible"]:
                assert r["sha"] != ex[op]["sha"], f"{mode} {op}: bit-identical to exact -- the split kernel did not run"
            else:
                assert r["sha"] == ex[op]["sha"], f"{mode} {op}: should stay on the exact kernel, bit for bit"
    # what the exact fp32 MFMA does to a single product: round to nearest (<= 2^-24) or not -- printed for the record, bounded above
    worst = max(r["worst"] for r in ex.values())
    print(f"exact child: worst single product {_lg(worst)} = {worst * 2.0 ** 24:.6f} x 2^-24")


@pytest.mark.timeout(900)
def test_dense_2d_launches_are_within_their_float64_bound(children):
    from tests.gpu_util import tol
    ops = list(children["exact"]["dense"])
    assert len(ops) >= 20
    for mode, c in [("exact", 0.0), ("bf16x3", 2.0 ** -14), ("bf16x6", 2.0 ** -22)]:
        assert list(children[mode]["dense"]) == ops
        for op, (got, ref, aref) in children[mode]["dense"].items():
            assert torch.isfinite(got).all(), f"{mode} {op}: non-finite"
            err = (got.double() - ref).abs()
            bound = (c + 2.0 ** -16) * aref + 1e-30        # (+ fp32 accumulation and storage rounding: <= n u sum|ab|, a few u sqrt(n) in practice)
            worst = float((err / bound).max())
            assert worst <= 1.0, f"{mode} {op}: error {worst:.2f} x its bound"
            if mode == "bf16x6":
                t = tol("f32")
                torch.testing.assert_close(got, ref.float(), rtol=t["rtol"], atol=t["atol"] * max(1.0, float(ref.abs().max())))
            if mode != "exact":
                assert not torch.equal(got, children["exact"]["dense"][op][0]), f"{mode} {op}: bit-identical to exact -- the split kernel did not run"
        # the BatchNorm partial sums from the forward's epilogue = the float64 sums of the output it stored
        assert len(children[mode]["stats"]) >= 2
        for op, (sums, got) in children[mode]["stats"].items():
            gd = got.double()
            cout = gd.shape[1]
            torch.testing.assert_close(sums[:, 0], gd.sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-4 * float(gd.abs().sum() / cout), msg=lambda m: f"{mode} {op} sums: {m}")
            torch.testing.assert_close(sums[:, 1], (gd * gd).sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-6, msg=lambda m: f"{mode} {op} sums of squares: {m}")
        # the dy the fused BatchNorm backward stored (element-wise fp32 arithmetic: the tolerance of test_conv_cat_forms_match_concat_buffer)
        for op, (stored, dy_ref) in children[mode]["aux"].items():
            torch.testing.assert_close(stored, dy_ref, rtol=1e-5, atol=1e-5, msg=lambda m: f"{mode} {op}: {m}")
