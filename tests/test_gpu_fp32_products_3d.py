"""The opt-in split-product modes of the fp32 3-D kernels (BIU_FP32_PRODUCTS_3D=bf16x3 | bf16x6) against the exact fp32 MFMA (the 3-D
default).  The mode is process-wide and latched on first use, so every side runs in a child process of its own:
  * network level (tests/variant_probe.py, unchanged): UNet3D(32) fp32 -- 3x3x3 convolutions forward / data / weight gradient with their
    BatchNorm and two-source forms, the folded decoder levels' skip halves -- and MultiOutputUnet3D(32, use_interpolation=True) fp32;
  * op level: every fp32 case of tests/test_gpu_ops.py (compared with torch fp32 at its fp32 tolerance) once more under bf16x6;
  * op level against float64 (tests/fp32_3d_probe.py): every covered op within c * sum|a||w| of the float64 result (c = 2^-14 bf16x3,
    2^-22 bf16x6, plus fp32 accumulation slack), bf16x6 also within the fp32 tolerance of tests/gpu_util.tol, and not bit-identical to the
    exact child's result (the ConvTranspose3d data gradient, exact in every mode, bit-identical);
  * the exact-fp32 in-situ bounds of tests/test_gpu_insitu.py hold for one bf16x6 step of cfg4 and both cfg5 forms;
  * the split kernels really ran: a split child's logits are not bit-identical to the exact child's.
The bounds here are dense sums whose fp32 accumulation slack (2^-16) is 64 x the c beside it: they catch indexing errors, not a missing term of a
split product.  The per-product statement (every single product within c, 2-D and 3-D) lives in tests/test_gpu_fp32_product_probes.py."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _env(mode):
    env = dict(os.environ)
    env.pop("BIU_DISABLE", None)
    env.pop("BIU_FP32_PRODUCTS_3D", None)
    if mode is not None:
        env["BIU_FP32_PRODUCTS_3D"] = mode
    return env


def _probe(which, mode, tmp_path):
    out = str(tmp_path / f"{which}_{mode}.pt")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "variant_probe.py"), which, out], check=True, env=_env(mode), timeout=300)
    return torch.load(out)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("which", ["unet3d_f32", "mo3d_interp_f32"])
def test_split_products_3d_agree_with_the_exact_fp32_mfma(which, tmp_path):
    ref = _probe(which, "exact", tmp_path)
    for mode, tol_out in [("bf16x6", 1e-5), ("bf16x3", 3e-4)]:
        got = _probe(which, mode, tmp_path)
        assert not torch.equal(got["logits"], ref["logits"]), f"{which} {mode}: bit-identical to exact -- the split kernels did not run"
        # the comparison of test_gpu_variants.py: logits, all gradients together within 2e-2, a single tensor within 4 x that (one LeakyReLU /
        # max-pool decision that falls the other way moves a small bottleneck BatchNorm vector by ~10 %)
        d = float((got["logits"] - ref["logits"]).norm() / ref["logits"].norm())
        assert d <= tol_out, f"{which} {mode}: logits differ by {d:.3e}"
        keys = [k for k in ref if k not in ("loss", "logits")]
        num = sum(float((got[k] - ref[k]).double().pow(2).sum()) for k in keys)
        den = sum(float(ref[k].double().pow(2).sum()) for k in keys)
        assert (num / den) ** 0.5 <= 2e-2, f"{which} {mode}: all gradients together differ by {(num / den) ** 0.5:.3e}"
        worst = max((float((got[k] - ref[k]).norm() / (ref[k].norm() + 1e-30)), k) for k in keys)
        assert worst[0] <= 8e-2, f"{which} {mode}: gradient of {worst[1]} differs by {worst[0]:.3e}"


_LATCH = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
import bio_image_unet_amd as B
from oracle import unet_oracle as O
B.set_fp32_products_3d("bf16x3")
m = B.UNet3D(1, 1, 16).cuda()
m.load_state_dict(O.init_unet3d(1, 1, 16, seed=0))
m.train()
x = torch.rand(2, 1, 16, 32, 32).cuda()
p, l = m(x)
l.sum().backward()
torch.cuda.synchronize()
assert torch.isfinite(l).all()
try:
    B.set_fp32_products_3d("exact")
    print("SWITCH ok")
except Exception as e:
    print("SWITCH refused:", e)
print("DONE")
"""


@pytest.mark.timeout(300)
def test_3d_mode_latches_at_the_first_step():
    r = subprocess.run([sys.executable, "-c", _LATCH, ROOT], env=_env(None), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "SWITCH refused" in r.stdout and "before the first forward" in r.stdout and "DONE" in r.stdout, r.stdout


@pytest.mark.timeout(600)
def test_fp32_op_tests_hold_with_bf16x6_3d_products():
    """bf16x6 is fp32-grade (<= 2^-22 per product: tests/test_gpu_fp32_product_probes.py): every fp32 op test of tests/test_gpu_ops.py holds unchanged under it."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_ops.py"), "-q", "-x", "-k", "f32", "-p", "no:cacheprovider"],
                       env=_env("bf16x6"), cwd=ROOT, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-3000:]


def _ops(mode, tmp_path):
    out = str(tmp_path / f"ops_{mode}.pt")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fp32_3d_probe.py"), out], check=True, env=_env(mode), timeout=300)
    return torch.load(out)


@pytest.mark.timeout(600)
def test_every_split_op_is_within_its_bound_and_ran(tmp_path):
    from tests.gpu_util import tol
    ops = {m: _ops(m, tmp_path) for m in ("exact", "bf16x3", "bf16x6")}
    for mode, c in [("exact", 0.0), ("bf16x3", 2.0 ** -14), ("bf16x6", 2.0 ** -22)]:
        for op, (got, ref, aref) in ops[mode].items():
            assert torch.isfinite(got).all(), f"{mode} {op}: non-finite"
            err = (got.double() - ref).abs()
            bound = (c + 2.0 ** -16) * aref + 1e-30        # (+ fp32 accumulation and storage rounding: <= n u sum|ab|, a few u sqrt(n) in practice)
            worst = float((err / bound).max())
            assert worst <= 1.0, f"{mode} {op}: error {worst:.2f} x its bound"
            if mode == "bf16x6":
                t = tol("f32")
                torch.testing.assert_close(got, ref.float(), rtol=t["rtol"], atol=t["atol"] * max(1.0, float(ref.abs().max())))
            if mode != "exact":
                same = torch.equal(got, ops["exact"][op][0])
                if op == "convt_dgrad":
                    assert same, f"{mode} {op}: should stay on the exact kernel"
                else:
                    assert not same, f"{mode} {op}: bit-identical to exact -- the split kernel did not run"


@pytest.mark.timeout(600)
def test_insitu_bounds_of_exact_fp32_hold_for_bf16x6():
    """One bf16x6 step of cfg4 (UNet3D) and the cfg5 forms (MultiOutputUnet3D, interpolation and ConvTranspose, base 32 and base 64 -- the
    latter with its 768-channel decode1) against the in-situ per-kernel-call bounds written for the exact fp32 kernels."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_insitu.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "train_step and (cfg4_unet3d_f32 or cfg5_mo3d) and not bf16"],
                       env=_env("bf16x6"), cwd=ROOT, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0 and "5 passed" in r.stdout, r.stdout[-3000:]
