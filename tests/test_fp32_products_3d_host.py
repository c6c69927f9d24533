"""CPU-side checks of the fp32 product mode of the 3-D kernels (include/biu.h: biu_set_fp32_products_3d, BIU_FP32_PRODUCTS_3D): argument
validation, independence from the 2-D mode, the environment switch, and the latch a packed-size query sets.  No GPU involved."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (each check in a fresh child process: the modes are process-wide and latch on first use)
_SETTERS = r"""
import sys
sys.path.insert(0, sys.argv[1])
import bio_image_unet_amd as B
import bio_image_unet_amd._lib as L
assert L.lib.biu_set_fp32_products_3d(0) == 0
assert L.lib.biu_set_fp32_products_3d(1) == 0
assert L.lib.biu_set_fp32_products_3d(2) == 0
assert L.lib.biu_set_fp32_products_3d(7) != 0
assert b"mode" in L.lib.biu_last_error()
try:
    B.set_fp32_products_3d("tf32")
    raise SystemExit("tf32 accepted")
except ValueError:
    pass
# setting one mode never makes the other refuse (neither setter latches anything)
for m2, m3 in [("bf16x3", "bf16x6"), ("exact", "bf16x3"), ("bf16x6", "exact")]:
    B.set_fp32_products(m2)
    B.set_fp32_products_3d(m3)
    B.set_fp32_products_3d("exact")
    B.set_fp32_products("bf16x6")
# a kd = 1 size query latches the 2-D mode only: the 3-D mode stays free, and the 2-D one refuses a change
assert L.lib.biu_conv_packed_bytes(0, 32, 32, 1, 3, 3, 1, L.BIU_F32) > 0
assert L.lib.biu_set_fp32_products(1) != 0 and b"before the first forward" in L.lib.biu_last_error()
for m3 in ("bf16x6", "bf16x3", "exact"):
    B.set_fp32_products_3d(m3)
print("SETTERS ok")
"""


def test_fp32_3d_product_mode_switch_validates_its_argument_and_is_independent_of_the_2d_one():
    r = subprocess.run([sys.executable, "-c", _SETTERS, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SETTERS ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# fp32 packed sizes of a 32 -> 32 layer: 3x3x3 (kd = 3) under the 3-D mode, 3x3 (kd = 1) under the 2-D mode; then try to switch the 3-D mode
_PROBE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import bio_image_unet_amd as B
import bio_image_unet_amd._lib as L
print("SIZE3D", L.lib.biu_conv_packed_bytes(0, 32, 32, 3, 3, 3, 1, L.BIU_F32))
B.set_fp32_products("exact")            # the 3-D latch leaves the 2-D mode free
print("SIZE2D", L.lib.biu_conv_packed_bytes(0, 32, 32, 1, 3, 3, 1, L.BIU_F32))
print("CONVT3D", L.lib.biu_convt_packed_bytes(0, 32, 32, 2, L.BIU_F32))
other = {"exact": "bf16x6", "bf16x3": "exact", "bf16x6": "exact"}[sys.argv[2]]
try:
    B.set_fp32_products_3d(other)
    print("SWITCH ok")
except Exception as e:
    print("SWITCH refused:", e)
B.set_fp32_products_3d(sys.argv[2])
print("SAME ok")
"""


def _probe(env3d, expect_mode):
    env = dict(os.environ, BIU_FP32_PRODUCTS="exact")
    env.pop("BIU_FP32_PRODUCTS_3D", None)
    if env3d is not None:
        env["BIU_FP32_PRODUCTS_3D"] = env3d
    r = subprocess.run([sys.executable, "-c", _PROBE, ROOT, expect_mode], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if " " in ln)
    return out, r.stderr


# 27 taps x 1 KiB per (row tile, k-step): 32 channels are 4 fp32 k-steps, 4 bf16x3 k-steps (2 chunks x 2 parts) or 6 bf16x6 k-steps
@pytest.mark.parametrize("env3d,mode,ksteps", [(None, "exact", 4), ("exact", "exact", 4), ("bf16x3", "bf16x3", 4), ("bf16x6", "bf16x6", 6)])
def test_environment_selects_the_3d_mode_and_a_size_query_latches_it(env3d, mode, ksteps):
    out, err = _probe(env3d, mode)
    assert int(out["SIZE3D"]) == ksteps * 27 * 1024
    assert int(out["CONVT3D"]) == ksteps * 8 * 1024
    assert int(out["SIZE2D"]) == 4 * 9 * 1024          # the 2-D mode (exact here) is untouched by the 3-D one
    assert out["SWITCH"].startswith("refused") and "before the first forward" in out["SWITCH"], out
    assert out["SAME"] == "ok"
    assert not [ln for ln in err.splitlines() if ln.startswith("[biu]")], err


def test_unknown_3d_mode_in_the_environment_is_named_and_ignored():
    out, err = _probe("bogus", "exact")
    assert int(out["SIZE3D"]) == 4 * 27 * 1024          # ignored: the default (exact) holds
    warned = [ln for ln in err.splitlines() if ln.startswith("[biu]")]
    assert len(warned) == 1 and "BIU_FP32_PRODUCTS_3D" in warned[0] and "bogus" in warned[0], err
