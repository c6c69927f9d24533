"""First-layer kernels for 1 to 4 input channels, host side (no GPU): biu_conv_first_ok is arithmetic on the descriptors (fake, 16-byte
aligned addresses that are never dereferenced), biu_conv_first_workspace is positive wherever it says yes, and
biu_conv_bwd_weight_workspace keeps meaning "the MFMA weight gradient takes this layer" (0 for 2 to 4 input channels)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import bio_image_unet_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [L.BIU_BF16, L.BIU_F32]


def act(addr, c, kd, pitch=None):
    a = L.biu_act()
    a.p, a.n, a.d, a.h, a.w, a.c, a.pitch = addr, 2, (6 if kd == 3 else 1), 20, 36, c, pitch or c
    return a


def first_ok(cin, cout, kd, dtype, k=3, dil=1, yaddr=2 << 20, xpitch=None):
    x, y = act(1 << 20, cin, kd, xpitch), act(yaddr, cout, kd)
    return L.lib.biu_conv_first_ok(C.byref(x), C.byref(y), kd, k, k, dil, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kd", [1, 3])
@pytest.mark.parametrize("cout", [16, 32])
@pytest.mark.parametrize("cin", [1, 2, 3, 4])
def test_first_layer_predicate_and_workspace(cin, cout, kd, dtype):
    assert first_ok(cin, cout, kd, dtype) == 1
    assert first_ok(cin, cout, kd, dtype, xpitch=cin + 8) == 1                    # a channel slice of a wider row
    assert L.lib.biu_conv_first_workspace(cin, cout, kd, dtype) > 0
    if cin >= 2:
        assert L.lib.biu_conv_bwd_weight_workspace(cin, 16, kd, 3, 3, dtype) == 0     # as before: no MFMA weight gradient below 16 channels


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kd", [1, 3])
def test_first_layer_predicate_refuses(kd, dtype):
    assert first_ok(5, 16, kd, dtype) == 0
    assert first_ok(2, 16, kd, dtype, dil=2) == 0
    assert first_ok(2, 16, 1, dtype, k=1) == 0
    assert first_ok(2, 4, kd, dtype) == 0
    assert first_ok(2, 16, kd, dtype, yaddr=(2 << 20) + 8) == 0                   # output off the 16-byte grid
    assert L.lib.biu_conv_first_workspace(5, 16, kd, dtype) == 0


_PROBE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import bio_image_unet_amd._lib as L
def act(addr, c):
    a = L.biu_act(); a.p, a.n, a.d, a.h, a.w, a.c, a.pitch = addr, 1, 4, 16, 32, c, c
    return a
y = act(2 << 20, 16)
print("OK", *[L.lib.biu_conv_first_ok(C.byref(act(1 << 20, c)), C.byref(y), 3, 3, 3, 1, L.BIU_BF16) for c in (1, 2, 4)])
print("WS", *[int(L.lib.biu_conv_first_workspace(c, 16, 3, L.BIU_BF16) > 0) for c in (1, 2, 4)])
"""


@pytest.mark.parametrize("disable,ok", [("cn", "1 0 0"), ("c1", "0 0 0"), ("cnx", "1 1 1")])
def test_cn_token_switches_only_the_multi_channel_route(disable, ok):
    """BIU_DISABLE=cn restores the earlier routing for 2 to 4 input channels and leaves one channel alone; c1 covers both (a child
    process: the library reads the environment once)."""
    r = subprocess.run([sys.executable, "-c", _PROBE, ROOT], env=dict(os.environ, BIU_DISABLE=disable), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"OK {ok}" in r.stdout and f"WS {ok}" in r.stdout, r.stdout
