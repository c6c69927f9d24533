"""What ``tests/golden/make_golden_mo3d_blend.py`` (the reference's own stitcher, CPU) and ``tests/test_gpu_mo3d_blend.py`` (``PredictMo3d`` on
the device) share: the geometries, the seeded input volumes and a stub network whose output depends on the position INSIDE the patch.

Per head the stub returns ``a_h * x + b_h * ramp[d, h, w]`` with one fixed, seeded ``ramp`` of the patch extent, repeated over the head's
channels.  Two patches that cover the same voxel therefore predict different values for it, and the blend weights decide what the
stitched volume holds there -- a point-wise stub cannot tell one convex blend from another.  ``a_h, b_h > 0`` and ``x, ramp >= 0``: every term
of the blend is non-negative, which the test's error bound relies on.  Both products and the sum are single IEEE fp32 operations, so the
CPU and the device compute the same patch outputs bit for bit."""
import zlib

import numpy as np
import torch

HEADS = {"a": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss"},
         "b": {"channels": 2, "activation": None, "loss": "DiceLoss"}}
COEF = {"a": (0.5, 0.25), "b": (0.25, 0.75)}           # (a_h, b_h), exact in fp32
RAMP_SEED = 77
BATCH_SIZE = 4

# name -> volume extent, max_patch_size, overlap_factor, volume seed
GEOMETRIES = {
    # N_z = 2 < blend_margin and patch height = width = blend_margin: the ramps fill the patch
    "ramps_fill_patch": dict(volume=(12, 40, 24), patch=(8, 16, 16), overlap=0.25, seed=3),
    # Z = [0, 6, 12], Y = [0, 24, 40], X = [0, 8]: N_z = 3 depth ramp planes, a weight-1 plateau behind the 16-voxel ramps, appended last starts
    "plateau_appended_start": dict(volume=(20, 72, 40), patch=(8, 32, 32), overlap=0.25, seed=4),
}


def make_volume(shape, seed):
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(50)).astype(np.float32)


def volume_checksum(vol):
    return zlib.crc32(np.ascontiguousarray(vol, dtype=np.float32).tobytes())


def make_ramp(extent):
    """float32 [d, h, w] in [0, 1): the position-dependent part of the stub's output."""
    return np.random.default_rng(RAMP_SEED).random(tuple(int(e) for e in extent), dtype=np.float32)


class PositionStub(torch.nn.Module):
    """Takes the reference constructor's keyword arguments; has one parameter so that it has a state_dict and a device."""

    def __init__(self, in_channels=1, n_filter=4, output_heads=None, use_interpolation=True):
        super().__init__()
        self.heads = output_heads
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self._ramp = {}

    def ramp(self, x):
        key = (tuple(x.shape[2:]), x.device)
        if key not in self._ramp:
            self._ramp[key] = torch.from_numpy(make_ramp(x.shape[2:])).to(x.device)
        return self._ramp[key]

    def forward(self, x):
        assert x.dtype == torch.float32 and x.dim() == 5 and x.shape[1] == 1
        r = self.ramp(x)[None, None]
        out = {}
        for k, v in self.heads.items():
            a, b = COEF[k]
            out[k] = torch.add(torch.mul(x, a), torch.mul(r, b)).repeat(1, v["channels"], 1, 1, 1)
        return out


def checkpoint():
    return {"in_channels": 1, "n_filter": 4, "output_heads": HEADS, "use_interpolation": True,
            "state_dict": PositionStub(output_heads=HEADS).state_dict()}
