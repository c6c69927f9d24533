"""What ``tests/golden/make_golden_predict_pins.py`` (the reference's own ``Predict`` constructors, CPU), ``tests/test_predict_pins_host.py``
(the port's host arithmetic) and ``tests/test_gpu_predict_pins.py`` (the port's ``Predict`` classes on the device) share: the named
geometries, the seeded inputs with a crc32 of their bytes, and stub networks whose output depends on the position INSIDE the patch.

Every stub adds ``b * ramp`` to a multiple of its input, ``ramp`` one seeded float32 array of the patch extent in [0, 1).  Two tiles that
cover the same pixel therefore predict different values for it and the stitcher decides what the result holds there: the overwrite order
of the 3-D layers, the safe-margin weights and the fill of the 2-D multi-output family, the origins of all of them.  Every coefficient is
a power of two, so the products are exact and each ``torch.add`` rounds once: the CPU (the recipe) and the device (the test) compute the
same bits, fused or not.  uint8 patches (what the port hands its network) are divided by a 255.0 TENSOR, a correctly rounded division on
both sides, which is ``patch.astype('float32') / 255`` of the reference.  All outputs lie in [0, 1) and are non-negative."""
import zlib

import numpy as np
import torch

RAMP_SEED = 91
# (a, b) per output channel: out = a * x + b * ramp
COEF_U8 = ((0.5, 0.25), (0.25, 0.5))
COEF_SIAM = (0.5, 0.25, 0.125)                          # current frame, previous frame, ramp: the two frames count differently
HEADS = {"a": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss"},
         "b": {"channels": 2, "activation": None, "loss": "DiceLoss"}}
COEF_HEADS = {"a": ((0.5, 0.25),), "b": ((0.25, 0.5), (0.5, 0.125))}
MO2D_BATCH = 3

# family -> name -> settings.  ``dtype`` is the input's; ``seed`` makes it (make_input).
GEOMETRIES = {
    "unet": {
        # 3 x 4 tiles, X_start [0 10 21], Y_start [0 17 35 53]: linspace origins that truncate
        "truncated_linspace": dict(shape=(2, 53, 101), dtype="float32", seed=11, resize_dim=(32, 48), add_tile=1, mode="single", invert=False,
                                   out_channels=1),
        # rows reflect-padded 20 -> 32, inverted, two output channels with their own coefficients
        "reflect_rows_two_channels": dict(shape=(1, 20, 100), dtype="uint16", seed=12, resize_dim=(32, 48), add_tile=0, mode="single", invert=True,
                                          out_channels=2),
        "first": dict(shape=(3, 40, 64), dtype="uint16", seed=13, resize_dim=(32, 32), add_tile=0, mode="first", invert=False, out_channels=1),
        "all": dict(shape=(3, 40, 64), dtype="uint16", seed=13, resize_dim=(32, 32), add_tile=0, mode="all", invert=False, out_channels=1),
    },
    "unet3d": {
        # N_z, N_x, N_y = 4, 6, 5 (add_patch compounds on N_x): 120 patches, voxels under more than three of them
        "compounded_add_patch": dict(shape=(20, 40, 36), dtype="uint16", seed=21, resize_dim=(8, 16, 16), add_patch=1, invert=False),
        # 1, 1, 3 patches, reflect padding in z and x
        "reflect_z_x": dict(shape=(6, 20, 36), dtype="float32", seed=22, resize_dim=(8, 32, 16), add_patch=0, invert=False),
    },
    "siam": {
        "pairs_2x2": dict(shape=(3, 40, 48), dtype="uint16", seed=31, resize_dim=(32, 32), add_tile=0, mode="single", invert=False),
        "constant_padding": dict(shape=(3, 20, 24), dtype="uint16", seed=32, resize_dim=(32, 32), add_tile=0, mode="all", invert=False),
        # a one-frame movie is paired with itself; 3 x 3 tiles
        "one_frame": dict(shape=(1, 40, 48), dtype="uint16", seed=33, resize_dim=(32, 32), add_tile=1, mode="single", invert=False),
    },
    "mo2d": {
        # 2 x 2 tiles, X_start [0 2], Y_start [0 32]: the columns between the safe margins get the fill
        "fill_2x2": dict(shape=(2, 50, 80), dtype="uint16", seed=41, max_patch_size=(48, 48), add_tile=0),
        # X_start [0 26 53]: rows cut at 0, 26, 52 and stitched at 0, 26, 53
        "drift": dict(shape=(1, 101, 150), dtype="uint16", seed=42, max_patch_size=(48, 64), add_tile=0),
        # N_x x N_y = 3 x 4, the stride yields 4 x 4 windows: one surplus row of windows, predicted (it counts in the fill) and not stitched
        "row_surplus": dict(shape=(1, 51, 100), dtype="uint16", seed=43, max_patch_size=(48, 48), add_tile=1),
        # patch (32, 48), reflect padding, one tile, no margins
        "one_tile_reflect": dict(shape=(1, 30, 40), dtype="float32", seed=44, max_patch_size=(48, 48), add_tile=0),
        # the transposed case: one surplus COLUMN of windows, which upstream's reshape scrambles; PredictMo2d refuses it
        "column_surplus": dict(shape=(1, 100, 51), dtype="uint16", seed=45, max_patch_size=(48, 48), add_tile=1),
    },
}
# PredictMo2d raises ValueError for these; their fixtures record what upstream computes
MO2D_REFUSED = ("column_surplus",)


def make_input(geo):
    rng = np.random.default_rng(geo["seed"])
    if geo["dtype"] == "uint16":
        return rng.integers(100, 60000, geo["shape"]).astype(np.uint16)
    return (rng.random(geo["shape"], dtype=np.float32) * np.float32(900) + np.float32(17)).astype(np.float32)


def crc32(arr):
    return zlib.crc32(np.ascontiguousarray(arr).tobytes())


def make_ramp(extent):
    """float32 in [0, 1) of the patch's spatial extent: the position-dependent part of every stub's output."""
    return np.random.default_rng(RAMP_SEED).random(tuple(int(e) for e in extent), dtype=np.float32)


def _unit(t):
    """uint8 patches as the port hands them over -> float32 ``byte / 255``, correctly rounded (a tensor divisor: torch's GPU division by a
    Python scalar multiplies by the rounded reciprocal instead)."""
    return torch.div(t.float(), torch.full((), 255.0, device=t.device)) if t.dtype == torch.uint8 else t


class _Positional(torch.nn.Module):
    """One parameter, so that there is a state_dict and a device; the ramp of the patch extent, per device."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self._ramp = {}

    def ramp(self, x):
        key = (tuple(x.shape[2:]), x.device)
        if key not in self._ramp:
            self._ramp[key] = torch.from_numpy(make_ramp(x.shape[2:])).to(x.device)[None, None]
        return self._ramp[key]


class StubU8(_Positional):
    """The 2-D and 3-D uint8 families: [B, 1, (D,) H, W] -> (prob, logits) of ``out_channels`` channels."""

    def __init__(self, n_filter=4, in_channels=1, out_channels=1, use_interpolation=False):
        super().__init__()
        self.out_channels = out_channels

    def forward(self, x):
        x = _unit(x)
        assert x.dtype == torch.float32 and x.shape[1] == 1
        r = self.ramp(x)
        p = torch.cat([torch.add(torch.mul(x, a), torch.mul(r, b)) for a, b in COEF_U8[:self.out_channels]], dim=1)
        return p, p


class StubSiam(_Positional):
    def __init__(self, n_filter=4, mode="max"):
        super().__init__()

    def forward(self, cur, prev):
        cur, prev = _unit(cur), _unit(prev)
        assert cur.dtype == prev.dtype == torch.float32 and cur.shape == prev.shape and cur.shape[1] == 1
        a, b, c = COEF_SIAM
        p = torch.add(torch.add(torch.mul(cur, a), torch.mul(prev, b)), torch.mul(self.ramp(cur), c))
        return p, p


class StubHeads2D(_Positional):
    def __init__(self, in_channels=1, n_filter=4, output_heads=None, deep_supervision=False, train_mode=False, dilation=False):
        super().__init__()
        self.heads = output_heads

    def forward(self, x):
        assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 1
        r = self.ramp(x)
        return {k: torch.cat([torch.add(torch.mul(x, a), torch.mul(r, b)) for a, b in COEF_HEADS[k]], dim=1) for k in self.heads}


def checkpoint(family, geo):
    if family in ("unet", "unet3d"):
        oc = geo.get("out_channels", 1)
        return {"n_filter": 4, "in_channels": 1, "out_channels": oc, "state_dict": StubU8(out_channels=oc).state_dict()}
    if family == "siam":
        return {"n_filter": 4, "mode": "max", "state_dict": StubSiam().state_dict()}
    return {"in_channels": 1, "n_filter": 4, "output_heads": HEADS, "deep_supervision": False,
            "state_dict": StubHeads2D(output_heads=HEADS).state_dict()}


def meta():
    """What the fixtures record of this module; the tests compare it with what they import."""
    return {"ramp_seed": RAMP_SEED, "coef_u8": [list(c) for c in COEF_U8], "coef_siam": list(COEF_SIAM), "heads": HEADS,
            "coef_heads": {k: [list(c) for c in v] for k, v in COEF_HEADS.items()}, "mo2d_batch": MO2D_BATCH,
            "geometries": {f: {n: {k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items()} for n, g in fam.items()}
                           for f, fam in GEOMETRIES.items()}}
