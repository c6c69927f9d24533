"""``preprocess='device'`` of the five ``Predict`` classes against ``preprocess='host'`` end to end on tiny networks: integer-valued input makes
the patches bit-identical (``tests/test_gpu_preprocess.py``) and the eval forward, the uint8 re-quantisation and the stitching use no float
atomics, so the results must be ``np.array_equal``.

The three uint8 families normalise in float64 on the host: any integer input is bit-equal.  The two multi-output families normalise in
float32 there; for them the input is chosen so that float32 loses nothing the float64 formula keeps: the brightest and the darkest value
are held by well over 0.02 % of the pixels (saturated pixels), so both percentiles are sample values and not interpolated; ``a - min`` of
integers is exact in either type; and the one division is correctly rounded in float32 on the host and rounded to float64 then float32 on
the device, which is the same number (double rounding of a quotient is innocuous when the wide type has at least 2 * 24 + 2 bits).  The
``+ 1e-8`` of the 3-D family vanishes in float32 and perturbs the float64 divisor by 1e-8 / range relative, less than the 2^-25 / range by
which a quotient of two integers below 2^24 stays clear of every float32 rounding boundary it is not exactly on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bio_image_unet_amd as B  # noqa: E402
import bio_image_unet_amd.multi_output_unet as mo2d  # noqa: E402
import bio_image_unet_amd.multi_output_unet3d as mo3d  # noqa: E402
import bio_image_unet_amd.siam_unet as siam  # noqa: E402
import bio_image_unet_amd.unet as unet  # noqa: E402
import bio_image_unet_amd.unet3d as unet3d  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "flow": {"channels": 2, "activation": "tanh", "loss": "DiceLoss", "weight": 0.5}}


def _randomise_bn(sd):
    g = torch.Generator().manual_seed(9)
    sd = {k: v.detach().cpu().clone() for k, v in sd.items()}
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        if k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    return sd


def _saturated(shape, seed, top=200):
    """Integers in [0, top] with about 2 % of the pixels at each end."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, top + 1, shape)
    u = rng.random(shape)
    x[u < 0.02] = 0
    x[u > 0.98] = top
    return x.astype(np.uint16)


def _both(make):
    host, dev = make("host"), make("device")
    return host, dev


@pytest.mark.parametrize("mode,invert", [("single", False), ("first", True), ("all", False)])
def test_predict2d(mode, invert):
    ck = {"n_filter": 4, "in_channels": 1, "out_channels": 1, "state_dict": _randomise_bn(O.init_unet2d(1, 1, 4, seed=5))}
    imgs = np.random.default_rng(0).integers(30, 9000, (2, 50, 70)).astype(np.uint16)
    host, dev = _both(lambda pp: unet.Predict(imgs.copy(), None, ck, network="Unet", resize_dim=(32, 48), add_tile=1, invert=invert,
                                              normalization_mode=mode, clip_threshold=(0.2, 99.8), show_progress=False, device="cuda",
                                              batch_size=4, preprocess=pp))
    assert dev.imgs_result.shape == (2, 50, 70) and dev.imgs_result.dtype == np.uint8 and dev.imgs_result.std() > 0
    assert np.array_equal(host.imgs_result, dev.imgs_result)
    assert (dev.N_x, dev.N_y, list(dev.X_start), list(dev.Y_start)) == (host.N_x, host.N_y, list(host.X_start), list(host.Y_start))


def test_predict2d_tile_larger_than_image():
    ck = {"n_filter": 4, "in_channels": 1, "out_channels": 1, "state_dict": _randomise_bn(O.init_unet2d(1, 1, 4, seed=5))}
    imgs = np.random.default_rng(1).integers(0, 4000, (1, 37, 53)).astype(np.int16)
    host, dev = _both(lambda pp: unet.Predict(imgs.copy(), None, ck, resize_dim=(48, 64), show_progress=False, device="cuda", preprocess=pp))
    assert dev.imgs_result.shape == (37, 53) and np.array_equal(host.imgs_result, dev.imgs_result)


def test_predict3d():
    ck = {"n_filter": 4, "in_channels": 1, "out_channels": 1, "state_dict": _randomise_bn(O.init_unet3d(1, 1, 4, seed=6))}
    vol = np.random.default_rng(2).integers(0, 500, (20, 40, 36)).astype(np.uint16)
    host, dev = _both(lambda pp: unet3d.Predict(vol.copy(), None, ck, resize_dim=(8, 16, 16), add_patch=0, progress_bar=False, device="cuda",
                                                preprocess=pp))
    assert dev.vol_result.shape == vol.shape and dev.vol_result.std() > 0
    assert np.array_equal(host.vol_result, dev.vol_result)


@pytest.mark.parametrize("mode", ["single", "first", "all"])
def test_predict_siam(mode):
    ck = {"n_filter": 4, "mode": "max", "state_dict": _randomise_bn(O.init_unet2d(1, 1, 4, seed=7, siam_mode="max"))}
    movie = np.random.default_rng(3).integers(0, 300, (3, 40, 48)).astype(np.uint8 if mode == "all" else np.uint16)
    host, dev = _both(lambda pp: siam.Predict(movie.copy(), None, ck, resize_dim=(32, 32), add_tile=0, normalization_mode=mode,
                                              clip_threshold=(0.2, 99.8), show_progress=False, device="cuda", preprocess=pp))
    assert dev.imgs_result.shape == movie.shape and dev.imgs_result.std() > 0
    assert np.array_equal(host.imgs_result, dev.imgs_result)


@pytest.mark.parametrize("mode", ["single", "all"])
def test_predict_mo3d(mode):
    torch.manual_seed(5)
    net = B.MultiOutputUnet3D(in_channels=1, output_heads=HEADS, n_filter=4, use_interpolation=True)
    ck = {"n_filter": 4, "in_channels": 1, "output_heads": HEADS, "use_interpolation": True, "state_dict": _randomise_bn(net.state_dict())}
    vol = _saturated((12, 40, 24), 4)
    host, dev = _both(lambda pp: mo3d.Predict(vol.copy(), ck, result_path=None, max_patch_size=(8, 16, 16), overlap_factor=0.25, batch_size=3,
                                              normalization_mode=mode, show_progress=False, device="cuda", preprocess=pp))
    for k in HEADS:
        assert dev.result[k].shape == host.result[k].shape and np.isfinite(dev.result[k]).all() and dev.result[k].std() > 0
        assert np.array_equal(host.result[k], dev.result[k]), k


@pytest.mark.parametrize("mode", ["single", "first"])
def test_predict_mo2d(mode):
    torch.manual_seed(6)
    net = B.MultiOutputNestedUNet(in_channels=1, output_heads=HEADS, n_filter=4, deep_supervision=False, train_mode=False)
    ck = {"n_filter": 4, "in_channels": 1, "output_heads": HEADS, "deep_supervision": False, "state_dict": _randomise_bn(net.state_dict())}
    imgs = _saturated((2, 50, 80), 5)
    host, dev = _both(lambda pp: mo2d.Predict(imgs.copy(), ck, max_patch_size=(48, 48), batch_size=4, normalization_mode=mode,
                                              show_progress=False, device="cuda", preprocess=pp))
    assert dev.patch_size == host.patch_size == (48, 48) and (dev.N_x, dev.N_y) == (2, 2)
    for k in HEADS:
        assert dev.result[k].shape == host.result[k].shape and np.isfinite(dev.result[k]).all() and dev.result[k].std() > 0
        assert np.array_equal(host.result[k], dev.result[k]), k


def test_unknown_preprocess_and_nan_raise():
    ck = {"n_filter": 4, "in_channels": 1, "out_channels": 1, "state_dict": O.init_unet2d(1, 1, 4, seed=5)}
    imgs = np.random.default_rng(7).random((2, 40, 48)).astype(np.float32)
    for cls, kw in ((unet.Predict, dict(result_name=None)), (unet3d.Predict, dict(result_name=None)), (siam.Predict, dict(result_name=None)),
                    (mo3d.Predict, {}), (mo2d.Predict, {})):
        with pytest.raises(ValueError, match="preprocess 'gpu' not valid"):
            cls(imgs, model_params=ck, device="cuda", preprocess="gpu", **kw)
    bad = imgs.copy()
    bad[1, 5, 6] = np.nan
    with pytest.raises(ValueError, match='preprocess="host"'):
        unet.Predict(bad, None, ck, resize_dim=(32, 32), show_progress=False, device="cuda", preprocess="device")
    with pytest.raises(ValueError, match='preprocess="host"'):
        mo2d.Predict(bad, ck, max_patch_size=(32, 32), device="cuda", preprocess="device")
    with pytest.raises(ValueError, match='preprocess="host"'):
        unet.Predict(imgs.astype(np.float64) + 1e-12, None, ck, resize_dim=(32, 32), show_progress=False, device="cuda", preprocess="device")
