"""The five Trainers on the CPU: what each family states on top of the shared epoch loop (``workflow._EpochLoop``) -- the checkpoint
dictionary, key for key and in order, the scheduler and the gradient clip.  No GPU: construction and ``_checkpoint`` launch nothing."""
import pytest
import torch

from bio_image_unet_amd import workflow as W

KEYS = {
    "2d": "epoch, best_loss, state_dict, optimizer, lr, loss_function, loss_params, n_filter, dilation, batch_size, augmentation, in_channels, "
          "out_channels, clip_threshold, noise_lims, brightness_contrast, shiftscalerotate",
    "3d": "val_loss, epoch, best_loss, state_dict, optimizer, lr, loss_function, loss_params, time_loss_weight, n_filter, use_interpolation, "
          "dilation, batch_size, augmentation, in_channels, out_channels, clip_threshold, noise_amp, brightness_contrast, shiftscalerotate",
    "siam": "epoch, best_loss, state_dict, optimizer, lr, loss, loss_params, n_filter, mode, augmentation, clip_threshold, noise_amp, "
            "brightness_contrast, shiftscalerotate",
    "mo3d": "epoch, epoch_start, best_loss, state_dict, optimizer, lr, loss_function, loss_params, time_loss_weight, n_filter, use_interpolation, "
            "dilation, batch_size, augmentation, clip_threshold, scale_limit, rotate_limit, gauss_noise_lims, shot_noise_lims, blur_limit, "
            "random_rotate, brightness_contrast, in_channels, output_heads",
    "mo2d": "epoch, epoch_start, best_loss, state_dict, optimizer, lr, n_filter, deep_supervision, dilation, batch_size, augmentation, "
            "clip_threshold, gauss_noise_lims, shot_noise_lims, brightness_contrast, random_rotate, in_channels, output_heads",
}
# family: (patience, factor, gradient clip, the 'optimizer' entry is the construction-time state)
LOOP = {"2d": (4, 0.1, None, True), "3d": (4, 0.1, None, True), "siam": (4, 0.1, None, False), "mo3d": (5, 0.2, 1.0, True), "mo2d": (5, 0.2, 1.0, True)}
HEADS3D = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0}}
HEADS2D = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
           "distance": {"channels": 1, "activation": None, "loss": "MSELoss", "weight": 0.5}}


class _Items(torch.utils.data.Dataset):
    """Ten tiny in-memory items with the reference's attributes; every attribute a checkpoint records has its own value."""
    aug_factor, clip_threshold, brightness_contrast = 3, (0.1, 99.9), (0.15, 0.25)
    noise_lims, noise_amp, shiftscalerotate = (0.4, 1.1), 7, (0.05, 0.1, 20)
    scale_limit, rotate_limit, gauss_noise_lims, shot_noise_lims, blur_limit, random_rotate = (0, 0.2), 30, (0.01, 0.2), (0.001, 0.02), (3, 5), False

    def __init__(self, shape, keys):
        self.dim_out, self.keys = shape, keys

    def __len__(self):
        return 10

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(i)
        return {k: torch.rand(self.dim_out, generator=g) for k in self.keys}


def _trainer(family, save_dir):
    kw = dict(batch_size=2, save_dir=str(save_dir), device="cpu")
    if family == "2d":
        return W.Trainer2D(_Items((16, 16), ("image", "mask")), 1, n_filter=4, **kw)
    if family == "3d":
        return W.Trainer3D(_Items((8, 16, 16), ("volume", "mask")), 1, n_filter=4, **kw)
    if family == "siam":
        return W.TrainerSiam(_Items((16, 16), ("image", "prev_image", "mask")), 1, n_filter=4, **kw)
    if family == "mo3d":
        return W.TrainerMo3d(_Items((8, 16, 16), ("volume", "mask")), HEADS3D, 1, n_filter=4, **kw)
    return W.TrainerMo2d(_Items((16, 16), ("image", "mask", "distance")), 1, output_heads=HEADS2D, n_filter=4, **kw)


@pytest.mark.parametrize("family", sorted(KEYS))
def test_checkpoint_dictionary_and_loop_settings(family, tmp_path):
    torch.manual_seed(0)
    tr = _trainer(family, tmp_path)
    assert isinstance(tr, W._EpochLoop)
    built = tr.optimizer.state_dict()                      # what a checkpoint of a refreshing family would hold
    ck = tr._checkpoint(2, torch.tensor(0.25))
    assert list(ck) == KEYS[family].split(", ")
    assert "online_augmentation" not in ck and tr.augmenter is None
    patience, factor, clip, construction_time = LOOP[family]
    assert (tr.scheduler.patience, tr.scheduler.factor, tr.grad_clip) == (patience, factor, clip)
    if construction_time:
        assert ck["optimizer"] is tr.params["optimizer"] and tr._checkpoint(3, torch.tensor(0.5))["optimizer"] is ck["optimizer"]
    else:
        assert not hasattr(tr, "params") and ck["optimizer"] is not tr._checkpoint(3, torch.tensor(0.5))["optimizer"]
    assert ck["optimizer"]["param_groups"][0]["lr"] == built["param_groups"][0]["lr"] == tr.lr == ck["lr"]
    # the leading entries, and every value the data set or the constructor supplies
    ds = tr.data
    assert ck["epoch"] == 2 and ck["best_loss"] is tr.best_loss and torch.isinf(ck["best_loss"])
    assert set(ck["state_dict"]) == set(tr.model.state_dict()) and ck["n_filter"] == 4 and ck["augmentation"] == 3
    assert ck["clip_threshold"] == ds.clip_threshold and ck["brightness_contrast"] == ds.brightness_contrast
    if family in ("2d", "3d", "siam"):
        assert ck["shiftscalerotate"] == ds.shiftscalerotate
        assert ck["noise_lims"] == ds.noise_lims if family == "2d" else ck["noise_amp"] == ds.noise_amp
    if family == "3d":
        assert float(ck["val_loss"]) == 0.25 and ck["time_loss_weight"] == 0.1 and ck["use_interpolation"] is False
    if family == "siam":
        assert ck["loss"] == "BCEDice" and ck["loss_params"] == (1, 1) and ck["mode"] == "max"
    if family in ("mo3d", "mo2d"):
        assert ck["epoch_start"] == 0 and ck["output_heads"] is (HEADS3D if family == "mo3d" else HEADS2D) and ck["in_channels"] == 1
        assert ck["gauss_noise_lims"] == ds.gauss_noise_lims and ck["shot_noise_lims"] == ds.shot_noise_lims and ck["random_rotate"] is False
    if family == "mo3d":
        assert ck["scale_limit"] == ds.scale_limit and ck["rotate_limit"] == 30 and ck["blur_limit"] == ds.blur_limit
    if family == "mo2d":
        assert ck["deep_supervision"] is False and ck["dilation"] is False and ck["lr"] == 1e-4


def test_multi_output_trainers_share_one_activation_and_count_epochs_on(tmp_path):
    assert W.TrainerMo2d._apply_activation is W.TrainerMo3d._apply_activation
    x = torch.tensor([[-1.0, 2.0]])
    assert torch.equal(W.TrainerMo2d._apply_activation(x, "relu"), torch.relu(x)) and W.TrainerMo3d._apply_activation(x, None) is x
    assert torch.equal(W.TrainerMo2d._apply_activation(x, "softmax"), torch.softmax(x, dim=1))
    # load_weights: the multi-output families count epochs on from the checkpoint (file names, 'epoch'), the others start at 0
    for family in ("mo3d", "2d"):
        d = tmp_path / family
        torch.manual_seed(0)
        tr = _trainer(family, d)
        tr.state = tr._checkpoint(4, torch.tensor(0.5))
        tr._save(tr.save_name)
        again = type(tr)(tr.data, *((HEADS3D, 1) if family == "mo3d" else (1,)), n_filter=4, batch_size=2, save_dir=str(d), device="cpu", load_weights=True)
        assert again.epoch_start == (4 if family == "mo3d" else 0)
        assert again._checkpoint(1, torch.tensor(0.5))["epoch"] == (5 if family == "mo3d" else 1)
        assert all(torch.equal(v, tr.model.state_dict()[k]) for k, v in again.model.state_dict().items())
