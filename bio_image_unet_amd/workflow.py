"""Trainer / Predict counterparts: the host-side callers of the hot path.

They keep the reference's constructor signatures, attribute names, checkpoint dictionary and -- deliberately -- its
numerics-relevant quirks, so a training run is step-for-step comparable:

* 2-D loss indexes the *batch* axis with the channel index and validation only counts the last batch
  (``unet/train.py:133-134,151-153``); the mask ``.view`` uses ``dim[0]`` twice (``:128``).
* 3-D adds ``SmoothL1(y_logits[1:], y_logits[:-1]) * time_loss_weight`` across the *batch* axis; validation hard-codes 0.1
  (``unet3d/train.py:140-145,163-169``).
* No ``model.eval()`` during validation: BatchNorm keeps using (and updating) batch statistics under ``no_grad``.
* ``DataLoader(shuffle=False, drop_last=True, num_workers=0, pin_memory=True)``; unseeded ``random_split``.
* The saved ``'optimizer'`` entry is the construction-time state (2-D / 3-D), never refreshed.

What differs by design: the network class comes from this package (every layer a HIP kernel), the optimizer is the fused
``biu_adam_step``, and data sets are any ``torch.utils.data.Dataset`` yielding the reference's dict items (TIFF I/O is out of scope; all five Trainers
take ``augment=True`` to augment the training batches of a ``feed.TileStore`` on the device, ``augment.py``).

Layout: all five Trainers sit on ``_EpochLoop`` (construction tail, batch loop, validation loop, epoch driver); a family is its constructor,
a few class attributes (scheduler, gradient clip, which lines it prints), ``_forward_loss`` (``_total_loss`` on the two multi-output families,
which share ``_MultiHeadLoop``), ``_checkpoint(epoch, val_loss)`` -- the dictionary it saves -- and ``_report`` where its text differs.

All five Predicts sit on ``_PredictBase`` (opening the input, loading checkpoint and network, the ``no_grad`` batch iterator, where a patch
is stitched) and run in one order: input, geometry and patches, model, batch loop into ``_Stitcher``s in HBM, crop and write.  A family is
its constructor signature, ``_origins`` -- its tile grid, the one list that both cuts the patches and places them in the stitch --, its host
normalisation and ``_split`` (one line over ``_cut``), ``_build(model_params, network)`` and what it does with one predicted patch; the two
multi-output families share ``_HeadStitch`` (a stitcher per head and image, the weight arrays by neighbour flags).  Every Predict takes
``preprocess='host'`` (numpy, the default) or ``'device'``: the raw stack is uploaded once in its own dtype and percentiles, rescale,
padding and tiling run in HBM (``preprocess.DeviceFrontEnd``) over the same ``_origins``; its docstring states where the two differ
(float32 input of the float32-arithmetic host paths, NaN, float64 that float32 cannot hold).
"""
from __future__ import annotations

import os
from typing import Optional, Union

import numpy as np
import torch
from torch import nn, optim
from torch.utils.data import DataLoader, random_split

from ._lib import check, lib, ptr, stream
from .losses import BCEDiceLoss, BCEDiceLossSiam, BCEDiceTemporalLoss, TverskyLoss, logcoshTverskyLoss, weightedBCELoss
from .models import AttentionUnet, MultiOutputNestedUNet, MultiOutputUnet3D, Siam_UNet, UNet3D, Unet, Unet_v0
from .optim import Adam
from .preprocess import DeviceFrontEnd
from .utils import get_device, init_weights

try:                                    # progress bars are cosmetic
    from tqdm import tqdm
except Exception:                       # pragma: no cover
    def tqdm(it, **_):
        return it


def _pick_device(device):
    return get_device() if device == "auto" else torch.device(device)


def _make_criterion(name, params, extra=None):
    table = {"BCEDice": BCEDiceLoss, "Tversky": TverskyLoss, "logcoshTversky": logcoshTverskyLoss}
    if extra:
        table.update(extra)
    if name not in table:
        raise ValueError(f'Loss "{name}" not defined!')
    return table[name](params[0], params[1])


def _resolve_augment(augment, dataset, device, recipe):
    """``augment`` keyword of the Trainers -> ``augment.Augmenter`` (the uint8 families), ``augment.AugmenterF32`` (recipe ``"mo2d"``),
    ``augment.AugmenterVol`` (recipe ``"mo3d"``) or None.
    On-device augmentation works on the batches of a ``DeviceFeeder``, so anything but a ``TileStore`` on a GPU is refused rather than
    silently trained un-augmented.  A ``feed.ImageStore`` (whole items, recipe ``"mo2d"`` only) or ``feed.VolumeStore`` (whole volumes, recipe
    ``"mo3d"`` only) is always augmented: ``None`` means ``True``."""
    from .feed import ImageStore
    if isinstance(dataset, ImageStore):
        # whole items: every patch is a random crop rendered on the device, so None means True here
        from .augment import AugmenterF32, AugmenterVol
        cls, store = {"mo2d": AugmenterF32, "mo3d": AugmenterVol}[dataset.recipe], type(dataset).__name__
        if recipe != dataset.recipe or torch.device(device).type != "cuda":
            raise ValueError(f'augment: a feed.{store} is the data set of recipe "{dataset.recipe}" '
                             f'({"TrainerMo2d" if dataset.recipe == "mo2d" else "TrainerMo3d"}) on a GPU device')
        if augment is None or augment is True:
            return cls.from_store(dataset, recipe)
        if not isinstance(augment, cls):
            raise ValueError(f"augment: None, True or an augment.{cls.__name__} (such a store cannot be trained un-augmented)")
        return augment
    if augment is None or augment is False:
        return None
    from .augment import Augmenter, AugmenterF32, AugmenterVol
    from .feed import TileStore
    cls = {"mo2d": AugmenterF32, "mo3d": AugmenterVol}.get(recipe, Augmenter)
    if not isinstance(dataset, TileStore) or torch.device(device).type != "cuda":
        raise ValueError("augment: on-device augmentation needs a feed.TileStore data set and a GPU device")
    if augment is True:
        return cls.from_store(dataset, recipe)
    if not isinstance(augment, cls):
        raise ValueError(f"augment: None, True or an augment.{cls.__name__}")
    return augment


def _loaders(dataset, train_data, val_data, batch_size, device, augmenter=None):
    """The reference's loaders (``DataLoader(shuffle=False, drop_last=True, num_workers=0, pin_memory=True)``, unet/train.py:92-93)
    -- or, for a memory-mapped ``feed.TileStore``, asynchronous uint8 feeders over the same index split (same order, same
    batches; the tiles cross PCIe as bytes while the previous step computes)."""
    from .feed import CropFeeder, DeviceFeeder, ImageStore, TileStore
    if isinstance(dataset, ImageStore):
        # patches of whole items (ImageStore, or its 3-D subclass VolumeStore): training crops are drawn with the running epoch, validation
        # crops with one fixed epoch key -- fully augmented but the same every epoch, as the reference's validation patches are augmented
        # once and then fixed
        from .augment import VALIDATION_EPOCH
        # cubic-spline targets: the tables of the store's "mask" fields, built once and shared by both feeders
        spline = (dataset.spline_tables(device, augmenter.spline_fields(dataset))
                  if getattr(augmenter, "target_interp", "linear") == "cubic" else None)
        return (CropFeeder(dataset, train_data.indices, batch_size, device, augmenter, spline=spline),
                CropFeeder(dataset, val_data.indices, batch_size, device, augmenter, epoch_key=VALIDATION_EPOCH, spline=spline))
    if isinstance(dataset, TileStore) and torch.device(device).type == "cuda":
        return (DeviceFeeder(dataset, train_data.indices, batch_size, device, augmenter=augmenter),     # training only, never validation
                DeviceFeeder(dataset, val_data.indices, batch_size, device))
    return (DataLoader(train_data, batch_size=batch_size, pin_memory=True, drop_last=True),
            DataLoader(val_data, batch_size=batch_size, pin_memory=True, drop_last=True))


def _target(t: torch.Tensor) -> torch.Tensor:
    """Targets arrive as float32 in [0, 1] (reference items) or as uint8 0..255 from a DeviceFeeder."""
    if t.dtype == torch.uint8:
        from .feed import u8_to_float
        return u8_to_float(t)
    return t


class _gc_paused:
    """The batch loop of an epoch runs with Python's cyclic garbage collector paused (restored, and run once, at the end): the host
    enqueues a step in 3-4 ms and runs only a few steps ahead of the GPU, while a generation-2 collection -- it walks every object torch
    has imported -- stalls it for 60-140 ms, i.e. the GPU idles for the length of 10-20 short steps (measured on ``Unet(1,1,32)`` at 2 x 256^2:
    one step in twenty took 60-115 ms instead of 4.9).  A training step creates no reference cycles; reference counting frees what it allocates."""

    def __enter__(self):
        import gc
        self.was = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self.was:
            gc.enable()
            gc.collect()
        return False


def _set_fp32_products(mode, three_d=False):
    """``fp32_products`` keyword of the Trainers: process-wide, ``None`` leaves the process's mode alone."""
    if mode is not None:
        from . import set_fp32_products, set_fp32_products_3d
        (set_fp32_products_3d if three_d else set_fp32_products)(mode)


class _EpochLoop:
    """The one loop under the five Trainers: split, loaders, Adam + ReduceLROnPlateau, the training batch loop, the validation loop and the
    epoch driver with best-validation checkpointing.  A family states what is its own as the class attributes below and provides
    ``_forward_loss(batch, validating) -> loss``, ``_checkpoint(epoch, val_loss) -> dict`` and, where its text differs, ``_report``."""
    patience, factor = 4, 0.1           # ReduceLROnPlateau
    grad_clip = None                    # max norm for clip_grad_norm_ between backward() and step()
    announces = True                    # "Starting training / validation epoch ..." lines
    validates_last_batch = False        # Trainer2D: the validation loss is the last batch's, not the mean
    resumes_epoch = False               # load_weights continues the checkpoint's epoch count (epoch_start)
    reads_loss = False                  # TrainerMo2d: the criterion keeps the step's loss for one host read per step
    writer = None                       # TrainerMo2d: tensorboard SummaryWriter, when it imports

    def _setup(self, dataset, num_epochs, batch_size, lr, val_split, save_dir, save_name, save_iter, augmenter=None, load_from=None):
        self.data, self.num_epochs, self.batch_size, self.lr = dataset, num_epochs, batch_size, lr
        self.best_loss = torch.tensor(float("inf"))
        self.save_iter, self.save_dir, self.save_name = save_iter, save_dir, save_name
        n_val = int(len(dataset) * val_split)
        train_data, val_data = random_split(dataset, [len(dataset) - n_val, n_val])
        self.augmenter = augmenter
        self.train_loader, self.val_loader = _loaders(dataset, train_data, val_data, batch_size, self.device, augmenter)
        self.optimizer = Adam(self.model.parameters(), lr=lr)
        self.scheduler = optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, mode="min", patience=self.patience, factor=self.factor)
        os.makedirs(save_dir, exist_ok=True)
        self.epoch_start = 0
        if load_from is not None:
            self.state = torch.load(load_from)
            self.model.load_state_dict(self.state["state_dict"])
            if self.resumes_epoch:
                self.epoch_start = self.state["epoch"]

    def _data_attr(self, *names):
        return {n: getattr(self.data, n, None) for n in names}

    def _augment_entry(self):
        """Checkpoint entry of on-device augmentation; nothing when it is off, so those checkpoints keep their keys."""
        return {} if self.augmenter is None else {"online_augmentation": self.augmenter.describe()}

    def _train_epoch(self, epoch):
        if self.announces:
            print("\nStarting training epoch %s ..." % epoch)
        clip, reads_loss, running = self.grad_clip, self.reads_loss, 0.0
        with _gc_paused():
            for batch in tqdm(self.train_loader, total=len(self.train_loader), unit="batch"):
                loss = self._forward_loss(batch, validating=False)
                self.optimizer.zero_grad()
                loss.backward()
                if clip is not None:
                    self.optimizer.clip_grad_norm_(clip)        # multi_output_unet/train.py:186, multi_output_unet3d/train.py:201, as three launches (biu_grad_clip)
                self.optimizer.step()
                if reads_loss:
                    running += self.criterion.item()             # total_loss.item() (multi_output_unet/train.py:189): the step's one host read
        if self.writer is not None:
            self.writer.add_scalar("Loss/train", running / max(len(self.train_loader), 1), epoch + self.epoch_start)

    def _validate(self, epoch):
        if self.announces:
            print("\nStarting validation epoch %s ..." % epoch)
        losses = []
        with torch.no_grad():
            for batch in tqdm(self.val_loader, total=len(self.val_loader), unit="batch"):
                losses.append(self._forward_loss(batch, validating=True).detach())
                if self.reads_loss:
                    self.criterion.check_range()
        if self.validates_last_batch:           # reference: appended once, after the loop -> last batch only
            losses = losses[-1:]
        val_loss = torch.stack(losses).mean()
        if self.writer is not None:
            self.writer.add_scalar("Loss/val", val_loss.item(), epoch + self.epoch_start)
        return val_loss

    def iterate(self, epoch, mode):
        return self._train_epoch(epoch) if mode == "train" else self._validate(epoch)

    def _report(self, epoch, improved, best, val, seconds):
        if improved:
            print("\nValidation loss improved from %s to %s - saving model state" % (round(best, 5), round(val, 5)))

    def _save(self, name):
        torch.save(self.state, os.path.join(self.save_dir, name))

    def start(self, test_data_path=None, result_path=None, test_resize_dim=(512, 512)):
        import time
        for epoch in range(self.num_epochs):
            t0 = time.time()
            self._train_epoch(epoch)
            with torch.no_grad():
                val_loss = self._validate(epoch)
                self.state = self._checkpoint(epoch, val_loss)
                self.scheduler.step(val_loss)
            improved = bool(val_loss < self.best_loss)
            self._report(epoch, improved, self.best_loss.item(), val_loss.item(), time.time() - t0)
            if improved:
                self.state["best_loss"] = self.best_loss = val_loss
                self._save(self.save_name)
            if self.save_iter:
                self._save(f"model_epoch_{epoch + self.epoch_start}.pt")
            if test_data_path is not None:
                raise NotImplementedError("per-epoch prediction of TIFF test folders is outside the hot path; call "
                                          "Predict on arrays instead")


class Trainer2D(_EpochLoop):
    """``bio_image_unet.unet.Trainer`` counterpart (``unet/train.py:16-198``)."""
    validates_last_batch = True

    def __init__(self, dataset, num_epochs, network=Unet, batch_size=4, lr=1e-3, in_channels=1, out_channels=1,
                 channel_weights=None, n_filter=64, dilation=1, val_split=0.2, save_dir="./", save_name="model.pt",
                 save_iter=False, load_weights=False, loss_function="BCEDice", loss_params=(0.5, 0.5),
                 device: Union[torch.device, str] = "auto", fp32_products: Optional[str] = None, augment=None):
        """``fp32_products`` (not in the reference): ``"exact"`` | ``"bf16x3"`` | ``"bf16x6"`` -- how the fp32 tensors of this trainer are
        multiplied (``bio_image_unet_amd.set_fp32_products``; process-wide).  ``"bf16x3"`` plays the role ``torch.backends.cudnn.allow_tf32``
        plays for the reference; ``None`` leaves the process's mode alone (default: bf16x6, fp32-grade split products).
        ``augment`` (not in the reference): ``True`` or an ``augment.Augmenter`` -- the training batches of a ``feed.TileStore`` are augmented on
        the device, fresh every epoch (recipe ``"unet"``); validation batches never are."""
        augmenter = _resolve_augment(augment, dataset, _pick_device(device), "unet")
        _set_fp32_products(fp32_products)
        self.device = _pick_device(device)
        self.network = network
        self.model = network(n_filter=n_filter, in_channels=in_channels, out_channels=out_channels, dilation=dilation).to(self.device)
        self.model.apply(init_weights)
        self.loss_function, self.loss_params, self.dim = loss_function, loss_params, dataset.dim_out
        self.n_filter, self.in_channels, self.out_channels = n_filter, in_channels, out_channels
        self.channel_weights = torch.ones(out_channels) if channel_weights is None else torch.tensor(channel_weights)
        self.criterion = _make_criterion(loss_function, loss_params)
        self._setup(dataset, num_epochs, batch_size, lr, val_split, save_dir, save_name, save_iter, augmenter,
                    os.path.join(save_dir, save_name) if load_weights else None)
        self.params = {"optimizer": self.optimizer.state_dict(), "lr": lr, "loss_function": loss_function,
                       "loss_params": loss_params, "n_filter": n_filter, "dilation": dilation, "batch_size": batch_size,
                       "augmentation": getattr(dataset, "aug_factor", None), "in_channels": in_channels,
                       "out_channels": out_channels,
                       **self._data_attr("clip_threshold", "noise_lims", "brightness_contrast", "shiftscalerotate"), **self._augment_entry()}

    def _forward_loss(self, batch, validating):
        d = self.dim
        x = batch["image"].view(self.batch_size, self.in_channels, d[0], d[1]).to(self.device)
        # the training branch reshapes the mask with dim[0] twice (square tiles assumed), the validation one does not
        y = _target(batch["mask"].view(self.batch_size, self.out_channels, d[0], d[1] if validating else d[0]).to(self.device))
        _, logits = self.model(x)
        cw = self.channel_weights
        # NOTE the reference indexes the BATCH axis with the channel index
        return sum(self.criterion(logits[ch], y[ch]) * cw[j] for j, ch in enumerate(range(self.out_channels))) / sum(cw)

    def _checkpoint(self, epoch, val_loss):
        return {"epoch": epoch, "best_loss": self.best_loss, "state_dict": self.model.state_dict(), **self.params}


class Trainer3D(_EpochLoop):
    """``bio_image_unet.unet3d.Trainer`` counterpart (``unet3d/train.py:18-217``)."""

    def __init__(self, dataset, num_epochs, network=UNet3D, use_interpolation=False, batch_size=4, lr=1e-3,
                 in_channels=1, out_channels=1, channel_weights=None, n_filter=64, dilation=1, val_split=0.2,
                 save_dir="./", save_name="model.pt", save_iter=False, load_weights=False, loss_function="BCEDice",
                 loss_params=(0.5, 0.5), time_loss_weight=0.1, device: Union[torch.device, str] = "auto",
                 fp32_products: Optional[str] = None, augment=None):
        """``fp32_products`` (not in the reference): ``"exact"`` | ``"bf16x3"`` | ``"bf16x6"`` -- how the fp32 3-D kernels of this trainer
        multiply (``bio_image_unet_amd.set_fp32_products_3d``; process-wide, default ``"exact"``); ``None`` leaves the process mode alone.
        ``augment``: as for ``Trainer2D``, recipe ``"unet3d"`` (every z-plane of a volume gets the same in-plane transform)."""
        augmenter = _resolve_augment(augment, dataset, _pick_device(device), "unet3d")
        _set_fp32_products(fp32_products, three_d=True)
        self.device = _pick_device(device)
        self.network = network
        self.model = network(n_filter=n_filter, in_channels=in_channels, out_channels=out_channels,
                             use_interpolation=use_interpolation).to(self.device)
        self.model.apply(init_weights)          # a no-op on Conv3d layers, as in the reference
        self.loss_function, self.loss_params, self.time_loss_weight = loss_function, loss_params, time_loss_weight
        self.n_filter, self.in_channels, self.out_channels = n_filter, in_channels, out_channels
        self.use_interpolation, self.dim = use_interpolation, dataset.dim_out
        self.channel_weights = torch.ones(out_channels) if channel_weights is None else torch.tensor(channel_weights)
        self.criterion = _make_criterion(loss_function, loss_params)
        self.criterion_time = nn.SmoothL1Loss()
        self._setup(dataset, num_epochs, batch_size, lr, val_split, save_dir, save_name, save_iter, augmenter,
                    os.path.join(save_dir, save_name) if load_weights else None)
        self.params = {"optimizer": self.optimizer.state_dict(), "lr": lr, "loss_function": loss_function,
                       "loss_params": loss_params, "time_loss_weight": time_loss_weight, "n_filter": n_filter,
                       "use_interpolation": use_interpolation, "dilation": dilation, "batch_size": batch_size,
                       "augmentation": getattr(dataset, "aug_factor", None), "in_channels": in_channels,
                       "out_channels": out_channels,
                       **self._data_attr("clip_threshold", "noise_amp", "brightness_contrast", "shiftscalerotate"), **self._augment_entry()}

    def _forward_loss(self, batch, validating):
        d = self.dim
        x = batch["volume"].view(self.batch_size, self.in_channels, d[0], d[1], d[2]).to(self.device)
        y = _target(batch["mask"].view(self.batch_size, self.out_channels, d[0], d[1], d[2]).to(self.device))
        _, logits = self.model(x)
        w = 0.1 if validating else self.time_loss_weight         # validation hard-codes 0.1
        # criterion(y_logits, y_i) + SmoothL1(y_logits[1:], y_logits[:-1]) * w (unet3d/train.py:140-145), one fused pass each way
        return self.criterion(logits, y, time_weight=w)

    def _checkpoint(self, epoch, val_loss):
        return {"val_loss": val_loss, "epoch": epoch, "best_loss": self.best_loss, "state_dict": self.model.state_dict(), **self.params}


class TrainerSiam(_EpochLoop):
    """``bio_image_unet.siam_unet.Trainer`` counterpart (``siam_unet/train.py:16-172``); the model class is fixed."""

    def __init__(self, dataset, num_epochs, batch_size=4, lr=1e-3, n_filter=32, mode="max", val_split=0.2,
                 save_dir="./", save_name="model.pt", save_iter=False, loss_function="BCEDice", loss_params=(1, 1),
                 load_weights=None, device: Union[torch.device, str] = "auto", fp32_products: Optional[str] = None, augment=None):
        augmenter = _resolve_augment(augment, dataset, _pick_device(device), "siam")      # see Trainer2D
        _set_fp32_products(fp32_products)                                                 # see Trainer2D
        self.device = _pick_device(device)
        self.model = Siam_UNet(n_filter=n_filter, mode=mode).to(self.device)      # no init_weights here (reference :61)
        self.n_filter, self.mode, self.dim = n_filter, mode, dataset.dim_out
        self.loss_function, self.loss_params = loss_function, loss_params
        # the Siam package's own criteria: its BCEDice takes nn.BCELoss on sigmoid(logits) (siam_unet/losses.py:5-39,73-105)
        self.criterion = _make_criterion(loss_function, loss_params, extra={"BCEDice": BCEDiceLossSiam, "weightedBCELoss": weightedBCELoss})
        self._setup(dataset, num_epochs, batch_size, lr, val_split, save_dir, save_name, save_iter, augmenter, load_weights)

    def _forward_loss(self, batch, validating):
        d = self.dim
        shape = (self.batch_size, 1, d[0], d[1])
        x = batch["image"].view(shape).to(self.device)
        px = batch["prev_image"].view(shape).to(self.device)
        y = _target(batch["mask"].view(shape).to(self.device))
        _, logits = self.model(x, px)
        return self.criterion(logits, y)

    def _checkpoint(self, epoch, val_loss):
        """The only family whose ``optimizer`` entry is taken every epoch."""
        return {"epoch": epoch, "best_loss": self.best_loss, "state_dict": self.model.state_dict(),
                "optimizer": self.optimizer.state_dict(), "lr": self.lr, "loss": self.loss_function,
                "loss_params": self.loss_params, "n_filter": self.n_filter, "mode": self.mode,
                "augmentation": getattr(self.data, "aug_factor", None),
                **self._data_attr("clip_threshold", "noise_amp", "brightness_contrast", "shiftscalerotate"), **self._augment_entry()}

    def _report(self, epoch, improved, best, val, seconds):
        if improved:
            print(f"\nEpoch {epoch}: Validation loss improved from {round(best, 5)} to {round(val, 5)} - saving model state")
        else:
            print(f"\nEpoch {epoch}: Validation loss did not improve from {round(best, 5)}")


class _MultiHeadLoop(_EpochLoop):
    """What the two multi-output families share: per-head criteria, activations and weights out of ``output_heads``, ``clip_grad_norm_(1.0)``
    before the step, ``ReduceLROnPlateau(patience=5, factor=0.2)``, no "Starting ..." lines, and a checkpoint that counts epochs on from the
    one ``load_weights`` read."""
    patience, factor, grad_clip, announces, resumes_epoch = 5, 0.2, 1.0, False, True

    def _set_heads(self, output_heads):
        self.output_heads = output_heads
        self.loss_functions = {name: self._get_loss_function(cfg["loss"]) for name, cfg in output_heads.items()}
        self.activations = {name: cfg.get("activation", None) for name, cfg in output_heads.items()}
        self.loss_weights = {name: cfg.get("weight", 1.0) for name, cfg in output_heads.items()}

    @staticmethod
    def _apply_activation(x, activation):
        fn = {"sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu, "softmax": lambda t: torch.softmax(t, dim=1)}
        return fn[activation](x) if activation in fn else x

    def _checkpoint(self, epoch, val_loss):
        return {"epoch": epoch + self.epoch_start, "epoch_start": self.epoch_start, "best_loss": self.best_loss,
                "state_dict": self.model.state_dict(), **self.params}


class TrainerMo3d(_MultiHeadLoop):
    """``bio_image_unet.multi_output_unet3d.Trainer`` counterpart (``multi_output_unet3d/train.py:17-292``).

    Per-head loss ``output_heads[name]['loss']`` applied to the model's (already activated) output, summed with the heads'
    weights, the whole sum as one fused autograd node (``multi_output_unet3d.losses.MultiHeadLoss``); ``clip_grad_norm_(1.0)`` before
    the step; validation applies the head activation once more before the loss (``:224``); scheduler
    ``ReduceLROnPlateau(patience=5, factor=0.2)``; the model stays in train mode during validation."""

    def __init__(self, dataset, output_heads, num_epochs, network=MultiOutputUnet3D, use_interpolation=False, batch_size=4,
                 lr=1e-3, in_channels=1, n_filter=64, dilation=1, val_split=0.2, save_dir="./", save_name="model.pt",
                 save_iter=False, load_weights=False, loss_function="BCEDice", loss_params=(0.5, 0.5), time_loss_weight=0.1,
                 device: Union[torch.device, str] = "auto", fp32_products: Optional[str] = None, augment=None):
        """``augment`` (not in the reference, which augments offline): ``True`` or an ``augment.AugmenterVol`` -- the training batches of a
        ``feed.TileStore`` are augmented on the device, fresh every epoch (``augment.py``, recipe ``"mo3d"``); validation batches never.
        A ``feed.VolumeStore`` (``multi_output_unet3d.prepare``) is always augmented: every patch is a random crop of a whole volume
        rendered on the device (``feed.CropFeeder``), validation patches with one fixed epoch key; ``augment=False`` is refused."""
        _set_fp32_products(fp32_products, three_d=True)             # see Trainer3D
        self.device = _pick_device(device)
        augmenter = _resolve_augment(augment, dataset, self.device, "mo3d")
        self.network = network
        self.model = network(n_filter=n_filter, in_channels=in_channels, output_heads=output_heads,
                             use_interpolation=use_interpolation).to(self.device)
        self.model.apply(init_weights)          # a no-op on Conv3d layers, as in the reference
        self.loss_function, self.loss_params, self.time_loss_weight = loss_function, loss_params, time_loss_weight
        self.n_filter, self.in_channels, self.use_interpolation, self.dim = n_filter, in_channels, use_interpolation, dataset.dim_out
        self._set_heads(output_heads)
        from .multi_output_unet3d.losses import MultiHeadLoss
        self.head_loss = MultiHeadLoss(output_heads, loss_functions=self.loss_functions)
        if loss_function == "BCEDiceTemporalLoss":
            self.criterion = BCEDiceTemporalLoss(loss_params=loss_params)
        else:
            self.criterion = _make_criterion(loss_function, loss_params)       # built but unused by the loop, as upstream
        self.criterion_time = nn.SmoothL1Loss()
        self._setup(dataset, num_epochs, batch_size, lr, val_split, save_dir, save_name, save_iter, augmenter,
                    load_from=os.path.join(save_dir, save_name) if load_weights else None)
        self.params = {"optimizer": self.optimizer.state_dict(), "lr": lr, "loss_function": loss_function,
                       "loss_params": loss_params, "time_loss_weight": time_loss_weight, "n_filter": n_filter,
                       "use_interpolation": use_interpolation, "dilation": dilation, "batch_size": batch_size,
                       "augmentation": getattr(dataset, "aug_factor", None),
                       **self._data_attr("clip_threshold", "scale_limit", "rotate_limit", "gauss_noise_lims", "shot_noise_lims", "blur_limit",
                                         "random_rotate", "brightness_contrast"),
                       "in_channels": in_channels, "output_heads": output_heads, **self._augment_entry()}

    @staticmethod
    def _get_loss_function(loss_name):
        from .multi_output_unet3d.losses import get_loss_function
        return get_loss_function(loss_name)

    def _total_loss(self, batch, validating):
        x = batch["volume"].to(self.device, non_blocking=True)
        y = {key: _target(batch[key].to(self.device, non_blocking=True)) for key in self.output_heads}
        if x.dim() == 4:
            x = x.unsqueeze(1)
        # one fused node over the heads; validation activates the activated outputs once more, in the forward kernel's registers
        return self.head_loss(self.model(x), y, pre_activations=self.activations if validating else None)

    _forward_loss = _total_loss

    def _report(self, epoch, improved, best, val, seconds):
        if improved:
            print(f"\nValidation loss improved from {best:.5f} to {val:.5f} - saving model state")
        else:
            print(f"\nValidation loss did not improve from {best:.5f}")


class _OwnKeywords(type):
    """``TrainerMo2d.__init__`` keeps the reference's parameter list exactly, names, order and defaults (the drop-in contract that
    ``tests/test_mo2d_losses_host.py`` pins).  A keyword this package adds is therefore taken where the class is called, keyword-only and
    behind everything the reference knows, and is in place on the instance when ``__init__`` runs."""

    def __call__(cls, *args, augment=None, **kwargs):
        self = cls.__new__(cls)
        self._augment = augment
        self.__init__(*args, **kwargs)
        return self


class TrainerMo2d(_MultiHeadLoop, metaclass=_OwnKeywords):
    """``bio_image_unet.multi_output_unet.Trainer`` counterpart (``multi_output_unet/train.py:18-131,144-232,369-407``).

    Per head the criterion ``output_heads[name]['loss']`` (one of the ten of ``multi_output_unet.losses``) on the model's already
    activated output, times the head's ``'weight'``; under deep supervision summed over the levels ``name_1 ... name_L`` with weights
    ``[0.5, 0.75, 1.0]`` (``levels=3``) or ``[0.5, 0.75, 0.875, 1.0]`` (``levels=4``).  The whole sum is one fused autograd node
    (``losses.MultiHeadLoss``).  ``clip_grad_norm_(1.0)`` before the step, ``ReduceLROnPlateau(patience=5, factor=0.2)``, and the
    reference's checkpoint / ``params`` keys.  The ``[0, 1]`` assertion of ``BCEDiceLoss`` is raised where the loop reads the loss
    (``total_loss.item()``, once per step), not in the middle of the step.

    Quirks of the reference that change numbers, kept:

    * validation applies the head activation (``softmax`` included) AGAIN to the already activated outputs (``:218,222``);
    * validation under deep supervision always weights levels 1-3 with ``[0.5, 0.75, 1.0]``, also for the four-level network (``:215``);
    * the model is never put in eval mode during validation: BatchNorm keeps using and updating batch statistics;
    * ``levels`` outside {3, 4} raises ``ValueError`` at the first training step under deep supervision (``:170-172``).

    ``SummaryWriter`` scalars (``Loss/train``, ``Loss/val``) are written only when ``tensorboard`` imports.  The PNG / TensorBoard image
    logging of the reference (``plot_images``, ``log_validation_images``) is outside the hot path and is not ported."""
    reads_loss = True

    def __init__(self, dataset, num_epochs: int, network=MultiOutputNestedUNet, levels: int = 4, batch_size: int = 4, lr: float = 1e-4,
                 in_channels: int = 1, output_heads: Optional[dict] = None, n_filter: int = 64, deep_supervision: bool = False,
                 dilation=False, val_split: float = 0.2, save_dir: str = "./", save_name: str = "model.pt", save_iter: bool = False,
                 load_weights: bool = False, device: Union[torch.device, str] = "auto"):
        """``TrainerMo2d(..., augment=None)`` (keyword only, not in the reference, which augments offline; taken by ``_OwnKeywords``): ``True`` or
        an ``augment.AugmenterF32`` -- the training batches of a ``feed.TileStore`` are augmented on the device, fresh every epoch
        (``augment.py``, recipe ``"mo2d"``); validation batches never.  A ``feed.ImageStore`` (``multi_output_unet.prepare``) is always
        augmented: every patch is a random crop of a whole item rendered on the device (``feed.CropFeeder``), validation patches with one
        fixed epoch key."""
        import random
        from .multi_output_unet.losses import MultiHeadLoss
        self.device = _pick_device(device)
        augmenter = _resolve_augment(getattr(self, "_augment", None), dataset, self.device, "mo2d")
        self.network = network
        self.model = network(n_filter=n_filter, in_channels=in_channels, output_heads=output_heads, dilation=dilation,
                             deep_supervision=deep_supervision).to(self.device)
        self.model.apply(init_weights)
        self.levels, self.n_filter, self.dilation, self.in_channels = levels, n_filter, dilation, in_channels
        self.dim = getattr(dataset, "dim_out", None)
        self._set_heads(output_heads)
        self.criterion = MultiHeadLoss(output_heads, deep_supervision=bool(getattr(self.model, "deep_supervision", False)), levels=levels,
                                       loss_functions=self.loss_functions)
        self._setup(dataset, num_epochs, batch_size, lr, val_split, save_dir, save_name, save_iter, augmenter,
                    os.path.join(save_dir, save_name) if load_weights else None)
        self.params = {"optimizer": self.optimizer.state_dict(), "lr": lr, "n_filter": n_filter, "deep_supervision": deep_supervision,
                       "dilation": dilation, "batch_size": batch_size, "augmentation": getattr(dataset, "aug_factor", None),
                       **self._data_attr("clip_threshold", "gauss_noise_lims", "shot_noise_lims", "brightness_contrast", "random_rotate"),
                       "in_channels": in_channels, "output_heads": output_heads, **self._augment_entry()}
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.writer = SummaryWriter(log_dir=os.path.join(save_dir, "logs"))
        except Exception:                   # tensorboard is optional here
            self.writer = None
        self.random_seed = 42
        random.seed(self.random_seed)

    @staticmethod
    def _get_loss_function(loss_name):
        from .multi_output_unet.losses import get_loss_function
        return get_loss_function(loss_name)

    def _batch(self, batch):
        x = batch["image"].to(self.device, non_blocking=True)
        y = {key: _target(batch[key].to(self.device, non_blocking=True)) for key in self.output_heads}
        return (x.unsqueeze(1) if x.dim() == 3 else x), y

    def _total_loss(self, batch, validating):
        x, y = self._batch(batch)
        pred = self.model(x)
        if not validating:
            return self.criterion(pred, y)
        # the activation once more on the activated outputs, and three level weights whatever the network's depth
        ds = self.criterion.deep_supervision
        keys = [f"{name}_{l}" for name in self.output_heads for l in (1, 2, 3)] if ds else list(self.output_heads)
        act = {k: self._apply_activation(pred[k], self.activations.get(k.rsplit("_", 1)[0] if ds else k)) for k in keys}
        return self.criterion(act, y, weights=[0.5, 0.75, 1.0] if ds else None)

    _forward_loss = _total_loss

    def _report(self, epoch, improved, best, val, seconds):
        print(f"\nEpoch {epoch} completed in {round(seconds, 2)} seconds.")
        super()._report(epoch, improved, best, val, seconds)


# ----------------------------------------------------------------------------------------------------------------------
# Prediction: open -> normalise -> tile -> forward (eval) -> stitch in HBM -> write
# ----------------------------------------------------------------------------------------------------------------------
def _percentile_rescale(imgs, mode, clip, top=None, invert=False):
    """Percentile clip, shift to 0 and divide by the maximum -- then times ``top`` and, with ``invert``, ``top - a``: per image ('single'), by
    the first image's histogram ('first') or the whole stack's ('all').  Lower bound ``nanpercentile``, upper ``percentile`` as upstream."""
    def scale(a, ref):
        a = np.clip(a, a_min=np.nanpercentile(ref, clip[0]), a_max=np.percentile(ref, clip[1]))
        a = a - np.min(a)
        a = a / np.max(a)
        if top is not None:
            a = a * top
        return top - a if invert else a

    if mode == "single":
        for i, img in enumerate(imgs):
            imgs[i] = scale(img, img)
        return imgs
    if mode == "first":
        return scale(imgs, imgs[0])
    if mode == "all":
        return scale(imgs, imgs)
    raise ValueError(f"normalization_mode {mode} not valid!")


def normalise_stack(imgs: np.ndarray, mode: str, clip, invert: bool) -> np.ndarray:
    """Percentile clip and rescale to [0, 255], ``a / max * 255`` in that order (``unet/predict.py:122-150``)."""
    return _percentile_rescale(imgs, mode, clip, 255, invert)


def tile_starts(extent: int, tile: int, n: int) -> np.ndarray:
    """Evenly spaced tile origins, truncated to uint16 like the reference (``unet/predict.py:170-171``)."""
    return np.linspace(0, extent - tile, n).astype("uint16")


class _Stitcher:
    """Stitched result volume kept in HBM: patches are added where the network wrote them (``biu_stitch_add``) and the volume is
    normalised once (``biu_stitch_finish``) -- no per-patch device-to-host copy, no host numpy accumulation.  ``layers`` > 1 keeps
    separate overwrite-mode layers (the three-layer buffer of ``unet3d/predict.py:173-195``)."""

    def __init__(self, device, channels, shape3, layers=1):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"Predict stitches on the GPU (biu_stitch_add / biu_stitch_finish); got device '{device}'. There is no CPU path.")
        self.device, self.channels, self.shape, self.layers = device, channels, tuple(shape3), layers
        d, h, w = self.shape
        self.acc = torch.zeros((layers, channels, d, h, w), dtype=torch.float32, device=device)
        self.wsum = torch.zeros((layers, d, h, w), dtype=torch.float32, device=device)

    def reset(self):
        self.acc.zero_()
        self.wsum.zero_()

    def add(self, patch: torch.Tensor, origin, weight: torch.Tensor = None, layer: int = 0, overwrite: bool = False):
        """patch: device tensor [channels, pd, ph, pw] (uint8 or float32); origin (z0, y0, x0); weight [pd, ph, pw] float32 or None."""
        patch = patch.contiguous()
        assert patch.dim() == 4 and patch.shape[0] == self.channels and patch.dtype in (torch.uint8, torch.float32)
        c, pd, ph, pw = patch.shape
        d, h, w = self.shape
        st = stream()
        check(lib.biu_stitch_add(ptr(patch), int(patch.dtype == torch.uint8), ptr(weight), c, pd, ph, pw,
                                 ptr(self.acc[layer]), ptr(self.wsum[layer]), d, h, w,
                                 int(origin[0]), int(origin[1]), int(origin[2]), int(overwrite), st), "stitch_add")

    def finish(self, as_uint8: bool) -> torch.Tensor:
        d, h, w = self.shape
        out = torch.empty((self.channels, d, h, w), dtype=torch.uint8 if as_uint8 else torch.float32, device=self.device)
        check(lib.biu_stitch_finish(ptr(self.acc), ptr(self.wsum), self.layers, self.channels, d * h * w, ptr(out), int(as_uint8), stream()),
              "stitch_finish")
        return out


class _HeadStitch:
    """The stitchers of the two multi-output Predicts, ``self[head]`` one ``_Stitcher`` per image or volume, and the weight arrays on the
    device, one per combination of neighbour flags.  ``make_weight(index, flags)`` is the family's: the weight array of the tile at grid
    position ``index`` of ``grid``, ``flags`` saying per axis whether it has a neighbour before and after."""

    def __init__(self, device, heads, count, shape3, grid, make_weight):
        self.device, self.grid, self.make_weight, self.weights = device, tuple(grid), make_weight, {}
        self.stitchers = {k: [_Stitcher(device, cfg["channels"], shape3) for _ in range(count)] for k, cfg in heads.items()}

    def __getitem__(self, head):
        return self.stitchers[head]

    def add(self, patches, image, origin, index):
        """patches: {head: [channels, pd, ph, pw] float32}, one patch's predictions; into image ``image`` at ``origin``."""
        flags = tuple(f for i, n in zip(index, self.grid) for f in (i > 0, i < n - 1))
        if flags not in self.weights:
            self.weights[flags] = torch.from_numpy(self.make_weight(index, flags)).to(self.device).contiguous()
        for k, patch in patches.items():
            self.stitchers[k][image].add(patch, origin, weight=self.weights[flags])


def _quantize_u8(prob: torch.Tensor) -> torch.Tensor:
    """``(res * 255).astype('uint8')`` (unet/predict.py:200) on the device."""
    prob = prob.contiguous().float()
    out = torch.empty(prob.shape, dtype=torch.uint8, device=prob.device)
    check(lib.biu_quantize_u8(ptr(prob), 255.0, ptr(out), prob.numel(), stream()), "quantize_u8")
    return out


def _check_preprocess(preprocess):
    """``preprocess`` of the Predict classes: ``'host'`` normalises and tiles in numpy as the reference does; ``'device'`` uploads the raw
    stack once and does both in HBM (``preprocess.DeviceFrontEnd``)."""
    if preprocess not in ("host", "device"):
        raise ValueError(f"preprocess '{preprocess}' not valid: 'host' or 'device'")


def _patch_batch(patches, i, j, device):
    """Patches ``i:j`` on the device: a slice of the host array sent up, or cut and normalised there by the device front end."""
    if isinstance(patches, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(patches[i:j])).to(device, non_blocking=True)
    return patches.batch(i, j)


def _cut(stack, origins, tile, dtype=None, mode="reflect"):
    """The host cut: ``stack`` [images, D, H, W], padded at the far ends where a tile is larger (``mode``), and the ``tile`` at every origin
    (image, z, y, x) -- the numpy counterpart of ``DeviceFrontEnd.tiles``.  Assignment casts to ``dtype`` (float -> uint8 truncates)."""
    pad = [(0, 0)] + [(0, max(0, t - n)) for t, n in zip(tile, stack.shape[1:])]
    if any(p for _, p in pad):
        stack = np.pad(stack, pad, mode)
    patches = np.empty((len(origins),) + tuple(tile), dtype=dtype or stack.dtype)
    for n, (i, z, y, x) in enumerate(origins):
        patches[n] = stack[i, z:z + tile[0], y:y + tile[1], x:x + tile[2]]
    return patches


def _unit_range(img):
    """``normalize_result``: shift to 0, divide by the 99.8th percentile, clip to [0, 1]."""
    img = img - np.nanmin(img)
    img = img / np.nanpercentile(img, 99.8)
    return np.clip(img, 0, 1)


def _write(result_name, arr, tif_dtype=None):
    if result_name is None:
        return
    try:
        import tifffile
        tifffile.imwrite(result_name, arr if tif_dtype is None else arr.astype(tif_dtype))
    except ImportError:
        np.save(result_name if result_name.endswith(".npy") else result_name + ".npy", arr)


def _write_heads(result_path, result):
    """``result_path`` given: one file per head (``result_path + name + '.tif'`` in an existing folder, else ``result_path_name.tif``) and
    ``None``; otherwise the dictionary itself."""
    if result_path is None:
        return result
    for k, arr in result.items():
        _write((result_path + k + ".tif") if os.path.exists(result_path) else (result_path + "_" + k + ".tif"), arr)
    return None


class _PredictBase:
    """The one pipeline under the five Predicts.  A constructor runs it in this order: ``_open`` the input; geometry and patches -- the host
    path normalises and ``_split``s in numpy, the device path hands ``_origins()`` to a ``DeviceFrontEnd``; ``_load_model``; the loop over
    ``_batches`` that runs ``_forward`` and stitches every predicted patch at ``_place(k)``; crop and write.  A family provides ``_origins()``
    (its tile grid, kept as ``self.origins``: the only statement of tile order, for cutting and for stitching), ``_split``, its
    normalisation, ``_build(model_params, network)`` and what it does with one predicted patch."""
    rank = 3            # of the stack; input one rank lower is a single image / volume and gets the leading axis

    def _open(self, data, device, preprocess):
        """The input as an array of ``rank`` axes (a path is read through ``tifffile``); sets ``self.device``."""
        _check_preprocess(preprocess)
        self.device = _pick_device(device)
        if isinstance(data, str):
            import tifffile                      # only needed for file input; not a dependency of the hot path
            data = tifffile.imread(data)
        data = np.asarray(data)
        return data[None] if data.ndim == self.rank - 1 else data

    def _load_model(self, model_params, network=None):
        """The checkpoint (a path or the dictionary itself) into ``model_params`` and the family's network, loaded and in eval mode."""
        mp = self.model_params = torch.load(model_params, map_location=self.device) if isinstance(model_params, str) else model_params
        self.model = self._build(mp, network).to(self.device)
        self.model.load_state_dict(mp["state_dict"])
        self.model.eval()
        return mp

    def _batches(self, patches, batch_size):
        """(index of its first patch, the batch on the device) over ``patches`` -- a host array that goes up slice by slice, or the device
        front end's tiles, cut in HBM."""
        for i in range(0, len(patches), batch_size):
            yield i, _patch_batch(patches, i, i + batch_size, self.device)

    @torch.no_grad()
    def _forward(self, *batch):
        """The network on one batch, outside autograd.  (``no_grad`` sits here and not around the ``yield`` of ``_batches``: held open across a
        ``yield`` it would stay in force after an exception in the loop body, until the suspended generator is collected.)"""
        return self.model(*batch)

    def _grid_2d(self, n_img):
        """Tile grid of the two 2-D uint8 families (``unet/predict.py:153-181``) over ``n_img`` images of ``imgs_shape[1:]``: ``add_tile`` extra
        tiles per axis, ``linspace`` origins; the order is image, row, column."""
        (h, w), (th, tw) = self.imgs_shape[1:], self.resize_dim
        self.N_x = int(np.ceil(h / th)) + self.add_tile
        self.N_y = int(np.ceil(w / tw)) + self.add_tile
        self.N_per_img = self.N_x * self.N_y
        self.X_start, self.Y_start = tile_starts(h, th, self.N_x), tile_starts(w, tw, self.N_y)
        self.origins = [(i, 0, int(xs), int(ys)) for i in range(n_img) for xs in self.X_start for ys in self.Y_start]
        return self.origins

    def _place(self, k):
        """Where patch ``k`` is stitched: (image or volume, origin in it) -- the two parts of the origin it was cut at."""
        o = self.origins[k]
        return o[0], o[1:]


class Predict2D(_PredictBase):
    """``bio_image_unet.unet.Predict`` counterpart (``unet/predict.py:14-229``) for in-memory arrays.

    Same preprocessing, tiling, uint8 re-quantisation ``(p*255).astype('uint8')`` and nan-mean stitching; patches are
    pushed through the network in batches (eval-mode BatchNorm makes that identical to the reference's batch of 1) so the
    device is not synchronised once per patch.  The result is kept in ``self.imgs_result`` and written to
    ``result_name`` (TIFF via tifffile when importable -- float16 like ``save_as_tif`` -- otherwise ``.npy``).

    ``preprocess='device'`` (default ``'host'``) normalises and tiles in HBM (``preprocess.DeviceFrontEnd``): fp64 from the values as
    uploaded, bit-equal to the host path for integer and float64 input (float64 goes up as float32 and raises ``ValueError`` unless every
    value is exactly representable); float32 input, which the host path normalises in numpy float32, gets the same formula in fp64
    rounded once; NaN raises ``ValueError`` (use ``preprocess='host'``); a constant image is 0 / 0 on both paths."""

    def __init__(self, imgs, result_name, model_params, network="Unet", resize_dim=(512, 512), invert=False,
                 normalization_mode="single", clip_threshold=(0., 99.8), add_tile=0, normalize_result=False,
                 show_progress=True, device: Union[torch.device, str] = "auto", progress_notifier=None, batch_size=8,
                 preprocess="host"):
        raw = self._open(imgs, device, preprocess)
        self.resize_dim, self.add_tile, self.imgs_shape = tuple(resize_dim), add_tile, raw.shape
        if preprocess == "device":
            # the raw stack goes up in its own dtype; percentiles, rescale, reflect padding and tiling happen in HBM (preprocess.py).  fp64
            # from the values as uploaded: bit-equal to the host path for integer and float64 input; float32 input, which the host path
            # normalises in numpy float32, comes out as the same formula evaluated in fp64
            fe = DeviceFrontEnd(raw, self.device)
            fe.normalise(normalization_mode, clip_threshold)
            patches = fe.tiles(self._origins(), (1,) + self.resize_dim, out="uint8", invert=invert)
        else:
            imgs = np.array(raw, dtype=np.float64 if raw.dtype.kind != "f" else raw.dtype)
            patches = self._split(normalise_stack(imgs, normalization_mode, clip_threshold, invert))
        self._load_model(model_params, network)
        self.imgs_result = self._predict_and_stitch(patches, batch_size)
        # float16 like ``save_as_tif`` in the TIFF only; the ``.npy`` fallback keeps the array as it is
        _write(result_name, _unit_range(self.imgs_result) if normalize_result else self.imgs_result, tif_dtype="float16" if normalize_result else None)

    def _build(self, mp, network):
        if network is None:
            network = mp.get("network")
            if network is None:
                raise ValueError("network is not defined")
        if network == "Unet_v0" and "in_channels" not in mp:        # legacy checkpoints carry no channel counts (unet/predict.py:93-97)
            mp["in_channels"] = mp["out_channels"] = 1
        if isinstance(network, str):
            table = {"Unet": Unet, "AttentionUnet": AttentionUnet, "Unet_v0": Unet_v0}
            if network not in table:
                raise ValueError(f"network '{network}' is not one of 'Unet', 'AttentionUnet', 'Unet_v0' (or pass a class)")
            network = table[network]
        # (the reference ignores the checkpoint's 'dilation' here, unet/predict.py:98-99 -- so does this)
        return network(n_filter=mp["n_filter"], in_channels=mp["in_channels"], out_channels=mp["out_channels"])

    def _origins(self):
        """Tile grid of ``unet/predict.py:153-181``: sets ``N_x``, ``N_y``, ``X_start``, ``Y_start`` and returns the patch order as
        (image, 0, row, column) in the (reflect-padded) stack -- shared by the host ``_split``, the device front end and the stitch."""
        return self._grid_2d(self.imgs_shape[0])

    def _split(self, imgs):
        return _cut(imgs[:, None], self._origins(), (1,) + self.resize_dim, "uint8")          # float -> uint8 truncation, as upstream

    def _predict_and_stitch(self, patches, batch_size):
        """uint8 patches up (divided by 255 in the input-layout kernel), eval-mode forward in batches that run across image borders,
        ``(p * 255)`` truncated to uint8 and added into the stitched image on the device; nan-mean of the overlapping uint8 tiles followed
        by the uint8 cast == floor(sum / count) (``unet/predict.py:184-229``).  One download per stack."""
        n_img, h, w = self.imgs_shape
        th, tw = self.resize_dim
        st = _Stitcher(self.device, self.model_params["out_channels"], (1, max(th, h), max(tw, w)))
        done = []
        for i, x in self._batches(patches, batch_size):             # uint8 across PCIe (host path) or cut in HBM (device path)
            q = _quantize_u8(self._forward(x)[0])
            for j in range(q.shape[0]):
                img, origin = self._place(i + j)
                if img != len(done):                                # the first patch of the next image: the one before is complete
                    done.append(st.finish(True))
                    st.reset()
                st.add(q[j].unsqueeze(1), origin)
        done.append(st.finish(True))
        res = torch.stack(done).cpu().numpy()[:, :, 0]              # (n_img, oc, H, W)
        return np.squeeze(res[:, :, :h, :w])


class Predict3D(_PredictBase):
    """``bio_image_unet.unet3d.Predict`` counterpart (``unet3d/predict.py:12-195``) for in-memory volumes.

    Whole-volume percentile clip to [0, 255]; patches of ``resize_dim`` (z, x, y) at ``linspace`` origins (reflect padding
    when the volume is smaller); one eval-mode forward per patch; uint8 re-quantisation; stitching through the
    reference's three-layer float16 buffer (patch ``n`` goes to layer ``n % 3``, later patches overwrite earlier ones of
    the same layer, then ``nanmean`` over the layers).  ``preprocess='device'``: as for ``Predict2D``, same departures (the host path
    computes in float64 for integer volumes and in float32 for float32 ones)."""

    def __init__(self, vol, result_name, model_params, network=UNet3D, resize_dim=(64, 128, 128), invert=False,
                 normalization_mode="single", clip_threshold=(0., 99.8), add_patch=0, normalize_result=False,
                 progress_bar=True, device: Union[torch.device, str] = "auto", progress_notifier=None, preprocess="host"):
        vol = self._open(vol, device, preprocess)
        self.resize_dim, self.add_patch, self.vol_shape = tuple(resize_dim), add_patch, vol.shape
        rd, vs = self.resize_dim, self.vol_shape
        if preprocess == "device":                                      # (departures as for Predict2D)
            fe = DeviceFrontEnd(vol, self.device, depth=vol.shape[0])
            fe.normalise("all", clip_threshold)
            patches = fe.tiles(self._origins(), rd, out="uint8", invert=invert)
        else:                                                           # the whole volume's histogram, whatever normalization_mode says
            patches = self._split(normalise_stack(vol, "all", clip_threshold, invert))
        self._load_model(model_params, network)
        # one eval-mode forward per patch as upstream (unet3d/predict.py:155-171); quantisation and the three-layer stitch buffer
        # (patch n overwrites layer n % 3, then the nan-mean over the layers, :173-195) stay on the device
        st = _Stitcher(self.device, 1, tuple(max(vs[a], rd[a]) for a in range(3)), layers=3)
        for i, x in self._batches(patches, 1):
            prob, _ = self._forward(x.view((1, 1) + rd))                   # uint8; /255 in the layout kernel
            st.add(_quantize_u8(prob).view((1,) + rd), self._place(i)[1], layer=i % 3, overwrite=True)
        out = st.finish(True)[0].cpu().numpy()
        self.vol_result = np.squeeze(out[:vs[0], :vs[1], :vs[2]])
        _write(result_name, _unit_range(self.vol_result).astype("float16") if normalize_result else self.vol_result)

    def _build(self, mp, network):
        return network(n_filter=mp["n_filter"], in_channels=mp["in_channels"], out_channels=mp["out_channels"],
                       use_interpolation=mp.get("use_interpolation", False))

    def _origins(self):
        """Patch grid of ``unet3d/predict.py:118-150``: sets the counts and ``Z_start`` / ``X_start`` / ``Y_start`` and returns the patch order
        as (0, z, x, y) in the (reflect-padded) volume -- shared by the host ``_split``, the device front end and the stitch."""
        vs, rd, ap = self.vol_shape, self.resize_dim, self.add_patch
        self.N_z = int(np.ceil(vs[0] / rd[0])) + ap
        self.N_x = int(np.ceil(vs[1] / rd[1])) + ap
        self.N_y = int(np.ceil(vs[2] / rd[2])) + ap
        self.N_x += ap if self.N_z > 1 else 0          # (sic) the reference bumps N_x twice (unet3d/predict.py:124-126)
        self.N_x += ap if self.N_x > 1 else 0
        self.N_y += ap if self.N_y > 1 else 0
        self.N = self.N_x * self.N_y * self.N_z
        self.Z_start = tile_starts(vs[0], rd[0], self.N_z)
        self.X_start = tile_starts(vs[1], rd[1], self.N_x)
        self.Y_start = tile_starts(vs[2], rd[2], self.N_y)
        self.origins = [(0, int(z), int(x), int(y)) for z in self.Z_start for x in self.X_start for y in self.Y_start]
        return self.origins

    def _split(self, vol):
        return _cut(vol[None], self._origins(), self.resize_dim, "uint8")


class PredictSiam(_PredictBase):
    """``bio_image_unet.siam_unet.Predict`` counterpart (``siam_unet/predict.py:16-250``) for an in-memory movie (T, H, W).

    Frame i is predicted together with its predecessor (frame 0 with frame 1, or with itself in a one-frame movie); every
    pair is normalised on its own (``normalization_mode`` over the two-frame stack), zero-padded (``'constant'``) up to
    ``resize_dim``, tiled, predicted and stitched by the nan-mean of overlapping uint8 tiles.

    ``preprocess='device'`` uploads the movie once and selects every pair's statistics in one batch before the frame loop (a pair is one
    unit in ``'first'`` / ``'all'``, every image its own in ``'single'``); the host path computes in float64 whatever the input, so the
    device path equals it bit for bit for every input it accepts (integers, float32, float64 that float32 holds exactly; NaN raises
    ``ValueError``)."""

    def __init__(self, movie, result_name, model_params, resize_dim=None, invert=False, normalization_mode="single",
                 clip_threshold=(0., 99.8), add_tile=0, normalize_result=False, show_progress=True,
                 device: Union[torch.device, str] = "auto", progress_notifier=None, batch_size=8, preprocess="host"):
        movie = self._open(movie, device, preprocess)
        self.tif_len, h, w = self.imgs_shape = list(movie.shape)
        self.resize_dim, self.add_tile = tuple(resize_dim) if resize_dim is not None else (h, w), add_tile
        th, tw = self.resize_dim
        if preprocess == "device":
            # the movie goes up once; every pair's order statistics are selected in one batch before the frame loop (float64 arithmetic on
            # the values as uploaded, as the host path's ``np.array([prev, cur], dtype=np.float64)``), zero padding written by the kernel
            fe = DeviceFrontEnd(movie, self.device)
            fe.normalise_pairs(normalization_mode, clip_threshold)
            pairs = fe.pair_tiles(self._origins(), self.resize_dim, invert=invert)
        self._load_model(model_params)
        stitch = _Stitcher(self.device, 1, (1, max(th, h), max(tw, w)))
        frames = []
        for i in range(self.tif_len):
            if preprocess == "device":
                patches = pairs.frame(i, self.N)
            else:                               # the host path normalises and cuts a pair when its turn comes, never the whole movie
                patches = self._pair_patches(movie, i, normalization_mode, clip_threshold, invert)
            stitch.reset()
            for b, both in self._batches(patches, batch_size):                  # uint8 (cur, prev)
                q = _quantize_u8(self._forward(both[:, 0:1].contiguous(), both[:, 1:2].contiguous())[0])
                for j in range(q.shape[0]):
                    stitch.add(q[j].unsqueeze(1), self._place(b + j)[1])
            frames.append(stitch.finish(True)[0, 0, :h, :w])                 # nan-mean of uint8 tiles, truncated like astype
        self.imgs_result = torch.stack(frames).cpu().numpy()
        _write(result_name, self.imgs_result)

    def _build(self, mp, network):
        return Siam_UNet(n_filter=mp["n_filter"], mode=mp["mode"])               # the model class is fixed

    def _origins(self):
        """Tile grid of one frame pair (``siam_unet/predict.py``, as ``Predict2D``'s): sets ``N_x``, ``N_y``, ``N``, ``X_start``, ``Y_start`` and
        returns the tile order as (0, 0, row, column) -- shared by the host ``_split``, the device front end and the stitch."""
        origins = self._grid_2d(1)
        self.N = self.N_per_img
        return origins

    def _pair_patches(self, movie, i, normalization_mode, clip_threshold, invert):
        """The host path's patches of frame ``i``: the frame and its predecessor (frame 0 goes with frame 1, or with itself in a one-frame
        movie, ``siam_unet/predict.py:108-117``), normalised as a two-frame stack, truncated to uint8 and cut."""
        prev = movie[(0 if self.tif_len == 1 else 1) if i == 0 else i - 1]
        pair = normalise_stack(np.array([prev, movie[i]], dtype=np.float64), normalization_mode, clip_threshold, invert).astype("uint8")
        return self._split(pair)

    def _split(self, pair):
        """(previous, current) -> patches [N, 2, th, tw] with the current frame in channel 0."""
        return _cut(pair[::-1][None], self._origins(), (2,) + self.resize_dim, "uint8", mode="constant")


class PredictMo3d(_PredictBase):
    """``bio_image_unet.multi_output_unet3d.Predict`` counterpart (``multi_output_unet3d/predict.py:13-307``).

    Float normalisation to [0, 1] (no uint8 step), patches of ``min(volume, max_patch_size)`` on a stride of
    ``patch * (1 - overlap_factor)`` plus a last patch flush with the border, batches of ``batch_size``, outputs kept as
    float32 per head, weighted blending with the reference's linear ramps over ``blend_margin`` voxels at interior patch
    faces (built exactly as upstream assigns them: plane by plane, later axes overwriting earlier ones).

    ``preprocess='device'``: normalisation and patch cutting in HBM.  The host path computes in numpy float32 (its percentiles included); the
    device path evaluates the same formula in fp64 on the uploaded values (uint8 / uint16 / int16 as they are, anything else after the
    host path's own cast to float32) and rounds to float32 once, so the two can differ in the last bit of a patch value.  NaN raises
    ``ValueError`` (use ``preprocess='host'``)."""
    rank = 4

    def __init__(self, imgs, model_params, result_path=None, network=MultiOutputUnet3D, max_patch_size=(64, 256, 256),
                 overlap_factor=0.1, batch_size=1, normalization_mode="single", clip_threshold=(0., 99.98), add_tile=0,
                 compress_tif=False, show_progress=True, device: Union[torch.device, str] = "auto", progress_notifier=None,
                 preprocess="host"):
        raw = self._open(imgs, device, preprocess)
        self.max_patch_size, self.overlap_factor, self.batch_size = max_patch_size, overlap_factor, batch_size
        if preprocess == "host" or not DeviceFrontEnd.native(raw.dtype):
            raw = np.array(raw, dtype="float32")                         # the host path's cast; the device path keeps small integers as they are
        if raw.ndim != 4:
            raise ValueError(f"Unsupported input shape: {raw.shape}")
        self.imgs_shape = raw.shape
        if preprocess == "device":
            # the host path normalises in numpy float32 (percentiles included); here the same formulas run in fp64 on the uploaded values
            # and are rounded to float32 once
            if normalization_mode not in ("single", "first", "all"):
                raise ValueError(f"Invalid normalization mode: {normalization_mode}")
            fe = DeviceFrontEnd(raw, self.device, depth=raw.shape[1])
            fe.normalise(normalization_mode, clip_threshold, family="minmax_eps" if normalization_mode == "single" else "lohi_eps")
            origins = self._origins(raw.shape)
            patches = fe.tiles(origins, self.patch_size, out="float32", view=(1,) + self.patch_size)
        else:
            patches = self._split(self._preprocess(raw, normalization_mode, clip_threshold))
        mp = self._load_model(model_params, network)
        self.target_keys = list(mp["output_heads"].keys())
        self.result = _write_heads(result_path, self._predict_and_blend(patches, batch_size))

    def _build(self, mp, network):
        return network(in_channels=mp["in_channels"], n_filter=mp["n_filter"], output_heads=mp["output_heads"],
                       use_interpolation=mp.get("use_interpolation", True))

    @staticmethod
    def _preprocess(imgs, mode, clip):
        if mode == "single":
            for i in range(len(imgs)):
                c = np.clip(imgs[i], np.percentile(imgs[i], clip[0]), np.percentile(imgs[i], clip[1]))
                imgs[i] = (c - c.min()) / (np.ptp(c) + 1e-8)
            return imgs
        if mode in ("first", "all"):
            lo, hi = np.percentile(imgs[0] if mode == "first" else imgs, [clip[0], clip[1]])
            imgs[:] = (np.clip(imgs, lo, hi) - lo) / (hi - lo + 1e-8)
            return imgs
        raise ValueError(f"Invalid normalization mode: {mode}")

    def _origins(self, shape):
        """Patch grid of ``multi_output_unet3d/predict.py:162-201``: sets ``patch_size``, the start lists and the counts and returns the
        patch order as (volume, z, y, x) -- shared by the host ``_split``, the device front end and the blend."""
        nvol, D, H, W = shape
        self.patch_size = ps = tuple(min(a, b) for a, b in zip((D, H, W), self.max_patch_size))
        stride = [max(1, int(s * (1 - self.overlap_factor))) for s in ps]

        def starts(extent, patch, st):
            v = list(range(0, max(extent - patch + 1, 1), st))
            if v[-1] + patch < extent:
                v.append(extent - patch)
            return v
        self.Z_start, self.Y_start, self.X_start = starts(D, ps[0], stride[0]), starts(H, ps[1], stride[1]), starts(W, ps[2], stride[2])
        self.N_z, self.N_y, self.N_x = len(self.Z_start), len(self.Y_start), len(self.X_start)
        self.N_per_vol = self.N_z * self.N_y * self.N_x
        self.origins = [(v, z, y, x) for v in range(nvol) for z in self.Z_start for y in self.Y_start for x in self.X_start]
        return self.origins

    def _split(self, imgs):
        return _cut(imgs, self._origins(imgs.shape), self.patch_size)[:, None]

    def _weights(self, flags, shape, blend_margin):
        """Blend mask of one patch; ``flags`` = (front, back, top, bottom, left, right) interior faces.  Restates the
        assignment order of ``predict.py:246-268`` including its index arithmetic: the 'far' ramps all land on plane 0
        (``max(-(i+1), 0) == 0``) and the depth ramps run over ``min(blend_margin, N_z)`` planes."""
        w = np.ones(shape, dtype="float32")
        nz = min(blend_margin, self.N_z)
        if flags[0]:
            for i in range(nz):
                w[:, i, :, :] = i / blend_margin
        if flags[1]:
            for i in range(nz):
                w[:, 0, :, :] = i / blend_margin
        if flags[2]:
            for i in range(blend_margin):
                w[:, :, i, :] = i / blend_margin
        if flags[3]:
            for i in range(blend_margin):
                w[:, :, 0, :] = i / blend_margin
        if flags[4]:
            for i in range(blend_margin):
                w[:, :, :, i] = i / blend_margin
        if flags[5]:
            for i in range(blend_margin):
                w[:, :, :, 0] = i / blend_margin
        return w

    def _predict_and_blend(self, patches, batch_size, blend_margin=16):
        """Batches of patches through the network; every head's float32 patch is multiplied by its blend mask and added into
        the head's volume on the device, then ``vol / wsum`` where ``wsum > 0`` (``multi_output_unet3d/predict.py:203-307``)."""
        nvol, D, H, W = self.imgs_shape
        grid = (self.N_z, self.N_y, self.N_x)
        heads = self.model_params["output_heads"]
        stitch = _HeadStitch(self.device, heads, nvol, (D, H, W), grid,
                             lambda index, flags: self._weights(flags, (1,) + self.patch_size, blend_margin)[0])
        for b, x in self._batches(patches, batch_size):
            preds = self._forward(x)
            for j in range(x.shape[0]):
                vol, origin = self._place(b + j)
                stitch.add({k: preds[k][j].float() for k in heads}, vol, origin, np.unravel_index((b + j) % self.N_per_vol, grid))
        return {k: np.squeeze(torch.stack([s_.finish(False) for s_ in stitch[k]]).cpu().numpy()) for k in heads}


class PredictMo2d(_PredictBase):
    """``bio_image_unet.multi_output_unet.Predict`` counterpart (``multi_output_unet/predict.py:13-285``) for in-memory arrays (a path
    goes through ``tifffile`` when importable).

    Float normalisation to [0, 1] per ``normalization_mode`` (no uint8 step); patches of ``min(image, max_patch_size)`` rounded up to a
    multiple of 16, reflect padding when the image is smaller; origins ``linspace(...).astype('uint16')``; the model is built with
    ``train_mode=False`` and the checkpoint's ``deep_supervision``, in eval mode.  The reference runs the model in fp16 on CUDA; here
    the engine's dtype stays what it is (fp32, or bf16 after ``set_compute_dtype``) and each patch result is rounded to float16
    before stitching, because the reference stores patches as float16.  Every head is stitched on the device (``biu_stitch_add`` /
    ``biu_stitch_finish``) with a weight plane of 1 whose ``safe_margin = 20`` rows / columns are zeroed on every side that has a
    neighbour; pixels no patch weights get the (float16) mean of that head's patches (``:279``).

    As upstream, patches are cut on a stride of ``X_start[1]`` / ``Y_start[1]`` (``:180-181``) and stitched at ``X_start`` / ``Y_start``.
    ALL windows of that stride are cut and predicted, rows outermost, and every one counts in the fill mean; the first ``N_x * N_y`` of them
    are stitched, window ``k`` at ``(X_start[k // N_y], Y_start[k % N_y])``.  Where truncation makes the stride short (``add_tile`` on an extent
    barely larger than a patch) it yields more windows than tiles: surplus ROWS of windows come last and are only predicted, as upstream's
    ``[:N_per_img]`` leaves them out (pinned by ``tests/golden/predict_pins_mo2d.npz``, ``row_surplus``).  Surplus COLUMNS shift every later
    window to another tile in upstream's reshape, which scrambles the image, and with several images upstream's ``N_per_img`` no longer
    separates them, so patches of one image land in the next: both raise ``ValueError`` here.  ``result`` is a dict of arrays per head, or
    ``None`` when ``result_path`` is given and the heads were written to ``result_path + name + '.tif'``.

    ``preprocess='device'``: as for ``PredictMo3d`` -- fp64 on the device, rounded to float32 once, against numpy float32 on the host; NaN
    raises ``ValueError``."""

    safe_margin = 20

    def __init__(self, imgs, model_params, result_path=None, network=MultiOutputNestedUNet, max_patch_size=(1024, 1024), batch_size=1,
                 normalization_mode="single", clip_threshold=(0., 99.98), add_tile=0, compress_tif=False, show_progress=True,
                 device: Union[torch.device, str] = "auto", progress_notifier=None, preprocess="host"):
        raw = self._open(imgs, device, preprocess)
        self.max_patch_size, self.batch_size, self.add_tile = max_patch_size, batch_size, add_tile
        self.normalization_mode, self.clip_threshold, self.result_path = normalization_mode, clip_threshold, result_path
        if preprocess == "host" or not DeviceFrontEnd.native(raw.dtype):
            raw = np.array(raw, dtype="float32")                         # the host path's cast; the device path keeps small integers as they are
        self.imgs_shape = raw.shape
        if preprocess == "device":
            # the host path normalises in numpy float32 (percentiles included); here the same formula runs in fp64 on the uploaded values and
            # is rounded to float32 once
            fe = DeviceFrontEnd(raw, self.device)
            fe.normalise(normalization_mode, clip_threshold)
            origins = self._origins()
            patches = fe.tiles(origins, (1,) + self.patch_size, out="float32")
        else:
            patches = self._split(self._preprocess(raw, normalization_mode, clip_threshold))
        mp = self._load_model(model_params, network)
        self.target_keys = list(mp["output_heads"].keys())
        self.result = _write_heads(result_path, self._predict_and_stitch(patches, batch_size))

    def _build(self, mp, network):
        return network(in_channels=mp["in_channels"], n_filter=mp["n_filter"], output_heads=mp["output_heads"],
                       deep_supervision=mp.get("deep_supervision", False), train_mode=False)

    @staticmethod
    def _preprocess(imgs, mode, clip):
        """Percentile clip, then to [0, 1] (``predict.py:129-151``; lower bound ``nanpercentile``, upper ``percentile``)."""
        return _percentile_rescale(imgs, mode, clip)

    @staticmethod
    def geometry(imgs_shape, max_patch_size, add_tile):
        """Tiling of ``predict.py:153-177``: (patch_size, N_x, N_y, padded extents, X_start, Y_start)."""
        _, h, w = imgs_shape
        ph = (min(h, max_patch_size[0]) + 15) // 16 * 16
        pw = (min(w, max_patch_size[1]) + 15) // 16 * 16
        n_x = int(np.ceil(h / ph)) + add_tile
        n_y = int(np.ceil(w / pw)) + add_tile
        H, W = h + max(ph - h, 0), w + max(pw - w, 0)
        return (ph, pw), n_x, n_y, (H, W), tile_starts(H, ph, n_x), tile_starts(W, pw, n_y)

    @classmethod
    def weight_plane(cls, j, k, n_x, n_y, patch_size):
        """Ones with ``safe_margin`` rows / columns zeroed on every side of tile (j, k) that has a neighbour (``predict.py:259-269``)."""
        w, m = np.ones(patch_size, dtype="float32"), cls.safe_margin
        if j > 0:
            w[:m, :] = 0
        if j < n_x - 1:
            w[-m:, :] = 0
        if k > 0:
            w[:, :m] = 0
        if k < n_y - 1:
            w[:, -m:] = 0
        return w

    def _strides(self):
        """``geometry`` into the attributes, and the stride the patches are cut on: ``X_start[1]`` / ``Y_start[1]`` (``predict.py:180-181``)."""
        self.patch_size, self.N_x, self.N_y, self.padded, self.X_start, self.Y_start = self.geometry(self.imgs_shape, self.max_patch_size, self.add_tile)
        self.N_per_img = self.N_x * self.N_y
        self.N = self.N_per_img * self.imgs_shape[0]
        sx = int(self.X_start[1]) if self.N_x > 1 else 1
        sy = int(self.Y_start[1]) if self.N_y > 1 else 1
        if sx < 1 or sy < 1:
            raise ValueError("slice step cannot be zero (add_tile on an image no larger than one patch)")      # as upstream's view[::0]
        return sx, sy

    def _origins(self):
        """The windows ``_split`` takes, as (image, 0, row, column) in the reflect-padded stack: every window of the stride that fits, rows
        outermost -- what the device front end cuts.  The first ``N_per_img`` are the tiles; a surplus row of windows (one image only)
        follows them and is predicted without being stitched.  Raises ``ValueError`` where upstream's result is scrambled (class docstring)."""
        sx, sy = self._strides()
        (ph, pw), (H, W) = self.patch_size, self.padded
        rows = list(range(0, H - ph + 1, sx))
        cols = list(range(0, W - pw + 1, sy))
        assert len(rows) >= self.N_x and len(cols) >= self.N_y          # a stride truncated downwards never yields fewer windows
        where = f"images {tuple(self.imgs_shape)}, max_patch_size {tuple(self.max_patch_size)}, add_tile {self.add_tile}"
        if len(cols) > self.N_y:
            raise ValueError(f"PredictMo2d: the column stride {sy} yields {len(cols)} windows for N_y = {self.N_y} tiles ({where}); upstream "
                             "reshapes the longer list to N_x x N_y and scrambles the image.  Use another add_tile or max_patch_size")
        if len(rows) > self.N_x and self.imgs_shape[0] > 1:
            raise ValueError(f"PredictMo2d: the row stride {sx} yields {len(rows)} windows for N_x = {self.N_x} tiles ({where}); with several "
                             "images upstream stitches patches of one image into the next.  Predict the images one by one, or use "
                             "another add_tile or max_patch_size")
        self.origins = [(i, 0, r, c) for i in range(self.imgs_shape[0]) for r in rows for c in cols]
        return self.origins

    def _place(self, k):
        """Window ``k`` of the cut list goes to its image at ``(X_start[j], Y_start[c])``, (j, c) being its place in the image's grid: the
        origin it was cut at wherever the stride ``X_start[1]`` reproduces ``X_start`` (always with up to two tiles per axis), and upstream's
        choice (``predict.py:252-253``) where truncation makes the two drift apart.  ``None`` for a surplus window, which is not stitched."""
        if len(self.origins) > self.N and k >= self.N_per_img:
            return None
        j, c = divmod(k % self.N_per_img, self.N_y)
        return self.origins[k][0], (0, int(self.X_start[j]), int(self.Y_start[c]))

    def _split(self, imgs):
        return _cut(imgs[:, None], self._origins(), (1,) + self.patch_size)[:, 0]

    def _predict_and_stitch(self, patches, batch_size):
        n_img, h, w = self.imgs_shape
        ph, pw = self.patch_size
        cin, grid = self.model_params["in_channels"], (self.N_x, self.N_y)
        heads = self.model_params["output_heads"]
        stitch = _HeadStitch(self.device, heads, n_img, (1, max(ph, h), max(pw, w)), grid,
                             lambda index, flags: self.weight_plane(*index, *grid, self.patch_size)[None])
        sums = {k: torch.zeros((), dtype=torch.float64, device=self.device) for k in heads}
        for b, x in self._batches(patches, batch_size):
            x = x.view(-1, cin, ph, pw)
            out, p16 = self._forward(x), {}
            for key, cfg in heads.items():
                want = (x.shape[0], cfg["channels"], ph, pw)
                if tuple(out[key].shape) != want:
                    raise RuntimeError(f"Shape mismatch for target key '{key}': predicted {tuple(out[key].shape)}, expected {want}")
                p16[key] = out[key].to(torch.float16).float()       # the reference keeps patches as float16
                sums[key] += p16[key].double().sum()
            for i in range(x.shape[0]):
                at = self._place(b + i)
                if at is not None:                                  # (a surplus window has been counted in the fill mean above, no more)
                    stitch.add({key: p[i].unsqueeze(1) for key, p in p16.items()}, *at, divmod((b + i) % self.N_per_img, self.N_y))
        result = {}
        for key, cfg in heads.items():
            fill = float(np.float16(float(sums[key]) / (len(patches) * cfg["channels"] * ph * pw)))      # np.mean of a float16 array is float16
            done = [torch.where(s_.wsum[0].unsqueeze(0) > 0, s_.finish(False), torch.full((), fill, device=self.device)) for s_ in stitch[key]]
            res = torch.stack(done).cpu().numpy()[:, :, 0]               # (n_img, channels, H, W)
            result[key] = np.squeeze(res[:, :, :h, :w])
        return result
