"""bio_image_unet_amd -- MI355X-native drop-in for the U-Net forward/backward hot path of danihae/bio-image-unet.

``import bio_image_unet_amd.unet as unet`` mirrors ``import bio_image_unet.unet as unet`` for the model classes
(and the Trainer / Predict counterparts that drive them).  All arithmetic runs in hand-written HIP kernels behind
the C ABI of ``include/biu.h``; importing the package fails if ``libbiu_hip.so`` has not been built.
"""
from . import _lib                      # noqa: F401  (raises ImportError when the HIP library is missing)
from .models import (AttentionUnet, BabyUnet, MultiOutputNestedUNet, MultiOutputNestedUNet_3Levels, MultiOutputUnet,  # noqa: F401
                     MultiOutputUnet3D, Siam_UNet, UNet3D, Unet, Unet_v0)

__version__ = "0.1.0"


def set_fp32_products(mode: str) -> None:
    """How the fp32 2-D 3x3 convolution / ConvTranspose kernels multiply (the 3-D kernels: ``set_fp32_products_3d``):

    * ``"bf16x6"`` (default): every fp32 operand is split hi + mid + lo in bf16 (24 significant bits) and a product is the six bf16 MFMA terms
      of order >= 2^-16, accumulated in fp32 -- <= 2^-22 relative per product (measured worst 2^-22.6), i.e. fp32-grade, at 2.7x the matrix-pipe rate of the fp32 MFMA;
    * ``"exact"``: ``v_mfma_f32_32x32x2_f32`` (fp32 FMA chains);
    * ``"bf16x3"`` (opt-in): hi + lo, three terms, <= 2^-15 relative per product, another 2x -- the counterpart of
      ``torch.backends.cudnn.allow_tf32`` for the reference's fp32 trainers.

    Process-wide, to be called before the first forward (``include/biu.h: biu_set_fp32_products``; environment: ``BIU_FP32_PRODUCTS``)."""
    modes = {"exact": 0, "bf16x3": 1, "bf16x6": 2}
    if mode not in modes:
        raise ValueError(f"set_fp32_products: {mode!r} (expected one of {sorted(modes)})")
    _lib.check(_lib.lib.biu_set_fp32_products(modes[mode]), "set_fp32_products")


def set_fp32_products_3d(mode: str) -> None:
    """How the fp32 3-D kernels -- 3x3x3 convolution, ConvTranspose3d k2 s2, the skip half of a folded decoder level -- multiply:

    * ``"exact"`` (default): ``v_mfma_f32_32x32x2_f32`` (fp32 FMA chains);
    * ``"bf16x6"`` (opt-in): every fp32 operand is split hi + mid + lo in bf16 and a product is the six bf16 MFMA terms of order >= 2^-16,
      accumulated in fp32 -- <= 2^-22 relative per product (measured worst 2^-22.6), i.e. fp32-grade;
    * ``"bf16x3"`` (opt-in): hi + lo, three terms, <= 2^-15 relative per product -- the counterpart of ``torch.backends.cudnn.allow_tf32``.

    Launches with fewer than 16 (or a non-multiple of 16) reduction channels stay exact, as do 3x3x3 launches too wide for LDS (more than
    1328 / 3056 reduction channels) and the data gradient of ConvTranspose3d.  Independent of ``set_fp32_products``, which governs the 2-D kernels only.  Process-wide, to be called before the first
    forward (``include/biu.h: biu_set_fp32_products_3d``; environment: ``BIU_FP32_PRODUCTS_3D``)."""
    modes = {"exact": 0, "bf16x3": 1, "bf16x6": 2}
    if mode not in modes:
        raise ValueError(f"set_fp32_products_3d: {mode!r} (expected one of {sorted(modes)})")
    _lib.check(_lib.lib.biu_set_fp32_products_3d(modes[mode]), "set_fp32_products_3d")
