"""Mirror of ``bio_image_unet.multi_output_unet``: the 2-D multi-output U-Net and the nested U-Net++ (four and three levels), their
``Trainer`` / ``Predict`` counterparts and the criteria (``losses``: fused HIP passes on the activated head outputs).  The reference's
own 2-D ``Trainer`` also takes these network classes through ``network=``."""
from ..models import MultiOutputNestedUNet, MultiOutputNestedUNet_3Levels, MultiOutputUnet  # noqa: F401
from ..dataprep import prepare_mo2d as prepare   # noqa: F401  (raw arrays and NaN-labelled targets -> feed.ImageStore, on the device)
from ..workflow import PredictMo2d as Predict, TrainerMo2d as Trainer  # noqa: F401
from . import losses  # noqa: F401
from .losses import (BCEDiceLoss, DistanceGradientLoss, HuberLoss, MAELoss, MSELoss, MultiHeadLoss, TverskyLoss,  # noqa: F401
                     WeightedDistanceGradientLoss, WeightedVectorFieldLoss, gradient_loss, logcoshTverskyLoss)
