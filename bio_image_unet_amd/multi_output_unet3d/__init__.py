from ..models import MultiOutputUnet3D  # noqa: F401
from ..workflow import PredictMo3d as Predict, TrainerMo3d as Trainer   # noqa: F401
from ..dataprep import prepare_mo3d as prepare   # noqa: F401  (raw volumes and NaN-labelled targets -> feed.VolumeStore, on the device)
from . import losses  # noqa: F401
from .losses import (BCEDiceLoss, BCEDiceTemporalLoss, DiceLoss, MultiHeadLoss, TemporalConsistencyLoss, TverskyLoss,  # noqa: F401
                     logcoshTverskyLoss)
