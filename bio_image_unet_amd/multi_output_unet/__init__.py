"""Mirror of ``bio_image_unet.multi_output_unet``: the 2-D multi-output U-Net and the nested U-Net++ (four and three levels).  The
reference's own 2-D ``Trainer`` takes these classes through ``network=``."""
from ..models import MultiOutputNestedUNet, MultiOutputNestedUNet_3Levels, MultiOutputUnet  # noqa: F401
