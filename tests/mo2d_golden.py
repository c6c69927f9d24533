"""The fixtures of the 2-D multi-output networks (tests/golden/make_golden_mo2d.py): case list, model construction from a fixture's
meta, and the oracle forward / loss the fixture was driven with."""
import bio_image_unet_amd as B
from tests import mo2d_oracle as M

CASES = ["mo2d_f2", "nested_f2", "nested_f2_ds", "nested3_f4_ds"]
CLASSES = {"MultiOutputUnet": B.MultiOutputUnet, "MultiOutputNestedUNet": B.MultiOutputNestedUNet,
           "MultiOutputNestedUNet_3Levels": B.MultiOutputNestedUNet_3Levels}


def build(meta):
    return CLASSES[meta["model"]](**meta["ctor"])


def targets(g):
    return {k.split(".", 1)[1]: v for k, v in g["in"].items() if k.startswith("target.")}


def forward(g, sd, x, training):
    meta = g["meta"]
    ctor = meta["ctor"]
    if meta["model"] == "MultiOutputUnet":
        return M.mo2d_forward(sd, x, ctor["output_heads"], training=training)
    return M.nested_forward(sd, x, ctor["output_heads"], levels=meta["levels"], deep_supervision=ctor.get("deep_supervision", False),
                            dilation=ctor.get("dilation", False), training=training)


def loss(g, outs, tg):
    ctor = g["meta"]["ctor"]
    return M.weighted_mse(outs, tg, ctor["output_heads"], deep_supervision=ctor.get("deep_supervision", False), levels=g["meta"]["levels"])
