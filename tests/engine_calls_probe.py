"""Helper of test_gpu_engine_calls, run as a subprocess so that the switches read once per process (BIU_DISABLE, BIU_FOLDT, BIU_ROLL,
BIU_SIDE_WGRAD_VOX) are the case's own: every library call the passes of one case issue, in issue order, as (api, label) pairs.

  CASE OUT   builds the case's network and its engine, then records through ``lib.prof`` while the passes run; OUT is a JSON file
             {"calls": [[api, label], ...], "heads": number of heads, "trunks": number of distinct tensors the heads read}

The engine is built before recording starts: the list is the launch sequence (and the host-side queries made between launches), not the
sizing queries of graph construction."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bio_image_unet_amd as B  # noqa: E402
from bio_image_unet_amd._lib import lib  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

case, out = sys.argv[1], sys.argv[2]
torch.manual_seed(0)
g = torch.Generator().manual_seed(5)
passes = ["train"]
if case in ("unet3d_bf16", "unet3d_bf16_rank1"):
    m = B.UNet3D(1, 1, 32).cuda()
    m.load_state_dict(O.init_unet3d(1, 1, 32, seed=7))
    m.set_compute_dtype(torch.bfloat16)
    shape = (2, 1, 16, 32, 32) if case == "unet3d_bf16" else (2, 1, 16, 16, 32)
elif case == "mo3d_interp_bf16":
    heads = {"seg": {"channels": 1, "activation": None}}
    m = B.MultiOutputUnet3D(1, heads, 32, True).cuda()
    m.load_state_dict(O.init_mo3d(1, heads, 32, True, seed=9))
    m.set_compute_dtype(torch.bfloat16)
    shape = (2, 1, 32, 64, 64)
elif case == "unet2d_f32":
    m = B.Unet(1, 1, 32).cuda()
    m.load_state_dict(O.init_unet2d(1, 1, 32, seed=3))
    shape = (2, 1, 64, 64)
    passes = ["train", "eval_nograd", "eval_grad"]
elif case in ("nested_ds", "siam_concat"):
    from tests.golden_util import load_case
    fx = load_case("nested_f2_ds" if case == "nested_ds" else "siam_f4_concat")
    if case == "nested_ds":
        from tests import mo2d_golden as MG
        m = MG.build(fx["meta"]).cuda()
    else:
        m = B.Siam_UNet(**fx["meta"]["ctor"]).cuda()
    m.load_state_dict(fx["sd"])
    shape = None
else:
    raise SystemExit(f"unknown case {case}")

if shape is not None:
    ins = [torch.rand(*shape, generator=g).cuda()]
    y = (torch.rand(*shape, generator=g) > 0.5).float().cuda()

    def loss_of(outs):
        return O.bce_dice_loss(outs["seg"] if isinstance(outs, dict) else outs[1], y)
elif case == "nested_ds":
    ins = [fx["in"]["x"].cuda()]
    tg = {k: v.cuda() for k, v in MG.targets(fx).items()}

    def loss_of(outs):
        return MG.loss(fx, outs, tg)
else:
    ins = [fx["in"]["x"].cuda(), fx["in"]["prev_x"].cuda()]
    y = fx["in"]["target"].cuda()

    def loss_of(outs):          # the Siam package's own BCEDice, as the fixture was driven (tests/test_oracle_golden.oracle_loss)
        return O.siam_bce_dice_loss(outs[1], y, 1.0, 1.0)

m.train()
eng = m._engine_for(*ins)
lib.prof = []
for p in passes:
    m.train(p == "train")
    if p == "eval_nograd":
        with torch.no_grad():
            m(*ins)
    else:
        m.zero_grad()
        loss_of(m(*ins)).backward()
torch.cuda.synchronize()
calls = [[name, label] for name, label, _, _ in lib.prof]
lib.prof = None
with open(out, "w") as f:
    json.dump({"calls": calls, "heads": len(eng.heads), "trunks": len({id(h.xin) for h in eng.heads})}, f)
