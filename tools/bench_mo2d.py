"""Train-step time of the 2-D multi-output networks: MultiOutputNestedUNet (two heads) and MultiOutputUnet at batch 4, 256 x 256.

    python tools/bench_mo2d.py [--steps 10] [--warmup 3] [--cases all|nested_f64_bf16,...] [--oracle]

One step = forward + the reference trainer's loss (weighted MSE, per-level supervision weights with deep supervision) + backward +
clip_grad_norm_(1.0) + Adam, both as the fused kernels of bio_image_unet_amd.optim.  Timing: device events around `--steps` steps after
`--warmup` untimed ones.  Prints one JSON line per case: ms/step, which concatenations the two-source kernels serve and which fall back
to a copy, and -- from one extra step timed per library call -- the bilinear kernels' share of the step and their achieved bandwidth
(the bytes the op must move: coarse read + fine write forward, fine read + coarse write backward, not counting the extra coarse read
of an accumulating backward).
`--oracle`: tests/mo2d_oracle.py run eagerly by PyTorch on the same GPU, an informative comparator (fp32 cases only).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bio_image_unet_amd as B  # noqa: E402
from bio_image_unet_amd import _lib  # noqa: E402
from bio_image_unet_amd import engine as E  # noqa: E402
from bio_image_unet_amd.optim import Adam  # noqa: E402

HEADS = {"seg": {"channels": 1, "activation": "sigmoid", "weight": 1.0}, "dist": {"channels": 1, "activation": None, "weight": 0.5}}
SHAPE = (4, 1, 256, 256)
SUP = [0.5, 0.75, 0.875, 1.0]


def cases():
    out = {}
    for f in (64, 32):
        for dt in ("bf16", "fp32"):
            for ds in (False, True):
                out[f"nested_f{f}_{dt}{'_ds' if ds else ''}"] = (B.MultiOutputNestedUNet, f, dt, ds)
    for dt in ("bf16", "fp32"):
        out[f"mo2d_f64_{dt}"] = (B.MultiOutputUnet, 64, dt, False)
    return out


def loss_of(out, tg, ds):
    total = 0
    for name, cfg in HEADS.items():
        if ds:
            for lvl, sw in enumerate(SUP, 1):
                total = total + sw * cfg["weight"] * torch.nn.functional.mse_loss(out[f"{name}_{lvl}"], tg[name])
        else:
            total = total + cfg["weight"] * torch.nn.functional.mse_loss(out[name], tg[name])
    return total


def bilinear_bytes(eng):
    """Bytes each bilinear node's forward and backward must move, by direction."""
    es = 2 if eng.tdtype == torch.bfloat16 else 4
    fwd = bwd = 0
    for nd in eng.nodes:
        if isinstance(nd, E.ResampleNode) and nd.kind == "bilinear":
            lo, hi = nd.xin.nvox * nd.xin.c * es, nd.y.nvox * nd.y.c * es
            fwd += lo + hi
            bwd += hi + lo
    return fwd, bwd


def run(name, cls, f, dt, ds, steps, warmup, oracle):
    torch.manual_seed(0)
    kw = dict(in_channels=1, output_heads=HEADS, n_filter=f)
    if cls is B.MultiOutputNestedUNet:
        kw["deep_supervision"] = ds
    m = cls(**kw).cuda().train()
    if dt == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(SHAPE, device="cuda", generator=g)
    tg = {n: torch.rand((SHAPE[0], c["channels"]) + SHAPE[2:], device="cuda", generator=g) for n, c in HEADS.items()}
    opt = Adam(m.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_of(m(x), tg, ds)
        loss.backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    assert torch.isfinite(loss).item(), "non-finite loss"
    eng = list(m._engines.values())[-1][-1]
    paths = getattr(eng, "cat_paths", {})
    res = dict(case=name, model=cls.__name__, n_filter=f, dtype=dt, deep_supervision=ds, shape=list(SHAPE), ms_per_step=round(ms, 3),
               two_source=sorted(k for k, v in paths.items() if v == "two-source"), copy=sorted(k for k, v in paths.items() if v == "copy"))
    if cls is B.MultiOutputNestedUNet:
        _lib.lib.prof = []                  # one more step with every library call timed by events
        step()
        torch.cuda.synchronize()
        calls = [(n, e0_.elapsed_time(e1_)) for n, _, e0_, e1_ in _lib.lib.prof]
        _lib.lib.prof = None
        tot = sum(t for _, t in calls)
        bf = sum(t for n, t in calls if n == "biu_bilinear_up_fwd")
        bb = sum(t for n, t in calls if n == "biu_bilinear_up_bwd")
        fb, bbytes = bilinear_bytes(eng)
        res.update(bilinear_fwd_ms=round(bf, 3), bilinear_bwd_ms=round(bb, 3), bilinear_share_of_library_time=round((bf + bb) / tot, 4),
                   bilinear_fwd_TBps=round(fb / (bf * 1e-3) / 1e12, 2), bilinear_bwd_TBps=round(bbytes / (bb * 1e-3) / 1e12, 2))
    if oracle and dt == "fp32":
        from tests import mo2d_oracle as M
        sd = {k: v.detach().clone().requires_grad_(k.endswith((".weight", ".bias"))) if v.is_floating_point() else v.clone()
              for k, v in m.state_dict().items()}
        fwd = (lambda: M.nested_forward(sd, x, HEADS, deep_supervision=ds)) if cls is B.MultiOutputNestedUNet else (lambda: M.mo2d_forward(sd, x, HEADS))
        for _ in range(2):
            loss_of(fwd(), tg, ds).backward()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(3):
            loss_of(fwd(), tg, ds).backward()
        e1.record()
        torch.cuda.synchronize()
        res["eager_pytorch_oracle_ms_fwd_bwd"] = round(e0.elapsed_time(e1) / 3, 3)
    print(json.dumps(res), flush=True)
    del m, opt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="all")
    ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    cs = cases()
    for name in (cs if a.cases == "all" else a.cases.split(",")):
        run(name, *cs[name], a.steps, a.warmup, a.oracle)


if __name__ == "__main__":
    main()
