"""Times the first-layer calls (biu_conv_fwd_stats, biu_conv_bwd_weight_bn) for 1 to 4 input channels, bf16 and fp32, by device events:
  3-D  4 x Cin x 128^3 -> 16 channels        2-D  16 x Cin x 512^2 -> 64 channels
on the first-layer kernels and, in a fresh child process with BIU_DISABLE=cn, on the route 2 to 4 input channels took before (the
any-shape kernels, plus the separate BatchNorm passes).  Each time is also given as a multiple of the HBM time of the layer's output
tensor (cout x voxels x element size at 8 TB/s, the figure bench.py and profiles/ use).  The first-layer run is made twice: the
difference between the two, and between them and the cn-off run on the Cin = 1 rows (same kernels), is the run-to-run spread.

    python tools/bench_first_layer.py --out profiles/r15_first_layer_cn.txt
    python tools/bench_first_layer.py --root OTHER_CHECKOUT      # time another built checkout of this package (e.g. the parent commit)"""
import argparse
import json
import os
import subprocess
import sys

HBM_PEAK = 8.0e12
SHAPES = [("3-D 4xCx128^3->16", 3, (4, 128, 128, 128), 16), ("2-D 16xCx512^2->64", 1, (16, 1, 512, 512), 64)]


def child(args):
    sys.path.insert(0, args.root)
    import ctypes as C
    import torch
    from bio_image_unet_amd import _lib as L
    lib, check = L.lib, L.check
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def timeit(f):
        for _ in range(args.warmup):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    rows = []
    for name, kd, (n, d, h, w), cout in SHAPES:
        nd = 3 if kd == 3 else 2
        for dtype, code, tdt in (("bf16", L.BIU_BF16, torch.bfloat16), ("f32", L.BIU_F32, torch.float32)):
            y = torch.randn(n, d, h, w, cout, device="cuda").to(tdt)
            da = torch.randn(n, d, h, w, cout, device="cuda").to(tdt)
            ay, ada = L.biu_act(y.data_ptr(), n, d, h, w, cout, cout), L.biu_act(da.data_ptr(), n, d, h, w, cout, cout)
            one, zero = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")      # dy = da: the in-place update stays bounded
            nfl = lib.biu_conv_fwd_stats_floats(C.byref(ay), kd)
            part = torch.empty(nfl, device="cuda")
            nblk = C.c_int(0)
            for cin in (1, 2, 3, 4):
                x = torch.rand(n, d, h, w, cin, device="cuda").to(tdt)
                ax = L.biu_act(x.data_ptr(), n, d, h, w, cin, cin)
                wt = torch.randn(cout, cin, *([3] * nd), device="cuda")
                b, dw = torch.randn(cout, device="cuda"), torch.empty_like(wt)
                wsz = lib.biu_conv_bwd_weight_workspace(cin, cout, kd, 3, 3, code)
                if "biu_conv_first_workspace" in L.SIGNATURES:
                    wsz = max(wsz, lib.biu_conv_first_workspace(cin, cout, kd, code))
                ws = torch.empty(max(wsz, 16), dtype=torch.uint8, device="cuda")
                fw = lambda: check(lib.biu_conv_fwd_stats(C.byref(ax), None, p(wt), None, p(b), kd, 3, 3, 1, C.byref(ay), p(part), nfl, C.byref(nblk),
                                                          None, 0, code, st), "conv_fwd_stats")
                wg = lambda: check(lib.biu_conv_bwd_weight_bn(C.byref(ax), None, C.byref(ada), C.byref(ay), p(one), p(zero), p(one), p(one), p(zero),
                                                              p(zero), kd, 3, 3, 1, p(dw), p(ws), ws.numel(), code, st), "conv_bwd_weight_bn")
                hbm_ms = cout * n * d * h * w * (2 if dtype == "bf16" else 4) / HBM_PEAK * 1e3
                rows.append(dict(shape=name, dtype=dtype, cin=cin, hbm_ms=hbm_ms, fwd_stats=timeit(fw), wgrad_bn=timeit(wg)))
                print(f"# {name} {dtype} cin {cin}: fwd_stats {rows[-1]['fwd_stats']:.3f} ms, wgrad_bn {rows[-1]['wgrad_bn']:.3f} ms", file=sys.stderr, flush=True)
    print("ROWS " + json.dumps(rows))


def run_child(args, disable, reps):
    env = dict(os.environ)
    env["BIU_DISABLE"] = ",".join(t for t in (os.environ.get("BIU_DISABLE", ""), disable) if t)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", args.root, "--reps", str(reps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        raise SystemExit(f"child ({disable or 'default'}) failed with {r.returncode}")
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("ROWS "))[5:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose built package is timed")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--off-reps", type=int, default=5, help="timed calls per row of the BIU_DISABLE=cn run (the any-shape kernels are slow)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["new", "off"], default=None, help="one run only (new: the default routing, off: BIU_DISABLE=cn)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = [f"# tools/bench_first_layer.py: device-event times after {args.warmup} warm-up calls, ms per call; 'xHBM' = time / (output tensor bytes / 8 TB/s)"]
    if args.only:
        rows = run_child(args, "cn" if args.only == "off" else "", args.off_reps if args.only == "off" else args.reps)
        lines.append(f"# one run ({'BIU_DISABLE=cn' if args.only == 'off' else 'default routing'}) of {args.root}")
        for r in rows:
            lines.append(f"{r['shape']:20s} {r['dtype']:5s} cin {r['cin']}   fwd_stats {r['fwd_stats']:9.3f} ({r['fwd_stats'] / r['hbm_ms']:8.1f} xHBM)   "
                         f"wgrad_bn {r['wgrad_bn']:9.3f} ({r['wgrad_bn'] / r['hbm_ms']:8.1f} xHBM)")
    else:
        a, b, off = run_child(args, "", args.reps), run_child(args, "", args.reps), run_child(args, "cn", args.off_reps)
        lines.append(f"# new: first-layer kernels (two runs of {args.reps} calls, the first one listed); cn off: BIU_DISABLE=cn in a fresh process ({args.off_reps} calls)")
        lines.append(f"{'shape':20s} {'dtype':5s} cin  {'op':10s} {'new ms':>9s} {'xHBM':>8s} {'cn-off ms':>10s} {'xHBM':>8s} {'off/new':>8s}")
        spread, spread1 = 0.0, 0.0
        for ra, rb, ro in zip(a, b, off):
            for op in ("fwd_stats", "wgrad_bn"):
                lines.append(f"{ra['shape']:20s} {ra['dtype']:5s} {ra['cin']:3d}  {op:10s} {ra[op]:9.3f} {ra[op] / ra['hbm_ms']:8.1f} {ro[op]:10.3f} "
                             f"{ro[op] / ro['hbm_ms']:8.1f} {ro[op] / ra[op]:8.2f}")
                spread = max(spread, abs(ra[op] - rb[op]) / min(ra[op], rb[op]))
                if ra["cin"] == 1:
                    spread1 = max(spread1, abs(ra[op] - ro[op]) / min(ra[op], ro[op]))
        lines.append(f"# run-to-run spread: largest |run 1 - run 2| / min over all rows {100 * spread:.1f} %; Cin = 1 rows, new against cn off (same kernels) {100 * spread1:.1f} %")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
