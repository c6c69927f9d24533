"""Step time of an fp32 3-D training step under the three product modes of the 3-D kernels (BIU_FP32_PRODUCTS_3D = exact | bf16x3 | bf16x6).

    python tools/bench_fp32_3d.py [--workload cfg4|cfg5] [--passes 3] [--steps 10] [--warmup 3]

cfg4: UNet3D(1, 1, 32) fp32 at (4, 1, 128, 128, 128); cfg5: MultiOutputUnet3D(1, 3 heads, 64, interpolation) fp32 at cfg5's shape.  One step =
forward + the reference loss + backward + fused Adam on synthetic seeded data (bench.make_step, every step from the seeded weights).  The
mode is process-wide, so each (pass, mode) runs in a child process of its own; the modes alternate over the passes on the same device.
Timing: device events around `--steps` steps after `--warmup` untimed ones.  Prints one JSON line per mode (ms/step of every pass, median,
spread) and the matrix-pipe ceiling the mode's split launches run against: bf16 peak / 3 (bf16x3) or / 6 (bf16x6), the fp32 MFMA peak (exact).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["exact", "bf16x6", "bf16x3"]


def child(workload, steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    wl = dict(bench.WORKLOADS[workload], dtype="f32")
    _, step, _, nvox, _ = bench.make_step(wl, torch.device("cuda:0"), keep_outputs=True)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        loss = step()
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item(), "non-finite loss"
    # checksum of the last step's outputs (every step starts from the seeded weights): differs between the modes when the split kernels ran
    outs = step.last["outs"]
    outs = list(outs.values()) if isinstance(outs, dict) else list(outs)
    chk = float(sum(o.double().abs().sum() for o in outs))
    print("RESULT " + json.dumps({"ms": t0.elapsed_time(t1) / steps, "loss": float(loss), "out_abs_sum": chk, "nvox": nvox}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4", choices=["cfg4", "cfg5"])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.workload, a.steps, a.warmup)
        return
    sys.path.insert(0, ROOT)
    import bench
    ceiling = {"exact": bench.MFMA_PEAK["f32"], "bf16x3": bench.MFMA_PEAK["bf16"] / 3, "bf16x6": bench.MFMA_PEAK["bf16"] / 6}
    res = {m: [] for m in MODES}
    for p in range(a.passes):
        for m in (MODES if p % 2 == 0 else MODES[::-1]):
            env = dict(os.environ, BIU_FP32_PRODUCTS_3D=m)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-3000:])
                raise SystemExit(f"{m}: child exited with {r.returncode}")
            line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
            res[m].append(json.loads(line[7:]))
    exact_med = None
    for m in MODES:
        ms = sorted(r["ms"] for r in res[m])
        med = ms[len(ms) // 2]
        exact_med = med if m == "exact" else exact_med
        print(json.dumps({"workload": a.workload + "_f32", "products_3d": m, "ms_per_step": [round(r["ms"], 3) for r in res[m]],
                          "median_ms": round(med, 3), "spread_ms": round(ms[-1] - ms[0], 3), "speedup_vs_exact": round(exact_med / med, 3),
                          "loss": res[m][-1]["loss"], "out_abs_sum": res[m][-1]["out_abs_sum"], "ceiling_tflops": round(ceiling[m] / 1e12, 1)}))


if __name__ == "__main__":
    main()
