#!/usr/bin/env python3
"""How many rounds does a block of a persistent convolution launch walk in the test suite?  (profiles/r10_walk_rounds.txt)

  1. the audit: every case of tests/test_gpu_ops.py that reaches an MFMA kernel, with the bricks of its launches, the blocks per column
     (tests/walk_geometry.py mirrors the launch functions) and the rounds = ceil(bricks / blocks) -- 1 means every block runs one brick and stops;
  2. the cases of tests/test_gpu_walk.py, from the `WALK` lines of a pytest log of that file (pytest -rA prints them), with the worst
     deviation of each as a fraction of its tolerance.

A SNAPSHOT, not a mirror to maintain: conv_launch, wgrad_launch and roll_items below restate the dispatch of biu_mfma_conv / biu_mfma_wgrad /
roll_plan as it stood when profiles/r10_walk_rounds.txt was written, for the one-off audit of part 1.  No test reads them and none should: the
record is the profile, and the geometry the tests rely on is tests/walk_geometry.py alone.  Part 2 only copies lines of a pytest log.

usage: python tools/walk_rounds.py [--cus N] [--log pytest.log]        (N defaults to the CU count of device 0)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("BIU_FOLDT", "always")          # as tests/conftest.py: the kernels the suite's cases take
os.environ.setdefault("BIU_ROLL", "always")

from tests import walk_geometry as G  # noqa: E402


def cdiv(a, b):
    return -(-a // b)


def roll_items(cus, n, sp, cols):
    """roll_plan: 8 x 32 windows x depth segments of at least 8 planes while the windows alone do not fill the column's blocks."""
    d, h, w = sp
    ncols = n * cdiv(h, 8) * cdiv(w, 32)
    budget = max(cus // cols, 1)
    nseg = 1
    while ncols * nseg < budget and d // (nseg * 2) >= 8:
        nseg *= 2
    seg = (cdiv(d, nseg) + 1) // 2 * 2
    return ncols * cdiv(d, seg)


def conv_launch(cus, nd, dtype, k, nout, n, sp, single=True):
    """(row, columns, bricks) of the 3x3(x3) launch that reduces k channels and writes nout (biu_mfma_conv's dispatch order)."""
    if single and dtype == "bf16" and nd == 3 and k in (16, 32) and ((nout == 16 and k == 32) or nout == 32) and sp[0] >= 4:
        cols = 1
        return "roll", cols, roll_items(cus, n, sp, cols)
    if single and dtype == "bf16" and k >= 32 and k % 32 == 0 and (nout == 16 or (k == 32 and nout % 32 == 0)):
        row = "conv16_3d" if nd == 3 else "conv16_2d"
        return row, nout // (16 if nout == 16 else 32), G.bricks(row, n, sp)
    ntiles = cdiv(nout, 32)
    nt = G.pick_nt(ntiles)
    wide = sp[-1] % 32 == 0
    row = "conv%dd_nt%d" % (nd, nt) + ("" if (nd == 3 and nt == 2) else ("_wide" if wide else "_narrow"))
    return row, ntiles // nt, G.bricks(row, n, sp)


def wgrad_launch(nd, dtype, cin, cout, n, sp):
    windows = cdiv(sp[-2], 8) * cdiv(sp[-1], 16)
    if dtype == "f32":
        row = "wgrad3d_f32" if nd == 3 else "wgrad2d_f32"
    elif nd == 3:
        row = "wgrad3d_rr16" if cin == 16 else ("wgrad_roll3d" if sp[0] >= 8 and n * windows >= 8 else "wgrad3d_bf16")
    else:
        row = "wgrad_roll2d" if n >= 8 and windows >= 8 and cin * cout > 1024 else "wgrad2d_bf16"
    return row, cdiv(cout, 32) * cdiv(cin, 32), G.bricks(row, n, sp)


def line(test, case, dtype, launch, row, cols, nb, cus):
    g = min(G.grid(row, cus, cols), nb)
    if row == "roll" and g & 7 and g > 8:
        g &= ~7                                         # roll_plan rounds after the cap at the item count
    return f"{test:34s} {str(case):44s} {dtype:4s} {launch:8s} {row:18s} cols={cols:2d} bricks={nb:4d} blocks/col={g:4d} rounds={cdiv(nb, g)}"


def audit(cus):
    from tests import test_gpu_ops as T
    out = []
    for case in T.MFMA_CASES:
        nd, n, cin, cout, sp = case
        for dt in T.DTYPES:
            out.append(line("test_conv_mfma_fwd_dgrad", case, dt, "fwd", *conv_launch(cus, nd, dt, cin, cout, n, sp), cus))
            out.append(line("test_conv_mfma_fwd_dgrad", case, dt, "dgrad", *conv_launch(cus, nd, dt, cout, cin, n, sp), cus))
            out.append(line("test_conv_mfma_fwd_dgrad", case, dt, "wgrad", *wgrad_launch(nd, dt, cin, cout, n, sp), cus))
    # the one op test that walks the brick kernels: its 2.6 GB sample has 1250 bricks (bf16, identity transform, no statistics, one column)
    big = (3, 1, 16, 16, (8, 400, 400))
    out.append(line("test_conv_mfma_sample_beyond_2gb", big, "bf16", "fwd", *conv_launch(cus, 3, "bf16", 16, 16, 1, big[4]), cus))
    out.append(line("test_conv_mfma_sample_beyond_2gb", big, "bf16", "dgrad", *conv_launch(cus, 3, "bf16", 16, 16, 1, big[4]), cus))
    out.append(line("test_conv_mfma_sample_beyond_2gb", big, "bf16", "wgrad", *wgrad_launch(3, "bf16", 16, 16, 1, big[4]), cus))
    for case in T.ROLL_CASES:
        n, cin, cout, sp = case
        out.append(line("test_conv_roll_fwd_stats_...", case, "bf16", "fwd", *conv_launch(cus, 3, "bf16", cin, cout, n, sp), cus))
        out.append(line("test_conv_roll_fwd_stats_...", case, "bf16", "dgrad", *conv_launch(cus, 3, "bf16", cout, cin, n, sp), cus))
    for case in T.CAT_CASES:
        nd, n, c0, c1, cout, sp = case
        for dt in T.DTYPES:
            out.append(line("test_conv_cat_forms_...", case, dt, "fwd", *conv_launch(cus, nd, dt, c0 + c1, cout, n, sp, single=False), cus))
            out.append(line("test_conv_cat_forms_...", case, dt, "dgrad", *conv_launch(cus, nd, dt, cout, c0 + c1, n, sp, single=False), cus))
            out.append(line("test_conv_cat_forms_...", case, dt, "wgrad", *wgrad_launch(nd, dt, c0 + c1, cout, n, sp), cus))
    for case in T.UPCONV_CASES:
        n, cin, cout, sp = case
        for dt in T.DTYPES:
            out.append(line("test_upconv_fwd_...", case, dt, "fwd", "upconv_fwd", G.columns("upconv_fwd", cin, cout), G.bricks("upconv_fwd", n, sp), cus))
            out.append(line("test_upconv_fwd_...", case, dt, "dgrad", "upconv_dgrad", G.columns("upconv_dgrad", cout, cin), G.bricks("upconv_dgrad", n, sp), cus))
    for case in T.FOLDT_CASES:
        n, cl, cup, cs, cout, sp = case
        # the folded half walks the coarse tensor in 4 x 8 x 16 bricks; at most the 8-column grid of the up-sampling form
        out.append(line("test_foldt_fwd_...", case, "both", "fwd", "upconv_fwd", G.columns("upconv_fwd", cl, cout), G.bricks("upconv_fwd", n, sp), cus))
    for case in T.CONVT_MFMA_CASES:
        nd, n, cin, cout, sp = case
        for dt in T.DTYPES:
            if dt == "bf16" and cin % 32 == 0 and cout % 32 == 0 and cin <= 64 and cout <= 64:
                out.append(f"{'test_convtranspose_mfma':34s} {str(case):44s} bf16 fwd+dgr  k_convt_all: grid capped at a quarter of its tiles -- every block walks >= 4 tiles")
                continue
            rf, rd = ("convt3d_fwd", "convt3d_dgrad") if nd == 3 else ("convt2d_fwd", "convt2d_dgrad")
            out.append(line("test_convtranspose_mfma", case, dt, "fwd", rf, G.columns(rf, cin, cout), G.bricks(rf, n, sp), cus))
            out.append(line("test_convtranspose_mfma", case, dt, "dgrad", rd, G.columns(rd, cout, cin), G.bricks(rd, n, sp), cus))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cus", type=int, default=0)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    cus = a.cus
    if not cus:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# persistent-launch rounds per block, {cus} CUs")
    print("#\n# 1. existing cases of tests/test_gpu_ops.py that reach an MFMA kernel (the *_bnred and *_weight_bn cases use these shapes or smaller)\n#")
    rows = audit(cus)
    for r in rows:
        print(r)
    walked = sum("rounds=1" not in r.split("blocks/col")[-1] for r in rows if "blocks/col" in r)
    print(f"#\n# launches with more than one round: {walked} of {sum('blocks/col' in r for r in rows)}")
    print("#\n# 2. cases of tests/test_gpu_walk.py (bricks, blocks/col and rounds: counted with the table's brick, not measured -- bound= says what the precondition was asserted from;\n#    worst = largest deviation from the float64 reference as a fraction of the tolerance)\n#")
    if a.log:
        seen = set()
        for ln in open(a.log, errors="replace"):
            if ln.startswith("WALK ") and ln not in seen:
                seen.add(ln)
                print(ln.rstrip()[5:])
    else:
        print("# (no --log given)")


if __name__ == "__main__":
    main()
