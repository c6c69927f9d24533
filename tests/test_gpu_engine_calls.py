"""The launch sequence of the engine, pinned: every library call a case's passes issue, in issue order, equals the recorded list line for
line (``tests/golden/engine_calls/<case>.txt``, one ``api<TAB>label`` per call).  A rewrite of the engine's dispatch that makes a node take
another, equally correct kernel -- the plain weight gradient where the rank-one one ran, no side stream -- passes every value test; it does
not pass this one.  Each case also names the calls it exists for, so a shape that stops reaching a path fails instead of pinning nothing."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_calls")
SCRUB = ("BIU_DISABLE", "BIU_FP32_PRODUCTS", "BIU_ROLL", "BIU_FOLDT", "BIU_SIDE_WGRAD_VOX")      # (BIU_FP32_PRODUCTS: every variable that starts so)

# case -> (environment, calls that must appear as api or (api, label suffix), calls that must not appear)
CASES = {
    # BIU_FOLDT=always: the fold's size rule is made for benchmark extents; this takes it wherever the kernels serve the level, as
    # tests/conftest.py does for the suite, so that the case does not depend on where that rule draws its line
    "unet3d_bf16": ({"BIU_FOLDT": "always"},
                    ["biu_foldt_fwd", "biu_foldt_bwd_data", ("biu_foldt_bwd_weight_bn_phase", "/chain"), ("biu_conv_bwd_weight", "/wgrad")], []),
    # BIU_ROLL=always: the rank-one weight gradient exists in the rolling-window form only, which is taken by size too
    # (tests/test_gpu_narrow_end.py runs its step of this shape under the same three switches)
    "unet3d_bf16_rank1": ({"BIU_FOLDT": "always", "BIU_ROLL": "always", "BIU_SIDE_WGRAD_VOX": "0"},
                          ["biu_conv_bwd_weight_bn_rank1"], ["biu_head_dlogits"]),
    "mo3d_interp_bf16": ({}, ["biu_upconv_fwd", "biu_upconv_bwd_data", "biu_upconv_bwd_weight_bn"], []),
    "unet2d_f32": ({}, ["biu_conv_fwd_cat", "biu_conv_bwd_data_bnred", "biu_conv_fwd", "biu_bn_eval_affine", "biu_bn_bwd_finalize_eval"], []),
    "nested_ds": ({}, ["biu_xform_apply", "biu_act_add"], []),
    "siam_concat": ({}, ["biu_maxpool_bwd_bnred"], []),
}


def _record(case, tmp_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith(SCRUB)}
    env.update(CASES[case][0])
    out = str(tmp_path / f"{case}.json")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "engine_calls_probe.py"), case, out], check=True, env=env, timeout=300)
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_engine_issues_the_recorded_calls(case, tmp_path):
    r = _record(case, tmp_path)
    got = [f"{api}\t{label}" for api, label in r["calls"]]
    _, must, must_not = CASES[case]
    for want in must:
        api, suffix = (want, "") if isinstance(want, str) else want
        assert any(a == api and lab.endswith(suffix) for a, lab in r["calls"]), f"{case} no longer reaches {want}"
    for api in must_not:
        assert all(a != api for a, _ in r["calls"]), f"{case}: {api} ran"
    if case == "nested_ds":
        # deep supervision: several heads, and the heads of one trunk go through ONE (stacked) backward
        nbwd = sum(a.startswith("biu_head_bwd") and not a.endswith("_workspace") for a, _ in r["calls"])
        assert r["heads"] > 1 and nbwd == r["trunks"], (r["heads"], r["trunks"], nbwd)
    with open(os.path.join(GOLDEN, f"{case}.txt")) as f:
        want = f.read().splitlines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{case}: call {i} is {a!r}, recorded {b!r}"
    assert len(got) == len(want), f"{case}: {len(got)} calls, recorded {len(want)}"
