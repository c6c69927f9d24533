"""Child of tests/test_gpu_walk.py::test_conv_walk_under_split_fp32_products_3d: one walking case of the fp32 3x3x3 convolution under the
product mode its spec names.  The mode latches at the first fp32 3-D call of a process, hence a process of its own; it is set before anything
else and the default is asked for again in a `finally` (refused by the library once latched: the process ends here anyway).

usage: walk_probe.py <spec id> <out.json>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("BIU_FOLDT", "always")          # as tests/conftest.py
os.environ.setdefault("BIU_ROLL", "always")

from tests import walk_geometry as G  # noqa: E402
from tests.gpu_util import lib  # noqa: E402

spec = G.SPEC_BY_ID[sys.argv[1]]
assert lib.biu_set_fp32_products_3d(spec.opts["mode"]) == 0, lib.biu_last_error()
try:
    from tests.test_gpu_walk import check_conv_walk
    rec = check_conv_walk(spec)
    json.dump({"rows_fwd": rec["rows_fwd"], "dev": rec["dev"]}, open(sys.argv[2], "w"))
finally:
    lib.biu_set_fp32_products_3d(0)
