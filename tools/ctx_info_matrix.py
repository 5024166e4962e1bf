#!/usr/bin/env python3
"""Creates a context on the product library for every case of tests/ctx_plan_cases.py and prints, as JSON, every field of
vgl_ctx_info() except `device` -- for the cases marked `tile` again after one synchronous 8-site host tile with every tag
requested -- or the code and text of a refusal.  tests/golden/ctx_plan/parent_info.json is this tool's output on the commit named
in the README beside it; tests/test_gpu_ctx_plan.py holds every later build to it.

    python tools/ctx_info_matrix.py > tests/golden/ctx_plan/parent_info.json      (needs a GPU)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ctx_plan_cases  # noqa: E402
from vcfgl_amd import _abi  # noqa: E402

if __name__ == "__main__":
    json.dump(ctx_plan_cases.collect(_abi.load_library()), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
