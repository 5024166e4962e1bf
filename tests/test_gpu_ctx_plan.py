"""What a context launches and owns is what it was before the host library was split into units: for every case of
tests/ctx_plan_cases.py the product library gives exactly the vgl_ctx_info() fields that tools/ctx_info_matrix.py recorded in
tests/golden/ctx_plan/parent_info.json -- workspace_bytes included, before and after one synchronous 8-site host tile with every
tag -- and refuses the same cases with the same code and text.  The case list is complete only if every recorded field takes at
least two values across it (size, abi_version and test_hooks cannot differ between two contexts of one library)."""
import json
import os

import pytest

import ctx_plan_cases as cpc
from vcfgl_amd import _abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctx_plan", "parent_info.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_every_recorded_field_takes_two_values(golden):
    assert sorted(golden) == sorted(c["name"] for c in cpc.CASES)
    seen = {}
    for rec in golden.values():
        for key in ("info", "info_after_tile"):
            for f, v in rec.get(key, {}).items():
                seen.setdefault(f, set()).add(v)
    assert set(seen) == {f for f, _ in _abi.CtxInfo._fields_} - {"device"}
    assert [f for f, vals in seen.items() if len(vals) < 2 and f not in cpc.CONSTANT_FIELDS] == []
    codes = {rec["code"] for rec in golden.values() if "code" in rec}
    assert codes == {_abi.VGL_E_ARG, _abi.VGL_E_UNSUPPORTED, _abi.VGL_E_QSBIN, _abi.VGL_E_ADJQ}


def test_the_library_reproduces_the_recorded_plan(golden):
    got = cpc.collect(_abi.load_library())
    assert sorted(got) == sorted(golden)
    for name in sorted(golden):
        assert got[name] == golden[name], name
