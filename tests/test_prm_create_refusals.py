"""CPU: oxhip_prm_create answers every recorded config as the library that wrote tests/golden/prm_create_refusals.json did (the
file names its commit): the same status code and the same oxhip_last_error_string, character for character.  The records cover
every refusal oxhip_prm_create makes before it chooses a device, configs that break two rules at once (the order of the checks)
and configs that pass validation.  Those last ones end with OXHIP_ERR_NO_DEVICE where there is no GPU; where there is one they
are created, which is what passing validation means there."""
import ctypes as C
import json
import os
import sys

import pytest

from oxmpl_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_create_refusals as gen  # noqa: E402

with open(os.path.join(HERE, "golden", "prm_create_refusals.json")) as _f:
    GOLDEN = json.load(_f)
RECORDS = GOLDEN["records"]


@pytest.fixture(scope="module")
def L():
    capi.build_library()
    return capi.lib()


def test_the_file_covers_the_refusals_and_names_its_commit():
    assert len(GOLDEN["_library_commit"]) == 40
    names = [r["name"] for r in RECORDS]
    assert len(set(names)) == len(names) and names == ["null_cfg", "null_out"] + [n for n, _ in gen.CASES]
    assert sum(n.startswith("order_") for n in names) >= 8 and sum(n.startswith("ok_") for n in names) >= 6
    # every text oxhip_prm_create can answer with before select_device (the file's _unreachable names the one it cannot)
    assert len({r["message"] for r in RECORDS}) >= 17 and len(GOLDEN["_unreachable"]) == 1
    for r in RECORDS:   # the records are the generator's cases, field for field
        assert set(r["fields"]) == {f for f, _ in capi.PrmConfig._fields_}
        assert (r["code"] == capi.ERR_NO_DEVICE) == r["name"].startswith("ok_"), r["name"]
    for (name, overrides), r in zip(gen.CASES, RECORDS[2:]):
        assert gen.fields_of(overrides) == r["fields"], name
    ok = {r["name"]: r["fields"] for r in RECORDS if r["name"].startswith("ok_")}
    so3 = [f for f in ok.values() if f["space"] == capi.SPACE_SO3]
    rn = [f for f in ok.values() if f["space"] == capi.SPACE_REAL_VECTOR]
    assert any(f["knn_k"] for f in rn) and any(not f["knn_k"] for f in rn) and so3
    assert any(f["connection_radius"] == "inf" for f in rn) and any(float.fromhex(f["connection_radius"]) <= 0.0 for f in rn)
    assert any(f["bounds"][4] == "nan" for f in so3)


@pytest.mark.parametrize("rec", RECORDS, ids=[r["name"] for r in RECORDS])
def test_prm_create_answers_as_recorded(L, rec):
    n = C.c_int32()
    has_gpu = L.oxhip_device_count(C.byref(n)) == capi.OK
    st, msg = gen.create(L, rec["fields"], rec["null"])
    if rec["name"].startswith("ok_") and has_gpu:
        assert st == capi.OK, (rec["name"], st, msg)
    else:
        assert (st, msg) == (rec["code"], rec["message"]), rec["name"]
