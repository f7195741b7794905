"""The planning decisions of the built library against a recording (tests/golden/plans.json) made
by scripts/dump_plans.py from a build of the commit before plan.hpp / exec.hpp were split out of
mpfft.hip: plan, workspace size and layout, stage kernels and inverse-column schedule of every
case, their squaring counterparts, the mul6 plans and the error codes.  No device is touched.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("dump_plans", os.path.join(ROOT, "scripts", "dump_plans.py"))
dump_plans = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_plans)

with open(os.path.join(ROOT, "tests", "golden", "plans.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def built(mp):
    return dump_plans.dump(mp.LIB_PATH)


def test_recording_covers_the_cases(built):
    assert len(GOLDEN) == len(dump_plans.CASES) + len(dump_plans.CASES6) + len(dump_plans.ERRORS)
    assert sorted(built) == sorted(GOLDEN)
    for name, want in GOLDEN.items():   # every non-error case was a valid plan when recorded
        if not name.startswith("error"):
            assert want.get("check_params", want.get("check_params6")) == 0, name


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_plan_matches_recording(built, name):
    want, got = GOLDEN[name], built[name]
    assert sorted(got) == sorted(want)
    for entry in sorted(want):
        w, g = want[entry], got[entry]
        if not isinstance(w, dict):
            assert g == w, (name, entry)
            continue
        assert g["rc"] == w["rc"], (name, entry)
        if w["out"] is None:
            assert g["out"] is None, (name, entry)
        elif isinstance(w["out"], str):   # ';'-joined fields or one launch per line
            sep = "\n" if "\n" in w["out"] else ";"
            ws, gs = w["out"].split(sep), g["out"].split(sep)
            assert len(gs) == len(ws), (name, entry)
            for i, (a, b) in enumerate(zip(gs, ws)):
                assert a == b, (name, entry, i)
        else:
            assert len(g["out"]) == len(w["out"]), (name, entry)
            for i, (a, b) in enumerate(zip(g["out"], w["out"])):
                assert a == b, (name, entry, i)
