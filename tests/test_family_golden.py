"""What the C ABI layer and the Python bindings decide, against a recording (tests/golden/family_answers.json)
made by scripts/dump_plans.py --families from a build of the commit before the per-family copies in
mpfft.hip and __init__.py were folded: plans, workspace sizes and layouts and kernel names of the mulmodw,
mulmodm1, cached-operand, dot and sdot entries, every chooser's picks, the status codes of the stage and
device entries for null pointers, and the package's public names.  No device is touched.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("dump_plans", os.path.join(ROOT, "scripts", "dump_plans.py"))
dump_plans = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_plans)

with open(os.path.join(ROOT, "tests", "golden", "family_answers.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def built(mp):
    return dump_plans.dump_families(mp.LIB_PATH)


def same(got, want, where):
    """field by field, so a difference names its place"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), where
        for k in sorted(want):
            same(got[k], want[k], where + (k,))
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, where + (i,))
    elif isinstance(want, str) and ";" in want:   # the ';'-joined stage fields
        same(got.split(";"), want.split(";"), where)
    else:
        assert got == want, where


def test_recording_covers_the_cases(built):
    assert sorted(built) == sorted(GOLDEN)
    shapes = len(dump_plans.MULMODW_SHAPES) + len(dump_plans.MULMODM1_SHAPES) + len(dump_plans.CASES) \
        + 2 * len(dump_plans.DOT_CASES)
    assert sum(1 for name in GOLDEN if "depth=" in name) == shapes
    for name, want in GOLDEN.items():   # every shape was a valid plan when recorded
        if "depth=" in name and "check_params" in want:
            assert want["check_params"] == 0, name
    codes = GOLDEN["argument checks"]   # 13 stage numbers, three ways, and no call got past its checks
    for entry, by_flag in codes.items():
        if entry != "device entries":
            assert sorted(by_flag) == ["acc", "driven", "plain"] and all(len(v) == 13 for v in by_flag.values()), entry
            assert all(c in (1, 4) for v in by_flag.values() for c in v), entry   # EINVAL or ENOMEM
    assert all(c in (1, 4) for c in codes["device entries"].values())


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_family_matches_recording(built, name):
    same(built[name], GOLDEN[name], (name,))
