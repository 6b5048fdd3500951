"""The edit-distance launchers against their recorded behaviour (tests/golden/edit_launch.json, written by tests/golden/make_golden_edit_launch.py from the
library of the commit the file names): for every case of edit_launch_cases.CASES the return code, the two kernel names, cigar_off[n] and a SHA-256 over
records, status words, cigar_off and CIGAR words are the recorded ones.  The expected values never come from the library under test."""
import pytest

import edit_launch_cases as EL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    fx = EL.load_fixture()
    assert set(fx["cases"]) == {c["id"] for c in EL.CASES}, "the fixture and the case list differ: record it again from the commit it names (%s)" % fx["commit"]
    assert all(r["rc"] == 0 for r in fx["cases"].values())
    return fx["cases"]


@pytest.mark.parametrize("case", EL.CASES, ids=[c["id"] for c in EL.CASES])
def test_edit_launch_is_the_recorded_one(ctx, recorded, case):
    got = EL.run_case(ctx, case)
    exp = recorded[case["id"]]
    print(case["id"], got)
    assert got == exp, "\n".join("%s: %r, recorded %r" % (k, got.get(k), exp.get(k)) for k in sorted(set(got) | set(exp)) if got.get(k) != exp.get(k))
