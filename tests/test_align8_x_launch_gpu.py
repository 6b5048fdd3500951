"""The launches of the exact-arithmetic forward kernels that the dispatch fixture does not reach, against their recorded behaviour
(tests/golden/align8_x_launch.json, written by tests/golden/make_golden_align_dispatch.py --list x-launch from the library of the commit the file names):
for every case of align8_x_launch_cases.X_CASES the return code, the two kernel names, the hand-over count, cigar_off[n] and a SHA-256 over records,
status words, cigar_off and CIGAR words are the recorded ones.  The expected values never come from the library under test."""
import pytest

import align8_x_launch_cases as XL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    fx = XL.load_fixture()
    assert set(fx["cases"]) == {c["id"] for c in XL.X_CASES}, "the fixture and the case list differ: record it again from the commit it names (%s)" % fx["commit"]
    return fx["cases"]


@pytest.mark.parametrize("case", XL.X_CASES, ids=[c["id"] for c in XL.X_CASES])
def test_x_launch_is_the_recorded_one(ctx, recorded, case):
    got = XL.run_case(ctx, case)
    exp = recorded[case["id"]]
    print(case["id"], got)
    assert got == exp, "\n".join("%s: %r, recorded %r" % (k, got.get(k), exp.get(k)) for k in sorted(set(got) | set(exp)) if got.get(k) != exp.get(k))
