"""The 8-bit aligner's dispatch against its recorded behaviour (tests/golden/align_dispatch.json, written by
tests/golden/make_golden_align_dispatch.py from the library of the commit the file names): for every case of align_dispatch_cases.CASES the
return code, the two kernel names, the hand-over count, cigar_off[n] and a SHA-256 over records, status words, cigar_off and CIGAR words are the
recorded ones.  The expected values never come from the library under test."""
import pytest

import align_dispatch_cases as AD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    fx = AD.load_fixture()
    assert set(fx["cases"]) == {c["id"] for c in AD.CASES}, "the fixture and the case list differ: record it again from the commit it names (%s)" % fx["commit"]
    return fx["cases"]


@pytest.mark.parametrize("case", AD.CASES, ids=[c["id"] for c in AD.CASES])
def test_dispatch_is_the_recorded_one(ctx, recorded, case):
    got = AD.run_case(ctx, case)
    exp = recorded[case["id"]]
    print(case["id"], got)
    assert got == exp, "\n".join("%s: %r, recorded %r" % (k, got.get(k), exp.get(k)) for k in sorted(set(got) | set(exp)) if got.get(k) != exp.get(k))
