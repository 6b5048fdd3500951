"""Generate tests/golden/align_dispatch.json: what the library of ONE named commit does with every case of tests/align_dispatch_cases.py -- the
return code, the kernel names, the hand-over count and a SHA-256 over everything the call leaves.  The file is the reference of
tests/test_align_dispatch_gpu.py for a change that must not alter behaviour, so it is recorded from the commit BEFORE such a change, never from
the code under test: build that commit's library, point BSA_LIB_PATH at it, and say which commit it is.

Run on the MI355X:  BSA_LIB_PATH=/path/to/that/libbsalign_hip.so python tests/golden/make_golden_align_dispatch.py --commit <sha>

--list x-launch records tests/golden/align8_x_launch.json from tests/align8_x_launch_cases.py instead (the reference of tests/test_align8_x_launch_gpu.py).  Every
case of that list must return 0 and leave no pair flagged BSA_ST_DEVICE -- a row-segment wait that gave up would make the digest depend on timing -- or nothing
is written."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import align_dispatch_cases as AD  # noqa: E402
import align8_x_launch_cases as XL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library is loaded (written into the file)")
    ap.add_argument("--list", default="dispatch", choices=["dispatch", "x-launch"], help="which list of cases, and with it which fixture")
    a = ap.parse_args()
    if len(a.commit) < 7 or any(ch not in "0123456789abcdef" for ch in a.commit):
        ap.error("--commit takes the hash of the commit being recorded")
    import bsalign_amd as B
    strict = a.list == "x-launch"
    todo, fixture = (XL.X_CASES, XL.FIXTURE) if strict else (AD.CASES, AD.FIXTURE)
    if strict:
        digest = AD._digest

        def checked(out, st, off, cig, cap):          # (run_case keeps the status words' hash alone)
            assert not (st & B.ST_DEVICE).any(), "a pair was given up by the device"
            return digest(out, st, off, cig, cap)
        AD._digest = checked
    ctx = B.Context(0)
    cases = {}
    for case in todo:
        cases[case["id"]] = AD.run_case(ctx, case)
        print(case["id"], json.dumps(cases[case["id"]]), flush=True)
        assert not strict or cases[case["id"]]["rc"] == 0, case["id"]
    ctx.close()
    with open(fixture, "w") as f:
        json.dump({"commit": a.commit, "library": os.path.basename(B.LIB_PATH), "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    handed = sum(1 for r in cases.values() if r.get("handover"))
    print("wrote %s: %d cases (%d with a hand-over), %d bytes" % (fixture, len(cases), handed, os.path.getsize(fixture)))


if __name__ == "__main__":
    main()
