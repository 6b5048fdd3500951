"""Generate tests/golden/edit_launch.json: what the library of ONE named commit does with every case of tests/edit_launch_cases.py -- the return code, the
kernel names and a SHA-256 over everything the call leaves.  The file is the reference of tests/test_edit_launch_gpu.py for a change that must not alter
behaviour, so it is recorded from the commit BEFORE such a change, never from the code under test: build that commit's library, point BSA_LIB_PATH at it,
and say which commit it is.  Every case must return 0, or nothing is written.

Run on the MI355X:  BSA_LIB_PATH=/path/to/that/libbsalign_hip.so python tests/golden/make_golden_edit_launch.py --commit <sha> [--out FILE]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import edit_launch_cases as EL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library is loaded (written into the file)")
    ap.add_argument("--out", default=EL.FIXTURE)
    a = ap.parse_args()
    if len(a.commit) < 7 or any(ch not in "0123456789abcdef" for ch in a.commit):
        ap.error("--commit takes the hash of the commit being recorded")
    import bsalign_amd as B
    ctx = B.Context(0)
    cases = {}
    for case in EL.CASES:
        cases[case["id"]] = EL.run_case(ctx, case)
        print(case["id"], json.dumps(cases[case["id"]]), flush=True)
        assert cases[case["id"]]["rc"] == 0, case["id"]
    ctx.close()
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "library": os.path.basename(B.LIB_PATH), "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (a.out, len(cases), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
