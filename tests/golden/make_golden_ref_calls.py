"""Generate tests/golden/ref_calls_*.npz: the real reference's answers (oracle/_ref/libbsref.so, built from the reference sources by
oracle/Makefile) to the calls the randomized reference-parity tests make, so that those tests run without the reference build.
Run where the reference build exists:  python tests/golden/make_golden_ref_calls.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
os.environ["BSA_RECORD_REF"] = "1"

import support as S  # noqa: E402
import test_diagdp_cpu  # noqa: E402
import test_kmer_cpu  # noqa: E402
import test_oracle  # noqa: E402


def main():
    assert S.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    test_oracle.test_align8_oracle_vs_reference_random()
    test_oracle.test_edit_oracle_vs_reference_random()
    test_kmer_cpu.test_host_pieces_against_the_live_reference()
    for k in range(len(test_diagdp_cpu.CASES)):
        test_diagdp_cpu.test_oracle_equals_the_reference_functions(k)
    for rc in S._RECORDING:
        rc.save()
        print("%s: %d calls, %d bytes" % (os.path.relpath(rc.path, os.path.dirname(os.path.dirname(HERE))), len(rc.keys), os.path.getsize(rc.path)))


if __name__ == "__main__":
    main()
