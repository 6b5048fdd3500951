"""Generate tests/golden/ref_calls_*.npz: the real reference's answers (oracle/_ref/libbsref.so, built from the reference sources by
oracle/Makefile) to the calls the randomized reference-parity tests make, so that those tests run without the reference build.
Run where the reference build exists:  python tests/golden/make_golden_ref_calls.py [NAME ...]
With names (e.g. ref_calls_align8_mtx) only those fixtures are recorded and written; the others stay as they are."""
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


def producers():
    """fixture name -> the test that makes its calls"""
    out = {
        "ref_calls_align8": test_oracle.test_align8_oracle_vs_reference_random,
        "ref_calls_edit": test_oracle.test_edit_oracle_vs_reference_random,
        "ref_calls_align8_mtx": test_oracle.test_align8_oracle_vs_reference_custom_matrices,
        "ref_calls_kmer": test_kmer_cpu.test_host_pieces_against_the_live_reference,
    }
    for k in range(len(test_diagdp_cpu.CASES)):
        out["ref_calls_diagdp_%d" % k] = (lambda k=k: test_diagdp_cpu.test_oracle_equals_the_reference_functions(k))
    return out


def main(names=None):
    assert S.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    prods = producers()
    names = list(names) if names else list(prods)
    unknown = [n for n in names if n not in prods]
    assert not unknown, "unknown fixtures %s (known: %s)" % (unknown, sorted(prods))
    for name in names:
        prods[name]()
    for rc in S._RECORDING:
        if rc.name not in names:
            continue
        rc.save()
        print("%s: %d calls, %d bytes" % (os.path.relpath(rc.path, os.path.dirname(os.path.dirname(HERE))), len(rc.keys), os.path.getsize(rc.path)))


if __name__ == "__main__":
    main(sys.argv[1:])
