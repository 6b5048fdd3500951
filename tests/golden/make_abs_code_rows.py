"""Records tests/golden/abs_code_rows.npz: the code rows that the absolute-score forward DP stores for the batch of tests/abs_code_rows_support.py, one run per
code layout.  Run on the GPU with the library whose rows are to be the reference (the build before a change of the kernel's flag arithmetic; BSA_LIB_PATH
selects a library):

    BSA_LIB_PATH=<reference libbsalign_hip.so> python tests/golden/make_abs_code_rows.py [output.npz]

The file holds the pairs themselves, so the test does not depend on a random generator's stream."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import abs_code_rows_support as A
import bsalign_amd as B


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else A.GOLDEN
    pairs = A.make_pairs()
    ctx = B.Context(0)
    data = {
        "q": np.concatenate([q for q, t in pairs]), "t": np.concatenate([t for q, t in pairs]),
        "qlen": np.array([len(q) for q, t in pairs], np.uint32), "tlen": np.array([len(t) for q, t in pairs], np.uint32),
    }
    for layout, (bw, sc, env) in A.LAYOUTS.items():
        for k in A.ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(A.ENV)
        os.environ.update(env)
        name, status, rows = A.code_rows(ctx, pairs, layout)
        assert "absolute scores" in name and ("two-bit" in name) == (layout == "two-bit"), name
        data["rows_" + layout] = np.concatenate([r.reshape(-1) for r in rows])
        data["status_" + layout] = status
        print(layout, name, data["rows_" + layout].nbytes, "bytes; status words", sorted(set(status.tolist())), "pairs flagged", int((status != 0).sum()))
    ctx.close()
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
