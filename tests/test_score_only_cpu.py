"""CPU: the score-only flag (BSA_MODE_SCORE_ONLY) is the same number in the header and in Python, apart from every other mode bit,
and the library carries its kernels and the Python entry point that uses it."""
import os
import re

import support as S

ROOT = S.ROOT


def _header_defines():
    text = open(os.path.join(ROOT, "include", "bsalign_hip.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(BSA_MODE_[A-Z_]+)\s+(0x[0-9A-Fa-f]+|\d+)", text)}


def test_flag_values_match_the_header():
    import bsalign_amd as B
    d = _header_defines()
    assert d["BSA_MODE_SCORE_ONLY"] == B.MODE_SCORE_ONLY == 0x400
    assert d["BSA_MODE_ROWRECORDS"] == B.MODE_ROWRECORDS
    # a flag bit of its own: not a mode value, not another flag
    assert B.MODE_SCORE_ONLY & 3 == 0 and B.MODE_SCORE_ONLY & B.MODE_ROWRECORDS == 0
    assert all(v & B.MODE_SCORE_ONLY == 0 for k, v in d.items() if k != "BSA_MODE_SCORE_ONLY")


def test_library_carries_the_score_only_kernels():
    import bsalign_amd as B
    blob = open(B.LIB_PATH, "rb").read()
    assert b"k_align8_score_finish" in blob
    assert b"k_score_only_trim" in blob
    assert callable(getattr(B.Context, "align_scores", None))
