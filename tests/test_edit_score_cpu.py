"""CPU: the edit aligner's score-only form (BSA_MODE_SCORE_ONLY on bsa_edit_*) is in the library, the header documents it for both aligners,
and Python has the entry point that uses it."""
import os

import support as S

ROOT = S.ROOT


def test_library_carries_the_edit_score_only_kernels():
    import bsalign_amd as B
    blob = open(B.LIB_PATH, "rb").read()
    assert b"k_edit_score_finish" in blob
    assert b"k_edit_fwd_grp32 score-only" in blob
    assert callable(getattr(B.Context, "edit_scores", None))


def test_header_covers_both_aligners():
    text = open(os.path.join(ROOT, "include", "bsalign_hip.h")).read()
    start = text.index("#define BSA_MODE_SCORE_ONLY")
    doc = text[start:text.index("*/", start)]
    assert "bsa_align_batch" in doc and "bsa_edit_batch" in doc
