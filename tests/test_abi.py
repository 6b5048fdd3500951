"""CPU: the C-ABI library loads, exports every symbol the public headers declare, and fails loudly without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import support as S

ROOT = S.ROOT


def _declared_symbols():
    names = set()
    inc = os.path.join(ROOT, "include")
    for fn in sorted(os.listdir(inc)):
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(inc, fn)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
        # prototypes: identifier followed by '(' at declaration level, terminated by ';'
        for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{}]*\)\s*;", text):
            name = m.group(1)
            if name not in ("sizeof", "int", "void"):          # (int / void: the return type of a function-pointer typedef)
                names.add((fn, name))
    return names


def test_library_exports_every_declared_symbol():
    import bsalign_amd as B
    libs = {"bsalign_hip.h": C.CDLL(B.LIB_PATH), "bsalign_msa.h": C.CDLL(B.LIB_PATH), "bsalign_poa.h": C.CDLL(B.LIB_PATH)}
    compat = os.path.join(ROOT, "bsalign_amd", "libbsalign_compat.so")
    if os.path.exists(compat):
        libs["bsalign_compat.h"] = C.CDLL(compat)
    decl = _declared_symbols()
    assert len(decl) >= 15
    missing = []
    for fn, name in sorted(decl):
        lib = libs.get(fn)
        if lib is None:
            continue
        if not hasattr(lib, name):
            missing.append("%s:%s" % (fn, name))
    assert not missing, "declared but not exported: %s" % missing


def test_result_struct_layout_matches_reference():
    import bsalign_amd as B
    assert B.RESULT_DTYPE.itemsize == 40          # seqalign_result_t = 10 x int32 (bsalign.h:213-218)
    assert B.RESULT_DTYPE.names == ("score", "qb", "qe", "tb", "te", "mat", "mis", "ins", "del", "aln")
    assert C.sizeof(B.AlignParams) == 28


def test_score_matrix_helper():
    import bsalign_amd as B
    p = B.make_params(0, 128, 2, -6)
    assert [p.matrix[i] for i in range(16)] == [2 if (i >> 2) == (i & 3) else -6 for i in range(16)]


def test_matrix_argument_arrives_in_order():
    """make_params(matrix=...) hands the 16 bytes over as given -- matrix[qbase * 4 + tbase], not transposed, not projected"""
    import bsalign_amd as B
    import matrix_support as MS
    m = MS.GENERAL["asym"]
    p = B.make_params(0, 128, 0, 0, -3, -2, matrix=m)
    got = np.array([p.matrix[i] for i in range(16)], dtype=np.int8)
    assert np.array_equal(got, m) and not np.array_equal(got, MS.transposed(m))
    assert bytes(p)[8:24] == m.tobytes()            # (mode, bandwidth, then the matrix: bsa_align_params_t)


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import bsalign_amd as B
    with pytest.raises(B.BsaError) as ei:
        B.Context(0)
    assert ei.value.code == -1


def test_synthetic_generator_host_equals_numpy():
    import bsalign_amd as B
    for L in (1, 31, 32, 33, 1000):
        ps = B.synth_pairs_host(4, L, first_pair=5)
        for k, (q, t) in enumerate(ps):
            q2, t2 = S.synth_pair(5 + k, L)
            assert np.array_equal(q, q2) and np.array_equal(t, t2)
    q, t = S.synth_pair(0, 10000)
    assert 9600 < len(q) < 10100          # eps 0.10 with ins:del 31:46 shrinks the query by ~1.5 %


def test_product_does_not_touch_the_oracle():
    """the shipped path must not import / link anything under oracle/"""
    pkg = os.path.join(ROOT, "bsalign_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".c", ".cpp")) or fn == "Makefile":
                text = open(os.path.join(dp, fn), errors="ignore").read()
                assert "liboracle" not in text and "orc_" not in text and "bsalign_oracle" not in text, fn
