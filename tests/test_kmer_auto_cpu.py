"""CPU: what the GPU tests of BSA_KMER_STRAND_AUTO (test_kmer_auto_gpu.py) rest on -- the constants, the keyword check, and that the cases built for the
flag are what their names say.  Every anchor count here comes from the host chainer (bsa_kmer_chain) alone."""
import os
import re

import numpy as np
import pytest

import bsalign_amd as B
import kmer_auto_cases as A
import kmer_flags_cases as F
import support as S


def _define(hdr, name):
    m = re.search(r"^#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, hdr, re.M)
    assert m, name
    return int(m.group(1), 0)


def test_python_constants_equal_the_header():
    hdr = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()
    assert B.KMER_STRAND_AUTO == _define(hdr, "BSA_KMER_STRAND_AUTO") == A.KMER_STRAND_AUTO == 2
    assert B.ST_REVCOMP == _define(hdr, "BSA_ST_REVCOMP") == A.ST_REVCOMP == 16
    others = [_define(hdr, n) for n in ("BSA_KMER_CHAIN_DEVICE", "BSA_MODE_SEQ2BIT", "BSA_MODE_QSTRAND")]
    assert others == [B.KMER_CHAIN_DEVICE, B.MODE_SEQ2BIT, B.MODE_QSTRAND] and all(B.KMER_STRAND_AUTO & o == 0 for o in others)
    bits = [_define(hdr, n) for n in ("BSA_ST_BAD_BASE", "BSA_ST_EMPTY", "BSA_ST_TRACE", "BSA_ST_DEVICE")]
    assert bits == [1, 2, 4, 8] and B.ST_REVCOMP < (1 << _define(hdr, "BSA_ST_MARGIN_SHIFT"))


def test_auto_strand_with_strands_raises():
    ctx = B.Context.__new__(B.Context)                       # the check comes before anything touches the device
    q = np.zeros(40, np.uint8)
    with pytest.raises(ValueError):
        ctx.kmer_chain_batch([(q, q)], ksz=13, strands=[False], auto_strand=True)
    with pytest.raises(ValueError):
        ctx.kmer_edit_batch([(q, q)], ksz=13, strands=[True], auto_strand=True)


@pytest.mark.parametrize("ksz", [8, 13])
def test_named_cases_are_what_their_names_say(ksz):
    cs = {name: (q, t) for name, q, t in A.extra_cases()}
    assert tuple(cs) == A.EXTRA
    fw, rv = A.both_strands([cs[n] for n in A.EXTRA], ksz)
    by = {n: (len(f), len(r)) for n, f, r in zip(A.EXTRA, fw, rv)}
    q, t = cs["palindrome"]
    assert np.array_equal(F.revcomp(q), q) and np.array_equal(fw[0], rv[0])
    # The palindrome ties at NO anchors: every canonical k-mer of a sequence that is its own reverse complement occurs at least twice in it, so the host
    # chainer finds no unique one (0 against 0 at ksz 8 and 13).  The tie of more than 500 anchors a side is `tie_with_anchors`.
    assert by["palindrome"][0] == by["palindrome"][1] == 0
    assert by["tie_with_anchors"][0] == by["tie_with_anchors"][1] > 500
    assert not np.array_equal(fw[4], rv[4])
    assert min(by["both_fwd_wins"]) >= 20 and by["both_fwd_wins"][0] > by["both_fwd_wins"][1]
    assert min(by["both_rev_wins"]) >= 20 and by["both_rev_wins"][1] > by["both_rev_wins"][0]
    if ksz == 13:                                            # (unrelated sequences of this length share a few 8-mers by chance: a handful of anchors a side)
        assert by["empty_both"] == (0, 0)
    _, _, _, strands = A.expected([cs[n] for n in A.EXTRA], ksz)
    assert list(strands[:3]) == [False, False, True] and not strands[4] and (ksz == 8 or not strands[3])
    names, pairs = A.named_pairs(ksz)
    assert len(names) == len(pairs) == len(set(names)) and set(A.EXTRA) <= set(names) and "identical/rc" in names


@pytest.mark.parametrize("ksz", [8, 13])
def test_random_batch_has_both_strands(ksz):
    pairs, flip = A.random_pairs()
    assert len(pairs) == 300 and int(flip.sum()) == 150
    fw, rv = A.both_strands(pairs, ksz)
    rev_wins = sum(1 for f, r, x in zip(fw, rv, flip) if x and len(r) > len(f))
    fwd_wins = sum(1 for f, r, x in zip(fw, rv, flip) if not x and len(f) > len(r))
    assert 3 * rev_wins >= 150 and 3 * fwd_wins >= 150, (rev_wins, fwd_wins)


def test_edit_batch_has_both_strands():
    pairs, flip = A.random_edit_pairs(31)
    assert len(pairs) == 3008 and int(flip.sum()) == 1504
    _, _, _, strands = A.expected(pairs, 11)
    assert 3 * int((strands & flip).sum()) >= 1504 and not (strands & ~flip).all()
    on = A.on_strand(pairs[:50], strands[:50])
    for (q, t), (sq, _), s in zip(on, pairs[:50], strands[:50]):
        assert np.array_equal(q, F.revcomp(sq) if s else sq)
