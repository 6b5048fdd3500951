"""CPU: the packed-sequence flag (BSA_MODE_SEQ2BIT) is the same number in the header and in Python, the library exports the device
packer, and the Python packers write the reference's BaseBank layout (dna.h bits2bit: base i at bits 62 - 2 (i % 32) of word i / 32)."""
import os
import re

import numpy as np
import pytest

import support as S

ROOT = S.ROOT


def _header_defines():
    text = open(os.path.join(ROOT, "include", "bsalign_hip.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(BSA_MODE_[A-Z0-9_]+)\s+(0x[0-9A-Fa-f]+|\d+)", text)}


def _bits2bit(words, i):
    """a literal restatement of the reference's bits2bit macro, one base at a time"""
    return (int(words[i >> 5]) >> (((~i) & 0x1F) << 1)) & 0x03


def _bit2bits(words, i, c):
    """... and of bit2bits, which writes one"""
    sh = ((~i) & 0x1F) << 1
    words[i >> 5] = (int(words[i >> 5]) & ~(0x3 << sh) & 0xFFFFFFFFFFFFFFFF) | (c << sh)


def test_flag_value_matches_the_header():
    import bsalign_amd as B
    d = _header_defines()
    assert d["BSA_MODE_SEQ2BIT"] == B.MODE_SEQ2BIT == 0x800
    assert B.MODE_SEQ2BIT & 3 == 0
    assert all(v & B.MODE_SEQ2BIT == 0 for k, v in d.items() if k != "BSA_MODE_SEQ2BIT")


def test_library_exports_the_device_packer():
    import bsalign_amd as B
    L = B.lib()
    assert hasattr(L, "bsa_seq_pack2bit")
    blob = open(B.LIB_PATH, "rb").read()
    assert b"k_stage2b" in blob and b"k_edit_stage2b" in blob and b"k_pack2bit" in blob
    for name in ("seq_pack2bit",):
        assert callable(getattr(B.Context, name, None))


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 64, 1000])
def test_pack2bit_is_the_reference_layout(n):
    import bsalign_amd as B
    rng = np.random.default_rng(n + 7)
    codes = rng.integers(0, 4, size=n).astype(np.uint8)
    w = B.pack2bit(codes)
    assert w.dtype == np.uint64 and w.size == (n + 31) // 32
    ref = [0] * ((n + 31) // 32)
    for i, c in enumerate(codes):
        _bit2bits(ref, i, int(c))
    assert [int(x) for x in w] == ref
    assert [_bits2bit(w, i) for i in range(n)] == [int(c) for c in codes]
    # codes above 3 go in as c & 3, the bits behind the last base are zero
    wide = B.pack2bit(codes | (rng.integers(0, 64, size=n).astype(np.uint8) << 2))
    assert np.array_equal(wide, w)
    if n % 32:
        assert int(w[-1]) & ((1 << (64 - 2 * (n % 32))) - 1) == 0


def test_pack2bit_worked_example_of_the_header():
    import bsalign_amd as B
    w = B.pack2bit(np.array(([0, 1, 2, 3] * 9)[:35], dtype=np.uint8))
    assert [int(x) for x in w] == [0x1B1B1B1B1B1B1B1B, 0x1800000000000000]


def test_unpack2bit_round_trips_at_every_offset():
    import bsalign_amd as B
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 4, size=200).astype(np.uint8)
    w = B.pack2bit(codes)
    for off in range(64):
        for n in (0, 1, 17, 32, 33, 200 - off):
            assert np.array_equal(B.unpack2bit(w, off, n), codes[off:off + n]), (off, n)


def test_pack_pairs_packed_uses_base_offsets():
    import bsalign_amd as B
    rng = np.random.default_rng(11)
    pairs = [(rng.integers(0, 4, size=int(rng.integers(1, 300))).astype(np.uint8),
              rng.integers(0, 4, size=int(rng.integers(1, 300))).astype(np.uint8)) for _ in range(40)]
    w, qoff, qlen, toff, tlen = B.pack_pairs(pairs, seq2bit=True)
    assert w.dtype == np.uint64 and w.nbytes % 8 == 0
    assert (qoff + qlen <= 4 * w.nbytes).all() and (toff + tlen <= 4 * w.nbytes).all()
    # base offsets, not word offsets, and not all on a word
    assert len({int(x) % 32 for x in np.concatenate([qoff, toff])}) > 8
    for k, (q, t) in enumerate(pairs):
        assert np.array_equal(B.unpack2bit(w, qoff[k], qlen[k]), q) and np.array_equal(B.unpack2bit(w, toff[k], tlen[k]), t)
    # the last pair ends in the last word
    assert (int(toff[-1]) + int(tlen[-1]) - 1) // 32 == w.size - 1
    # the byte form is what it was
    seqs, bq, bql, bt, btl = B.pack_pairs(pairs)
    assert seqs.dtype == np.uint8 and np.array_equal(bql, qlen) and np.array_equal(btl, tlen)
    assert np.array_equal(seqs[int(bq[0]):int(bq[0]) + int(bql[0])], pairs[0][0])
