"""CPU: the staged codes themselves.  bsa_seq16 (bsalign_amd/csrc/bsa_seq.h) is the one reader behind the four staging kernels and the window pass's
gather; bsa_seq16_internal is its host side.  Both blob forms and every strand form against a model of a few numpy lines (revcomp, slice, pad), at every
offset residue 0 .. 63, the lengths around one, two, three and four pieces, every piece up to the first that is pure padding, pad codes 0 and 4.

Every blob ends with the sequence's last byte or last word, as a caller's may, and lies against an unreadable page: a load behind the blob (or, for the
reverse strand, in front of one that begins with the sequence's word) does not come back."""
import ctypes as C
import mmap

import numpy as np
import pytest

import bsalign_amd as B

OFFSETS = range(64)
LENGTHS = list(range(41)) + [47, 48, 49, 63, 64, 65]
PADCODES = (0, 4)
REVS = (0, 1, 2)          # forwards, the reverse complement, forwards through the BSA_MODE_QSTRAND instantiation
PAGE = mmap.PAGESIZE


class Guarded:
    """one writable page between two unreadable ones"""

    def __init__(self):
        self.mm = mmap.mmap(-1, 3 * PAGE)
        self.base = C.addressof(C.c_char.from_buffer(self.mm))
        self.libc = C.CDLL(None, use_errno=True)
        self.libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
        self._protect(0)          # PROT_NONE

    def _protect(self, prot):
        for page in (0, 2):
            if self.libc.mprotect(self.base + page * PAGE, PAGE, prot) != 0:
                raise OSError(C.get_errno(), "mprotect")

    def place(self, data, at_end=True):
        """the bytes of `data` against the page behind (or, not at_end, the page in front) -> their address"""
        raw = data.tobytes()
        assert len(raw) <= PAGE
        pos = 2 * PAGE - len(raw) if at_end else PAGE
        self.mm[pos:pos + len(raw)] = raw
        return self.base + pos

    def close(self):
        self._protect(mmap.PROT_READ | mmap.PROT_WRITE)
        self.mm = None          # (the exported pointer keeps the mapping until the object goes)


@pytest.fixture(scope="module")
def guarded():
    g = Guarded()
    yield g
    g.close()


def _read(addr, off, length, i, packed, rev, padcode):
    out, bad = (C.c_uint8 * 16)(), C.c_uint32(7)
    assert B.lib().bsa_seq16_internal(C.c_void_p(addr), off, length, i, int(packed), rev, padcode, out, C.byref(bad)) == 0
    assert bad.value in (0, 1)
    return bytes(out), bad.value


def _model(seq, i, rev, padcode):
    """seq: the stored codes (any byte values).  -> the 16 staged codes of piece i of the strand, and whether a code above 3 lies in the piece"""
    strand = B.revcomp(seq & 3) if rev == 1 else seq & 3          # the staged code: c & 3, or (c & 3) ^ 3 = 3 - (c & 3) on the reverse strand
    raw = seq[::-1] if rev == 1 else seq
    piece = np.full(16, padcode, dtype=np.uint8)
    part = strand[i:i + 16]
    piece[:part.size] = part
    return piece.tobytes(), int((raw[i:i + 16] > 3).any())


def _pieces(length):
    """every multiple of 16 from 0 through the first piece that is pure padding"""
    return range(0, (length + 15) // 16 * 16 + 1, 16)


def test_pieces_end_with_the_first_pure_padding():
    assert list(_pieces(0)) == [0] and list(_pieces(1)) == [0, 16] and list(_pieces(16)) == [0, 16] and list(_pieces(17)) == [0, 16, 32]


@pytest.mark.parametrize("rev", REVS)
def test_byte_blob(guarded, rev):
    """1 B/base: codes above 3 are planted in the sequence (one base in ten) and fill the bytes in front of it.  `bad` is set exactly when such a code
    lies in [i, i + 16) and [0, len) of the strand being read; the staged code is c & 3, or (c & 3) ^ 3 on the reverse strand"""
    rng = np.random.default_rng(100 + rev)
    seen_bad = seen_clean = 0
    for off in OFFSETS:
        for length in LENGTHS:
            seq = rng.integers(0, 4, size=length).astype(np.uint8)
            plant = rng.random(length) < 0.1
            seq[plant] |= (rng.integers(1, 64, size=int(plant.sum())) << 2).astype(np.uint8)
            blob = np.concatenate([np.full(off, 0xFF, dtype=np.uint8), seq])          # ends with the sequence's last byte
            places = (True, False) if rev == 1 and off == 0 else (True,)
            for at_end in places:
                addr = guarded.place(blob, at_end)
                for i in _pieces(length):
                    for padcode in PADCODES:
                        want = _model(seq, i, rev, padcode)
                        assert _read(addr, off, length, i, False, rev, padcode) == want, (off, length, i, padcode, at_end)
                        seen_bad += want[1]
                        seen_clean += 1 - want[1]
    assert seen_bad > 1000 and seen_clean > 1000


@pytest.mark.parametrize("rev", REVS)
def test_packed_blob(guarded, rev):
    """BSA_MODE_SEQ2BIT words and base offsets: `bad` is never set.  The words end with the one that holds the sequence's last base; for the reverse
    strand the blob is also laid against the page in front, where offsets below 32 make its first word the one that holds the sequence's first base"""
    rng = np.random.default_rng(200 + rev)
    for off in OFFSETS:
        for length in LENGTHS:
            words = B.pack2bit(rng.integers(0, 4, size=off + length).astype(np.uint8))          # ends with the word of base off + length - 1
            seq = B.unpack2bit(words, off, length)
            places = (True, False) if rev == 1 and off < 32 else (True,)
            for at_end in places:
                addr = guarded.place(words, at_end)
                for i in _pieces(length):
                    for padcode in PADCODES:
                        want = (_model(seq, i, rev, padcode)[0], 0)
                        assert _read(addr, off, length, i, True, rev, padcode) == want, (off, length, i, padcode, at_end)


def test_python_wrapper_and_bad_arguments():
    seq = np.array([0, 1, 2, 3, 7, 0, 1], dtype=np.uint8)
    out, bad = B.seq16(seq, 2, 5, 0, rev=1, padcode=4)
    assert out.tolist() == [2, 3, 0, 0, 1] + [4] * 11 and bad is True
    out, bad = B.seq16(B.pack2bit(seq), 2, 5, 0, packed=True, rev=1, padcode=4)
    assert out.tolist() == [2, 3, 0, 0, 1] + [4] * 11 and bad is False
    out, bad = B.seq16(seq, 0, 4, 16)
    assert out.tolist() == [0] * 16 and bad is False
    with pytest.raises(ValueError):
        B.seq16(seq, 0, 4, 0, rev=3)
