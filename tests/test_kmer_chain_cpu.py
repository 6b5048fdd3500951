"""CPU: the device k-mer chainer's interface without a GPU -- the new symbols and their signatures, the flag check of
bsa_kmer_edit_batch2, the NumPy statement of the packed-arena contract (kmer_chain_cases.host_arena, reused by the GPU test) against
per-pair bsa_kmer_chain calls, and that the inputs of test_kmer_chain_gpu.py exercise what they are there for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kmer_chain_cases as KC
import kmer_support as K
import support as S


def _proto(name):
    text = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{}]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/bsalign_hip.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_new_symbols_and_signatures():
    import bsalign_amd as B
    lib = C.CDLL(B.LIB_PATH)
    for name in ("bsa_kmer_chain_batch", "bsa_kmer_edit_batch2", "bsa_ctx_last_kmer_chain_ms"):
        assert hasattr(lib, name), name
    assert _proto("bsa_kmer_chain_batch") == [
        "bsa_ctx_t *ctx", "const uint8_t *seqs", "size_t seqs_bytes", "const uint64_t *qoff", "const uint32_t *qlen",
        "const uint64_t *toff", "const uint32_t *tlen", "size_t n", "uint32_t ksz", "uint64_t *maps", "size_t maps_cap",
        "uint64_t *maps_off", "uint32_t *status"]
    old = _proto("bsa_kmer_edit_batch")
    assert _proto("bsa_kmer_edit_batch2") == old + ["uint32_t flags"]
    assert _proto("bsa_ctx_last_kmer_chain_ms") == ["bsa_ctx_t *ctx", "double *ms", "long *pairs_on_device", "long *pairs_on_host"]
    text = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()
    assert re.search(r"#define\s+BSA_KMER_CHAIN_DEVICE\s+1u", text)
    assert B.KMER_CHAIN_DEVICE == 1
    assert hasattr(B.Context, "kmer_chain_batch") and hasattr(B.Context, "last_kmer_chain_ms")
    import inspect
    assert inspect.signature(B.Context.kmer_edit_batch).parameters["device_chain"].default is False


def test_unknown_flag_bit_is_an_argument_error_without_a_gpu():
    import bsalign_amd as B
    seqs, qoff, qlen, toff, tlen = B.pack_pairs([(np.zeros(20, np.uint8), np.zeros(20, np.uint8))])
    par = B.KmerParams()
    par.ksz, par.threads = 13, 1
    out = np.zeros(1, dtype=B.RESULT_DTYPE)
    fn = B.lib().bsa_kmer_edit_batch2
    for flags in (2, 3, 0x80000000):
        assert fn(None, B._p(seqs), seqs.size, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), 1, C.byref(par), B._p(out), None, 0, None, None, flags) == -2
    # no context: an argument error as well, with or without the flag (never a crash)
    for flags in (0, 1):
        assert fn(None, B._p(seqs), seqs.size, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), 1, C.byref(par), B._p(out), None, 0, None, None, flags) == -2
    off = np.zeros(2, dtype=np.uint64)
    assert B.lib().bsa_kmer_chain_batch(None, B._p(seqs), seqs.size, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), 1, 13, None, 0, B._p(off), None) == -2


def test_arena_contract_against_per_pair_chains():
    rng = np.random.default_rng(5)
    T = rng.integers(0, 4, 1500).astype(np.uint8)
    bad = S.mutate(rng, T, 0.05)
    bad[40] = 9
    pairs = [(S.mutate(rng, T, 0.05), T), (np.zeros(0, np.uint8), T), (T.copy(), T), (bad, T), (S.mutate(rng, T, 0.4), T), (T[:7].copy(), T)]
    rc, maps, off, st = KC.host_arena(pairs, 11)
    assert rc == 0 and off[0] == 0 and len(off) == len(pairs) + 1 and int(off[-1]) == len(maps)
    for k, (q, t) in enumerate(pairs):
        mine = maps[int(off[k]):int(off[k + 1])]
        if st[k]:
            assert len(mine) == 0
        else:
            assert np.array_equal(mine, K.kmer_chain(11, q, t)), k
    assert list(st) == [0, KC.ST_EMPTY, 0, KC.ST_BAD_BASE, 0, 0]
    assert len(maps[int(off[0]):int(off[1])]) > 0 and off[6] == off[5]         # shorter than k: none
    # anchors are in query order, query offset << 32 | target offset
    m0 = maps[int(off[2]):int(off[3])]
    assert np.array_equal(m0 >> np.uint64(32), m0 & np.uint64(0xFFFFFFFF)) and np.all(np.diff((m0 >> np.uint64(32)).astype(np.int64)) > 0)
    # too small an arena: the code and the words needed, nothing else
    need = int(off[-1])
    rc2, maps2, off2, _ = KC.host_arena(pairs, 11, maps_cap=need - 1)
    assert rc2 == KC.E_CIGAR_CAP and int(off2[-1]) == need and len(maps2) == 0
    assert KC.host_arena(pairs, 11, maps_cap=need)[0] == 0
    # k-mer sizes above 15 mean 15, 0 gives nothing
    assert np.array_equal(KC.host_arena(pairs, 20)[1], KC.host_arena(pairs, 15)[1])
    assert int(KC.host_arena(pairs, 0)[2][-1]) == 0
    assert KC.host_arena([], 13)[2].tolist() == [0]


@pytest.mark.parametrize("ksz", [8, 13])
def test_restatement_equals_the_host_chainer(ksz):
    """chain_py is only trusted to count filter passes and bisections because it returns bsa_kmer_chain's words"""
    for name, q, t in KC.cases(ksz, with_long=False):
        if len(q) > 6000 and name not in ("staircase",):
            continue
        got, _ = KC.chain_py(ksz, q, t)
        assert np.array_equal(got, K.kmer_chain(ksz, q, t)), name


def test_inputs_reach_the_filter_twice_and_the_lis_bisection():
    """The staircase pair takes the diagonal filter through more than one dropping pass (so at least three passes), the crossing pair
    sends hits through the LIS bisection, and the low-complexity pairs have k-mer 0 in play.

    The bisection's third branch -- stop on equality -- cannot be reached by any input: every hit is a k-mer that occurs exactly once in
    the target, so two hits never share a target offset, and the value looked up is never one the tail holds.  What is checked instead is
    exactly that premise (dup_toff == 0 and lis_equal == 0 on every input); the device code keeps the branch as the reference writes it."""
    saw_search = 0
    for ksz in (8, 13):
        for name, q, t in KC.cases(ksz, with_long=False):
            if len(q) > 6000 and name != "staircase":
                continue
            maps, info = KC.chain_py(ksz, q, t)
            assert info["dup_toff"] == 0 and info["lis_equal"] == 0, name
            saw_search += info["lis_search"]
            if name == "staircase":
                assert info["filter_iters"] >= 3 and len(maps) > 0, info
                d = (maps >> np.uint64(32)).astype(np.int64) - (maps & np.uint64(0xFFFFFFFF)).astype(np.int64)
                assert np.all(d == 0)                      # both insertions' anchors are gone
            if name == "crossing":
                assert info["lis_search"] > 0, info
    assert saw_search > 0
    # k-mer 0 and the sentinel: two poly-A sequences of exactly k bases share the k-mer 0 once each and still get no anchor
    assert len(K.kmer_chain(13, np.zeros(13, np.uint8), np.zeros(13, np.uint8))) == 0
    assert KC.chain_py(13, np.zeros(13, np.uint8), np.zeros(13, np.uint8))[1]["hits"] == 0
