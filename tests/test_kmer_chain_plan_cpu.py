"""CPU: the resident form of the k-mer chain call (bsa_kmer_chain_plan_create / bsa_kmer_chain_run) without a GPU -- its symbols and signatures,
bsa_kmer_chain_words_bound against NumPy, the argument errors that need no device, and the Python surface."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import support as S

SYMBOLS = ("bsa_kmer_chain_plan_create", "bsa_kmer_chain_plan_destroy", "bsa_kmer_chain_plan_chunks", "bsa_kmer_chain_words_bound", "bsa_kmer_chain_run")


def _proto(ret, name):
    text = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^;{}]*)\)\s*;" % (ret, name), text)
    assert m, "%s %s(...) is not declared in include/bsalign_hip.h" % (ret, name)
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_symbols_and_signatures():
    import bsalign_amd as B
    lib = C.CDLL(B.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert _proto("int", "bsa_kmer_chain_plan_create") == [
        "bsa_ctx_t *ctx", "const uint64_t *qoff", "const uint32_t *qlen", "const uint64_t *toff", "const uint32_t *tlen", "size_t n",
        "uint32_t ksz", "uint32_t flags", "bsa_kmer_chain_plan_t **out"]
    assert _proto("void", "bsa_kmer_chain_plan_destroy") == ["bsa_kmer_chain_plan_t *plan"]
    assert _proto("uint32_t", "bsa_kmer_chain_plan_chunks") == ["const bsa_kmer_chain_plan_t *plan"]
    assert _proto("uint64_t", "bsa_kmer_chain_words_bound") == ["const uint32_t *qlen", "const uint32_t *tlen", "size_t n"]
    assert _proto("int", "bsa_kmer_chain_run") == [
        "bsa_kmer_chain_plan_t *plan", "const uint8_t *d_seqs", "uint64_t *d_maps", "size_t maps_cap", "uint64_t *d_maps_off", "uint32_t *d_status"]
    text = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()
    assert "typedef struct bsa_kmer_chain_plan bsa_kmer_chain_plan_t;" in text
    # the sentence the header used to end the host-pointer calls with now points at the resident form
    assert not re.search(r"Neither takes device pointers\.\s*\n", text)


def test_words_bound_is_the_sum_of_the_shorter_lengths():
    import bsalign_amd as B
    fn = B.lib().bsa_kmer_chain_words_bound
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 1000):
        qlen = rng.integers(0, 5000, n).astype(np.uint32)
        tlen = rng.integers(0, 5000, n).astype(np.uint32)
        if n >= 7:
            qlen[2], tlen[3], qlen[5], tlen[5] = 0, 0, 0, 0
        want = int(np.minimum(qlen, tlen).astype(np.uint64).sum())
        assert fn(B._p(qlen), B._p(tlen), n) == want
        assert B.kmer_chain_words_bound(qlen, tlen) == want
    assert fn(None, None, 0) == 0 and B.kmer_chain_words_bound([], []) == 0
    # 64 bits: more than 2^32 words
    big = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
    assert fn(B._p(big), B._p(big), 3) == 3 * 0xFFFFFFFF
    assert B.kmer_chain_words_bound([10, 0, 3], [4, 9, 3]) == 7


def test_argument_errors_that_need_no_device():
    import bsalign_amd as B
    seqs, qoff, qlen, toff, tlen = B.pack_pairs([(np.zeros(20, np.uint8), np.zeros(20, np.uint8))])
    create = B.lib().bsa_kmer_chain_plan_create
    h = C.c_void_p(0x1234)
    assert create(None, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), 1, 13, 0, C.byref(h)) == -2           # no context
    fake = C.c_void_p(0x1000)                                                                              # never dereferenced: `out` is tested first
    assert create(fake, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), 1, 13, 0, None) == -2                # no `out`
    assert create(None, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), 1, 13, 0, None) == -2
    # no plan: the run, the chunk count and the destructor take NULL
    off = np.zeros(2, dtype=np.uint64)
    assert B.lib().bsa_kmer_chain_run(None, None, None, 0, B._p(off), None) == -2
    assert B.lib().bsa_kmer_chain_plan_chunks(None) == 0
    B.lib().bsa_kmer_chain_plan_destroy(None)


def test_python_surface():
    import bsalign_amd as B
    assert inspect.isclass(B.KmerChainPlan) and callable(B.kmer_chain_words_bound)
    par = inspect.signature(B.KmerChainPlan.__init__).parameters
    assert list(par)[:6] == ["self", "ctx", "qoff", "qlen", "toff", "tlen"] and par["ksz"].default == 13 and par["flags"].default == 0
    run = inspect.signature(B.KmerChainPlan.run).parameters
    assert list(run) == ["self", "d_seqs", "d_maps", "d_maps_off", "d_status"] and run["d_status"].default is None
    assert hasattr(B.KmerChainPlan, "chunks") and hasattr(B.KmerChainPlan, "close")
