"""CPU: the SNV caller behind the window chain without a GPU -- the loop closed on the host, as test_window_msa_cpu.py closes it for the consensus: a
truth, a second haplotype with planted substitutions, a draft with small edits, ten error-free reads of each haplotype through the Python statements
of the chain, the host consensus caller and bsa_msa_call_snvs.  The called sites, as window * w + lpos, are exactly the planted ones."""
import numpy as np
import pytest

import snv_cases as SC
import window_msa_cases as W


@pytest.mark.parametrize("w", [100, 50])
def test_planted_sites_of_a_diploid_sample_are_the_calls(w):
    SC.need_symbols()
    import bsalign_amd.msa as MSA
    truth, hap2, draft, ws, sites, reads, rec, rng = SC.diploid_loop(11, w)
    assert len(sites) >= 8 and all(b - a >= 30 for a, b in zip(sites, sites[1:])) and all(20 <= s % w <= w - 21 for s in sites)
    assert not np.array_equal(truth[:len(draft)], draft[:len(truth)]) and int((truth != hap2).sum()) == len(sites)
    b, status = W.through_the_references(rng, len(reads), w, False, reads=reads, recs=[rec] * len(reads), cigs=[ws] * len(reads), draft=draft)
    assert np.all(status == 0)
    off, cwin, cols = W.window_msa_ref(b, 0)
    called, cns_all = [], []
    for g in range(b.nwin):
        r = cwin[g]
        nall, nseq, mlen = int(r["nall"]), int(r["nseq"]), int(r["mlen"])
        assert nall == 21 and nseq == 20
        mine = cols[int(off[g]):int(off[g + 1])].copy()
        cns_all.append(MSA.call_consensus(mine, None, nall, nseq, int(r["nmax"]), mlen, W.PAR7)[0])
        snv, pexp, nsites = MSA.call_snvs(mine, nall, nseq, SC.params())
        ref = SC.snv_ref(mine, nall, nseq, SC.params())
        assert snv.tobytes() == ref[0].tobytes() and np.float32(pexp) == ref[1] == np.float32(0.01) and nsites == ref[2]
        for v in snv:
            assert int(v["refn"]) == 10 and int(v["altn"]) == 10 and int(v["covn"]) == 20 and int(v["qual"]) == 14
            called.append(g * w + int(v["lpos"]))
            d = g * w + int(v["lpos"])
            assert {int(v["refb"]), int(v["altb"])} == {int(truth[[i for i in range(len(truth)) if truth[i] != hap2[i]][sites.index(d)]]),
                                                       int(hap2[[i for i in range(len(truth)) if truth[i] != hap2[i]][sites.index(d)]])}
    assert called == sites
    got = np.concatenate(cns_all)
    assert len(got) == len(truth) and np.all((got == truth) | (got == hap2))
