"""Regenerates tests/golden/snv.npz from the real reference: `oracle/_ref/bsalign_ref_cli poa -v` (built by __graft_entry__.build() where the
reference sources are present) on synthetic read sets, its stdout recorded and parsed.  Data only: the reads, the recorded text and the arrays
parsed from it.

    python tests/golden/make_golden_snv.py

The printed MSA is the tidied one call_snvs_bspoa saw: its letters map one to one to the codes 0-6 ("ACGT-.*", case-insensitive), the [CNS] row
is byte nall of a column, [QLT] and [ALT] (minus '!') the other two.  Row [000] is the command line's empty placeholder read, so a replay uses
skip_first_row = 1.  Per set k the fixture holds
    reads_k / read_off_k   the reads' codes one behind the other, and their offsets
    stdout_k               the recorded text (uint8)
    cols_k                 the parsed columns, (mlen, nall + 3)
    snp_k                  the SNP lines as printed (uint8)
    snv_k                  the records parsed from them: mpos, cpos, qual, covn, refn, altn, refb, altb (int64 rows)
    meta_k                 nall, nseq, mlen, the recorded MSA_SNV_ERR_PROB x 10000
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLI = os.path.join(ROOT, "oracle", "_ref", "bsalign_ref_cli")
LETTERS = {c: i for i, c in enumerate("ACGT-.*")}

# (reads, length, error rate, reads carrying the alternative allele: None = every second read)
SETS = [(40, 300, 0.04, None), (70, 500, 0.08, None), (24, 300, 0.02, None), (20, 400, 0.0, None), (20, 400, 0.0, 2), (48, 300, 0.03, None)]


def make_reads(rng, nreads, length, err, nalt):
    truth = rng.integers(0, 4, length)
    other = truth.copy()
    sites = list(range(40, length - 40, 60))                      # planted substitutions, 60 apart
    for p in sites:
        other[p] = (other[p] + 1 + rng.integers(0, 3)) % 4
    reads = []
    for r in range(nreads):
        src = other if (r % 2 == 1 if nalt is None else r < nalt) else truth
        out = []
        for b in src:
            u = rng.random()
            if u < err * 0.5:
                out.append((b + 1 + rng.integers(0, 3)) % 4)         # substitution
            elif u < err * 0.75:
                continue                                          # deletion
            elif u < err:
                out.extend((b, rng.integers(0, 4)))                # insertion behind the base
            else:
                out.append(b)
        reads.append(np.array(out, dtype=np.uint8))
    return reads


def parse(text):
    """the recorded stdout -> (cols, nall, snp lines, records, recorded rate x 10000)"""
    rows, snp, prob = {}, [], None
    for line in text.split("\n"):
        m = re.match(r"BSALIGN MSA \[(\d+|CNS|QLT|ALT)\] (\S+)", line)
        if m:
            rows.setdefault(m.group(1), []).append(m.group(2))
        elif line.startswith("BSALIGN SNP\t"):
            snp.append(line + "\n")
        elif line.startswith("[MSA_SNV_ERR_PROB:"):
            prob = int(round(float(line[len("[MSA_SNV_ERR_PROB:"):line.index("]")]) * 10000))
    ids = sorted(k for k in rows if k.isdigit())
    nall = len(ids)
    full = {k: "".join(v) for k, v in rows.items()}
    mlen = len(full["CNS"])
    cols = np.zeros((mlen, nall + 3), dtype=np.uint8)
    for r, k in enumerate(ids):
        assert int(k) == r and len(full[k]) == mlen
        cols[:, r] = [LETTERS[c.upper()] for c in full[k]]
    cols[:, nall] = [LETTERS[c.upper()] for c in full["CNS"]]
    cols[:, nall + 1] = [ord(c) - 33 for c in full["QLT"]]
    cols[:, nall + 2] = [ord(c) - 33 for c in full["ALT"]]
    recs = []
    for line in snp:
        f = line.rstrip("\n").split("\t")
        # label SNP, cpos, mpos, flank, flank quality, ref base, refn, alt base, altn, flank, flank quality, covn, qual, genotypes
        recs.append((int(f[2]), int(f[1]), int(f[12]), int(f[11]), int(f[6]), int(f[8]), "ACGT".index(f[5]), "ACGT".index(f[7])))
    return cols, nall, "".join(snp), np.array(recs, dtype=np.int64).reshape(-1, 8), prob


def main():
    if not os.path.exists(CLI):
        sys.exit("oracle/_ref/bsalign_ref_cli is missing: run __graft_entry__.build() where the reference sources are present")
    rng = np.random.default_rng(20261021)
    out = {"nsets": np.array(len(SETS))}
    for k, (nreads, length, err, nalt) in enumerate(SETS):
        reads = make_reads(rng, nreads, length, err, nalt)
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "reads.fa")
            with open(fa, "w") as f:
                for r, s in enumerate(reads):
                    f.write(">r%d\n%s\n" % (r, "".join("ACGT"[c] for c in s)))
            text = subprocess.run([CLI, "poa", "-v", fa], check=True, capture_output=True).stdout.decode()
        cols, nall, snp, recs, prob = parse(text)
        out["reads_%d" % k] = np.concatenate(reads)
        out["read_off_%d" % k] = np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64)
        out["stdout_%d" % k] = np.frombuffer(text.encode(), dtype=np.uint8)
        out["cols_%d" % k] = cols
        out["snp_%d" % k] = np.frombuffer(snp.encode(), dtype=np.uint8)
        out["snv_%d" % k] = recs
        out["meta_%d" % k] = np.array([nall, nall, cols.shape[0], prob], dtype=np.int64)
        print("set %d: %d reads of %d at %.2f -> nall %d mlen %d rate %.4f, %d SNP lines, qual %s" % (k, nreads, length, err, nall, cols.shape[0], prob / 10000.0, len(recs),
                                                                                                      sorted(set(recs[:, 2].tolist()))))
    np.savez_compressed(os.path.join(HERE, "snv.npz"), **out)


if __name__ == "__main__":
    main()
