"""BSA_MODE_CIGAR_EQX: the seeded corpora and parameter sets of test_cigar_eqx_cpu.py and test_cigar_eqx_gpu.py, so that what the CPU
file vets against the oracle's own mat / mis counts (and its share of pairs the reference cannot trace) is exactly what the GPU file sends."""
import functools

import numpy as np

import support as S

G, O, E = S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND
ROWRECORDS = 0x100

SC = {
    "affine": (2, -6, -3, -2, 0, 0),
    "linear": (2, -6, 0, -3, 0, 0),
    "twopiece": (2, -6, -3, -2, -8, -1),
    "big": (10, -30, -20, -10, 0, 0),           # outside the exact-arithmetic guard (test_align8_gpu.py BIG_SCORINGS)
    # gap costs the checked whole-query kernel flags pairs for (test_align8_gpu.py::test_checked_systolic_kernel_flags_...): pairs are handed over
    "clamp0": (40, -40, -20, -25, 0, 0),
    "clamp1": (20, -40, -25, -15, 0, 0),
    "clamp2": (5, -60, -3, -60, 0, 0),
    "clamp3": (37, -59, -13, -1, 0, 0),
}


def _mk_pairs(rng, n, lens, eps_list=(0.01, 0.1, 0.2), ratios=(1.0, 1.0, 0.9, 1.1)):
    """the generator of test_align8_gpu.py"""
    pairs = []
    for _ in range(n):
        L = int(rng.choice(lens))
        T = rng.integers(0, 4, size=L).astype(np.uint8)
        Q = S.mutate(rng, T, float(rng.choice(eps_list)))
        r = float(rng.choice(ratios))
        if r != 1.0:
            Lq = max(1, int(len(Q) * r))
            Q = Q[:Lq] if Lq <= len(Q) else np.concatenate([Q, rng.integers(0, 4, size=Lq - len(Q)).astype(np.uint8)])
        if len(Q) == 0:
            Q = np.array([0], dtype=np.uint8)
        pairs.append((Q, T))
    return pairs


def _sub(t, cols):
    q = t.copy()
    for c in cols:
        q[c] = (q[c] + 1) & 3
    return q


LONG_L = 10000


@functools.lru_cache(maxsize=None)
def corpus(name):
    rng = np.random.default_rng({"mixed": 11, "mid": 12, "longq": 13, "clamp": 9200, "edit": 14, "editwide": 15, "editgen": 16, "long": 17, "gt1024": 18}.get(name, 1))
    if name == "mixed":
        return _mk_pairs(rng, 48, [1, 15, 16, 17, 63, 64, 65, 100, 300, 1000, 2000])
    if name == "mid":
        return _mk_pairs(rng, 32, [10, 100, 700, 1500])
    if name == "gt48":         # every query longer than the bandwidth 48: no whole-query band, the run-time-width kernel
        return [(q, t) for q, t in corpus("mid") if len(q) > 48]
    if name == "gt1024":       # ... than 1024
        return [(q, t) for q, t in _mk_pairs(rng, 14, [1200, 1500, 2000], ratios=(1.0, 1.1)) if len(q) > 1024]
    if name == "longq":        # queries above 256 bases: bandwidth 0 takes the systolic kernel
        return [(q, t) for q, t in _mk_pairs(rng, 30, [300, 500, 700, 1000, 2000], eps_list=(0.0, 0.05, 0.2)) if len(q) > 256]
    if name == "clamp":        # the pairs of test_checked_systolic_kernel_flags_what_the_int8_arithmetic_clamps
        return [(q, t) for q, t in _mk_pairs(rng, 40, [300, 500, 700, 1000], eps_list=(0.02, 0.1, 0.3), ratios=(1.0, 0.9, 1.1)) if len(q) > 256]
    if name == "edit":         # one launch class at bandwidth 256 in global mode (test_edit_gpu.py::test_rows_tiled_eight_at_a_time)
        pairs = _mk_pairs(rng, 40, [300, 700, 1500, 3000], eps_list=(0.0, 0.01, 0.1, 0.2), ratios=(1.0, 1.0, 0.97, 1.03))
        return [(q, t) for q, t in pairs if len(q) > 256 and (len(q) + len(t) - 1) // len(t) + 1 <= 256]
    if name == "editwide":     # queries above 1024 bases: bandwidth 0 is the wave-per-pair kernel
        return [(q, t) for q, t in _mk_pairs(rng, 12, [1100, 1500, 2500], eps_list=(0.02, 0.1, 0.2), ratios=(1.0, 0.8, 1.2)) if len(q) > 1024]
    if name == "editgen":      # queries above the bandwidth 1088: a moving wide band, the generic kernel
        return [(q, t) for q, t in _mk_pairs(rng, 8, [2500, 4000], eps_list=(0.02, 0.1), ratios=(1.0,)) if len(q) > 1088]
    if name == "long":
        # one M word of 10 000 columns (the whole-wave path of the pass, 512 columns a trip): identical pairs, one substitution at column 0, at the
        # last column, at every multiple of 512 - 1 / + 0 / + 1, and all of those at once
        t = rng.integers(0, 4, size=LONG_L).astype(np.uint8)
        pairs = [(t.copy(), t), (_sub(t, [0]), t), (_sub(t, [LONG_L - 1]), t), (_sub(t, [0, LONG_L - 1]), t)]
        edges = []
        for m in range(512, LONG_L, 512):
            for c in (m - 1, m, m + 1):
                pairs.append((_sub(t, [c]), t))
                edges.append(c)
        pairs.append((_sub(t, edges), t))
        pairs.append((_sub(t, range(0, LONG_L, 2)), t))          # alternating columns: 10 000 words out of one
        pairs.append((_sub(t, range(LONG_L)), t))                # all mismatches (the band stays on the diagonal: a gap costs more than it saves only with cheap X)
        return pairs
    if name == "words":        # plain CIGARs of more than 64 and of more than 4096 words (tile and trip boundaries)
        return [S.synth_pair(3, 10000), S.synth_pair(4, 40000), S.synth_pair(5, 700)]
    raise KeyError(name)


# (id, corpus, mode, bandwidth, scoring, mode flags, environment, substring of the forward kernel's name or None, of the traceback kernel's or None)
ALIGN_CASES = [
    ("bw128-global", "mixed", G, 128, "affine", 0, {}, "two-bit", "k_align8_trace_codes_wave"),
    ("bw128-overlap", "mixed", O, 128, "affine", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw128-extend", "mixed", E, 128, "affine", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw128-planes", "mixed", G, 128, "affine", 0, {"BSA_ALIGN8_DO2": "0"}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw128-lds", "mixed", G, 128, "affine", 0, {"BSA_ALIGN8_TRACE_WAVE": "0"}, "k_align8_fwd_x", "k_align8_trace_codes_lds"),
    ("bw128-simple", "mixed", G, 128, "affine", 0, {"BSA_ALIGN8_TRACE_SIMPLE": "1"}, "k_align8_fwd_x", "k_align8_trace_codes_simple"),
    ("bw64-global", "mixed", G, 64, "affine", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw64-extend", "mixed", E, 64, "affine", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw256-global", "mixed", G, 256, "affine", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw256-overlap", "mixed", O, 256, "affine", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw128-linear", "mixed", G, 128, "linear", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw64-linear", "mixed", O, 64, "linear", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("bw128-twopiece", "mixed", G, 128, "twopiece", 0, {}, "k_align8_fwd_x2", "k_align8_trace_codes2_wave"),
    ("bw128-twopiece-extend", "mixed", E, 128, "twopiece", 0, {}, "k_align8_fwd_x2", "k_align8_trace_codes2_wave"),
    ("bw64-twopiece", "mixed", G, 64, "twopiece", 0, {}, "k_align8_fwd_x2", "k_align8_trace_codes2"),
    ("bw64-twopiece-overlap", "mixed", O, 64, "twopiece", 0, {}, "k_align8_fwd_x2", "k_align8_trace_codes2"),
    # off the compact path
    ("rowrecords", "mixed", G, 128, "affine", ROWRECORDS, {}, "row records", "k_align8_backcal"),
    ("rowrecords-overlap", "mid", O, 128, "affine", ROWRECORDS, {}, "row records", "k_align8_backcal"),
    ("bw32", "mid", G, 32, "affine", 0, {}, "row records", "k_align8_backcal"),
    ("bw512", "mid", O, 512, "affine", 0, {}, "row records", "k_align8_backcal"),
    ("bw48", "gt48", E, 48, "affine", 0, {}, "k_align8_fwd_gen", "k_align8_backcal"),
    ("bw1024", "gt1024", G, 1024, "affine", 0, {}, "k_align8_fwd_gen", "k_align8_backcal"),
    ("sys-global", "longq", G, 0, "affine", 0, {}, "k_align8_fwd_sys", "k_align8_trace_sys"),
    ("sys-overlap", "longq", O, 0, "affine", 0, {}, "k_align8_fwd_sys", "k_align8_trace_sys"),
    ("sys-extend", "longq", E, 0, "twopiece", 0, {}, "k_align8_fwd_sys", "k_align8_trace_sys"),
    ("sys-checked", "longq", G, 0, "big", 0, {}, "k_align8_fwd_sys<CHK>", "k_align8_trace_sys"),
    ("width-classes", "mixed", O, 0, "affine", 0, {}, None, None),          # bsa_align_batch: one sub-batch per width class of the whole-query bands
    ("debug-handover", "mixed", G, 128, "affine", 0, {"BSA_DEBUG_HANDOVER": "3"}, None, None),
    # long words and long CIGARs
    ("long-words", "long", G, 128, "affine", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
    ("many-words", "words", G, 128, "affine", 0, {}, "k_align8_fwd_x", "k_align8_trace_codes_wave"),
]
# scorings outside the guard whose flagged pairs bsa_align_batch hands over to the literal kernels: the sum of the hand-overs must not be zero
HANDOVER_CASES = [("handover-%s-%d" % (sc, mode), "clamp", mode, 0, sc, 0, {}, "k_align8_fwd_sys<CHK>", None)
                  for sc in ("clamp0", "clamp1", "clamp2", "clamp3") for mode in (G, O, E)
                  # (global and extend mode of these two: the reference's traceback does not terminate on 7.5 % and 20 % of the pairs)
                  if mode == O or sc in ("clamp0", "clamp2")]

# (id, corpus, mode, bandwidth, environment, substring of the forward kernel's name or None, of the traceback kernel's, a substring it must not have)
EDIT_CASES = [
    ("tiled", "edit", G, 256, {}, "tiled", "k_edit_trace_wave (rows tiled", None),
    ("format0", "edit", G, 256, {"BSA_EDIT_TILED": "0"}, "k_edit_fwd", "k_edit_trace_wave", "tiled"),
    ("per-lane", "edit", G, 256, {"BSA_EDIT_TRACE_WAVE": "0"}, "k_edit_fwd", "k_edit_trace", "k_edit_trace_wave"),
    ("bw256-overlap", "mid", O, 256, {}, None, "k_edit_trace", None),
    ("bw256-extend", "mid", E, 256, {}, None, "k_edit_trace", None),
    ("bw64-global", "mid", G, 64, {}, None, "k_edit_trace", None),
    ("bw0-global", "mid", G, 0, {}, None, "k_edit_trace", None),
    ("wide-extend", "editwide", E, 0, {}, "k_edit_fwd_wide", "k_edit_trace", None),
    ("wide-overlap", "editwide", O, 0, {}, "k_edit_fwd_wide", "k_edit_trace", None),
    ("generic", "editgen", G, 1088, {}, "k_edit_fwd_gen", "k_edit_trace", None),
    ("long-words", "long", G, 256, {}, None, "k_edit_trace", None),
    ("many-words", "words", G, 256, {}, None, "k_edit_trace", None),
]

MAX_UNTRACEABLE = 0.05       # share of a parameter set's pairs on which the reference's traceback does not terminate (compared by status only)


@functools.lru_cache(maxsize=None)
def align_oracle(cname, mode, bw, scname):
    """[(record, CIGAR words, word count or ORC_ERR_TRACE)] of a corpus under one parameter set"""
    return [S.oracle_align(q, t, mode, bw, *SC[scname]) for q, t in corpus(cname)]


@functools.lru_cache(maxsize=None)
def edit_oracle(cname, mode, bw):
    return [S.oracle_edit(q, t, mode, bw) for q, t in corpus(cname)]


def well_formed(words):
    """no word of length 0, no two neighbouring words with the same op, only M-free ops"""
    w = np.asarray(words, dtype=np.uint32)
    ops = w & np.uint32(15)
    return bool((w >> np.uint32(4) != 0).all() and (ops[1:] != ops[:-1]).all() and np.isin(ops, (1, 2, 7, 8)).all())
