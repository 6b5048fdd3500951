"""trace_choose (bsa_align8_codes.hip), the one function that decides what the traceback launcher of the compact path launches, on a grid of chunks, host only
(bsa_align8_trace_choice_internal).  What is asserted is the launcher's contract, not its code: every combination the launcher had a kernel for gets a launch
with that kernel's name (the table below is written out from the launcher as it stood before trace_choose; tests/test_walk_corpus_gpu.py expects the same
names from a run), code format 1 launches exactly where the plan is told the traceback reads it, the grid covers every pair, the LDS walker's pairs per wave
are what the launcher's loop gave, and everything else is an error."""
import itertools

import pytest

import bsalign_amd as B

KNOBS = ("BSA_ALIGN8_TRACE_WAVE", "BSA_ALIGN8_TRACE_SIMPLE")
ENVS = [{}, {"BSA_ALIGN8_TRACE_WAVE": "0"}, {"BSA_ALIGN8_TRACE_SIMPLE": "1"}, {"BSA_ALIGN8_TRACE_WAVE": "0", "BSA_ALIGN8_TRACE_SIMPLE": "1"}]
CUS = (8, 256)
WAVE, LDS, SIMPLE, CODES2, CODES2_WAVE = ("k_align8_trace_codes_wave", "k_align8_trace_codes_lds", "k_align8_trace_codes_simple", "k_align8_trace_codes2",
                                          "k_align8_trace_codes2_wave")
PAIRS_PER_BLOCK = {WAVE: 1, CODES2_WAVE: 1, SIMPLE: 64, CODES2: 64}          # (the LDS walker: its pairs per wave)
FORM = {WAVE: B.TR_WAVE, LDS: B.TR_LDS, SIMPLE: B.TR_SIMPLE, CODES2: B.TR_CODES2, CODES2_WAVE: B.TR_CODES2_WAVE}


def counts(cus):
    full = 3 * 4 * cus * 4          # the LDS walker doubles its pairs per wave above about three waves a SIMD
    return (1, 63, 64, 65, full - 1, full + 1, 100000)


def expected_name(bw, pw, wave_off, simple):
    """the kernel of (bandwidth, gap model) under the two switches"""
    if pw == 2:          # two-piece gaps: BSA_ALIGN8_TRACE_SIMPLE is not looked at
        return CODES2_WAVE if bw == 128 and not wave_off else CODES2
    if simple:
        return SIMPLE
    if not wave_off:
        return WAVE
    return SIMPLE if bw == 256 else LDS


def reads_do2(bw, pw, wave_off, simple):
    """where the plan lets the forward pass write code format 1: affine gaps at bandwidth 128 under the one-walk-per-wave kernel"""
    return pw == 1 and bw == 128 and not simple and not wave_off


def lds_lanes(count, cus):
    lanes = 4
    while lanes < 32 and count // lanes > cus * 4 * 3:
        lanes *= 2
    return lanes


@pytest.mark.parametrize("env", ENVS, ids=["+".join("%s=%s" % (k[11:], v) for k, v in e.items()) or "defaults" for e in ENVS])
def test_the_choice_keeps_the_launchers_contract(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wave_off, simple = env.get("BSA_ALIGN8_TRACE_WAVE") == "0", env.get("BSA_ALIGN8_TRACE_SIMPLE") == "1"
    seen = set()
    for bw, pw, fmt, cus in itertools.product((64, 128, 256), (0, 1, 2), (0, 1), CUS):
        for count in counts(cus):
            d = B.align8_trace_choice(bw, pw, fmt, count, cus)
            if fmt == 1:
                assert d["launch"] == reads_do2(bw, pw, wave_off, simple), (bw, pw, count, cus)
            else:
                assert d["launch"]
            if not d["launch"]:
                assert d["form"] == B.TR_NONE and d["name"] == ""
                continue
            name = expected_name(bw, pw, wave_off, simple)
            assert d["name"] == name and d["form"] == FORM[name], (bw, pw, fmt, count, cus)
            assert d["W"] * 16 == bw and d["fmt"] == fmt
            if name == LDS:
                assert d["lanes"] in (4, 8, 16, 32) and d["lanes"] == lds_lanes(count, cus) and d["pairs_per_block"] == d["lanes"]
            else:
                assert d["lanes"] == 0 and d["pairs_per_block"] == PAIRS_PER_BLOCK[name]
            assert d["grid"] * d["pairs_per_block"] >= count > (d["grid"] - 1) * d["pairs_per_block"]
            seen.add(name)
    want = {(False, False): {WAVE, CODES2, CODES2_WAVE}, (True, False): {LDS, SIMPLE, CODES2}, (False, True): {SIMPLE, CODES2, CODES2_WAVE},
            (True, True): {SIMPLE, CODES2}}[(wave_off, simple)]
    assert seen == want


def test_widths_without_kernels_and_bad_arguments():
    for bw in (0, 16, 32, 80, 512):
        for pw in (0, 1, 2):
            assert not B.align8_trace_choice(bw, pw, 0, 100)["launch"]
    assert not B.align8_trace_choice(128, 2, 1, 100)["launch"] and not B.align8_trace_choice(128, 1, 2, 100)["launch"]
    for bad in ((128, 1, 0, 0, 256), (128, 3, 0, 10, 256), (128, -1, 0, 10, 256), (128, 1, 0, 10, 0)):
        with pytest.raises(ValueError):
            B.align8_trace_choice(*bad)
