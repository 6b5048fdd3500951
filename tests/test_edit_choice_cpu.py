"""edit_choose (bsa_edit.hip), the one function that decides what the edit-distance launchers launch for a launch class, on a grid of classes, host only
(bsa_edit_choice_internal).  What is asserted is the launcher's contract with its kernels, not its code: every pair of the class has a lane in every launch, a
kernel is only asked for at a template argument it is built for, row format 1 is written by the tiled k_edit_fwd_grp32 exactly where the tiled
k_edit_trace_wave reads it, the generic kernel runs wherever a pair can be its own, and the names say what ran."""
import ctypes as C

import pytest

import bsalign_amd as B

G, O, E = B.MODE_GLOBAL, B.MODE_OVERLAP, B.MODE_EXTEND
KNOBS = ("BSA_EDIT_TILED", "BSA_EDIT_GRP", "BSA_EDIT_GRP32", "BSA_EDIT_FWD_LANES", "BSA_EDIT_GEN_LANES", "BSA_EDIT_TRACE_WAVE", "BSA_EDIT_TRACE_LANES", "BSA_EDIT_TRACE_COOP")
CHOICE_KNOBS = set(KNOBS) - {"BSA_EDIT_TILED", "BSA_EDIT_GEN_LANES"}          # each of these keeps row format 0
_ONE = [{}, {"BSA_EDIT_TILED": "0"}, {"BSA_EDIT_TILED": "1"}, {"BSA_EDIT_GRP": "0"}, {"BSA_EDIT_GRP": "1"}, {"BSA_EDIT_GRP32": "0"}, {"BSA_EDIT_GRP32": "1"},
        {"BSA_EDIT_FWD_LANES": "16"}, {"BSA_EDIT_FWD_LANES": "65"}, {"BSA_EDIT_GEN_LANES": "4"}, {"BSA_EDIT_TRACE_WAVE": "0"}, {"BSA_EDIT_TRACE_WAVE": "1"},
        {"BSA_EDIT_TRACE_LANES": "16"}, {"BSA_EDIT_TRACE_LANES": "1"}, {"BSA_EDIT_TRACE_LANES": "3"}, {"BSA_EDIT_TRACE_COOP": "0"}, {"BSA_EDIT_TRACE_COOP": "1"}]
ENVS = _ONE + [{"BSA_EDIT_TRACE_LANES": "4", "BSA_EDIT_TRACE_COOP": "0"}, {"BSA_EDIT_GRP": "1", "BSA_EDIT_GRP32": "1"}, {"BSA_EDIT_TILED": "0", "BSA_EDIT_TRACE_WAVE": "1"},
               {"BSA_EDIT_GRP32": "0", "BSA_EDIT_FWD_LANES": "16"}]
CLASSES = [(bw, 0) for bw in range(64, 1025, 64)] + [(0, w) for w in (0, 1, 2, 4, 8)]
MODES = ((G, 0), (G, 2048), (O, 0), (E, 0))
CUS = (8, 256)
OCC = ((8, 8), (16, 10))
FWD_PREFIX = {B.E_REG: "k_edit_fwd ", B.E_GRP: "k_edit_fwd_grp ", B.E_GRP32: "k_edit_fwd_grp32 ",
              B.E_WIDE: "k_edit_fwd_wide / k_edit_fwd_gen ", B.E_GEN: "k_edit_fwd_wide / k_edit_fwd_gen "}          # (one name for a class above 1024 columns, whichever of the two runs)


def counts(cus):
    """both sides of what the launchers weigh a class by: a wave of pairs, the resident waves of the device, the pair-per-lane kernels' limits, the generic kernel's blocks"""
    return (1, 63, 64, 65, 2 * cus * 32, 2 * cus * 32 + 1, 8 * cus * 32, 8 * cus * 32 + 1, 8 * cus * 16 + 1, 64 * cus * 16 + 1, 16384, 16385, 131103, 131104, 524295, 524296, 2097183, 2097184)


def fwd(d, i):
    return {k[5:]: v for k, v in d.items() if k.startswith("fwd%d_" % i)}


def check(env, d, bw, wide, mode, bandwidth, score, alone, count):
    assert d["launch"]
    f0, f1 = fwd(d, 0), fwd(d, 1)
    launches = [f for f in (f0, f1) if f["form"] != B.E_NONE]
    assert launches and f0["form"] != B.E_NONE
    # every pair has a lane in every launch, and each kernel is asked for at an argument it is built for
    for f in launches:
        form, n = f["form"], f["n"]
        if form == B.E_REG:
            assert n == bw // 64 and 1 <= n <= 16 and 1 <= f["lanes"] <= 64 and f["block"] == 64 and f["grid"] * f["lanes"] >= count
            assert f["track"] == int(mode != G)
        elif form == B.E_GRP:
            assert bw >= 128 and bw // 64 <= n and n in (2, 4, 8, 16) and f["block"] == 256 and f["grid"] * 4 * (64 // n) >= count
        elif form == B.E_GRP32:
            assert bw >= 64 and (bw + 31) // 32 <= n and n in (2, 4, 8, 16) and f["block"] == 256 and f["grid"] * 4 * (64 // n) >= count
        elif form == B.E_WIDE:
            assert bw == 0 and n == wide and n in (1, 2, 4, 8) and f["block"] == 256 and f["grid"] * 4 >= count
        else:
            assert form == B.E_GEN and bw == 0 and 1 <= f["lanes"] <= 64 and f["block"] == 64 and f["grid"] * f["lanes"] >= count
        if form != B.E_REG:
            assert not f["track"]
        if f["tiled"]:
            assert form == B.E_GRP32 and n in (2, 4, 8) and not score
    # bands above 1024 columns: the wave-per-pair kernel where the class has one, the generic kernel wherever a pair may be its own
    forms = [f["form"] for f in launches]
    if bw:
        assert len(launches) == 1 and forms[0] in (B.E_REG, B.E_GRP, B.E_GRP32)
    else:
        assert (B.E_WIDE in forms) == (wide in (1, 2, 4, 8))
        assert (B.E_GEN in forms) == (wide == 0 or (mode == G and bandwidth != 0))
        assert forms == [x for x in (B.E_WIDE, B.E_GEN) if x in forms]
    # the walk: a wave a pair, or a power of two of pairs a wave, cooperative for two to eight of them
    tf, lanes = d["trace_form"], d["trace_lanes"]
    assert tf in (B.T_WAVE, B.T_PLAIN, B.T_COOP) and 1 <= lanes <= 64 and lanes & (lanes - 1) == 0
    assert d["trace_grid"] * lanes >= count
    if tf == B.T_WAVE:
        assert lanes == 1 and d["trace_grid"] == count
    elif lanes == 1:
        assert env.get("BSA_EDIT_TRACE_LANES") == "1"
    assert (tf == B.T_COOP) == (tf != B.T_WAVE and 2 <= lanes <= 8 and env.get("BSA_EDIT_TRACE_COOP") != "0")
    # row format 1: written by one kernel, read by one kernel, for a class that both have to themselves
    tiled_pair = f0["form"] == B.E_GRP32 and f0["tiled"] == 1 and tf == B.T_WAVE and d["trace_tiled"] == 1
    assert d["row_fmt"] in (0, 1) and (d["row_fmt"] == 1) == tiled_pair
    assert f0["tiled"] == d["trace_tiled"] == d["row_fmt"] and not f1["tiled"]
    if not alone or score or env.get("BSA_EDIT_TILED") == "0" or CHOICE_KNOBS & set(env):
        assert d["row_fmt"] == 0
    # the names say what ran
    fn, tn = d["fwd_name"], d["trace_name"]
    assert fn.startswith(FWD_PREFIX[f0["form"]])
    assert ("score-only" in fn) == bool(score) and ("tiled" in fn) == bool(f0["tiled"])
    assert tn == "k_edit_trace" if tf != B.T_WAVE else tn.startswith("k_edit_trace_wave")
    assert ("tiled" in tn) == bool(d["trace_tiled"])
    return forms, tf


def chooser():
    """B.edit_choice without its per-call costs (B.lib() compares the environment at every call): one look at the knobs, one set of buffers"""
    fn = B.lib().bsa_edit_choice_internal
    out, fname, tname = (C.c_uint64 * len(B.EDIT_CHOICE_FIELDS))(), C.create_string_buffer(200), C.create_string_buffer(200)

    def choose(bw, wide, count, mode, bandwidth, score, alone, cus, occ):
        rc = fn(bw, wide, count, mode, bandwidth, int(score), int(alone), cus, occ[0], occ[1], out, fname, tname, 200)
        assert rc >= 0
        d = dict(zip(B.EDIT_CHOICE_FIELDS, out))
        d.update(fwd_name=fname.value.decode(), trace_name=tname.value.decode(), launch=rc == 1)
        return d
    return choose


@pytest.mark.parametrize("env", ENVS, ids=["+".join("%s=%s" % (k[9:], v) for k, v in e.items()) or "defaults" for e in ENVS])
def test_the_choice_keeps_the_launchers_contract(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    choose = chooser()
    seen_fwd, seen_trace, tiled = set(), set(), 0
    for bw, wide in CLASSES:
        for mode, bandwidth in MODES:
            for score in (False, True):
                for alone in (False, True):
                    for cus in CUS:
                        for occ in OCC:
                            for count in counts(cus):
                                d = choose(bw, wide, count, mode, bandwidth, score, alone, cus, occ)
                                forms, tf = check(env, d, bw, wide, mode, bandwidth, score, alone, count)
                                seen_fwd.update(forms)
                                seen_trace.add(tf)
                                tiled += d["row_fmt"]
    if not env:
        assert seen_fwd == {B.E_REG, B.E_GRP, B.E_GRP32, B.E_WIDE, B.E_GEN} and seen_trace == {B.T_WAVE, B.T_PLAIN, B.T_COOP} and tiled > 0


def test_bad_arguments():
    assert B.edit_choice(128, 0, 48)["launch"]
    for bw, wide, count in ((128, 0, 0), (96, 0, 48), (1088, 0, 48), (128, 1, 48), (0, 3, 48)):
        with pytest.raises(ValueError):
            B.edit_choice(bw, wide, count)
    with pytest.raises(ValueError):
        B.edit_choice(128, 0, 48, cus=0)
