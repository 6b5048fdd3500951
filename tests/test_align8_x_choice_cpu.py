"""x_choose (bsa_align8_x.hip), the one function that decides what the exact-arithmetic forward launchers launch, on a grid of chunks, host only
(bsa_align8_x_choice_internal).  What is asserted is the launcher's contract with its kernels and its callers, not its code: the grid covers every pair, row
segments cover every row and fit the buffer the caller has, a buffer of bsa_align8_xq_bytes admits row segments wherever a row-segment form exists, the
absolute-score form is chosen exactly where bsa_align8_abs_rows allows it, score-only launches write no codes, every combination the kernels exist for gets a
launch and every other one an error."""
import ctypes as C
import re

import pytest

import bsalign_amd as B

SC = {"linear": (2, -6, 0, -3, 0, 0), "affine": (2, -6, -3, -2, 0, 0), "twopiece": (2, -6, -3, -2, -8, -1),
      "s57": (54, -2, -1, -1, 0, 0)}          # s57: integer maxima at bandwidth 256 (tests/test_align8_m3_gpu.py)
PW = {"linear": 0, "affine": 1, "twopiece": 2, "s57": 1}
CUS = (8, 256)
TLENS = (50, 10000)
KNOBS = ("BSA_ALIGN8_XQ", "BSA_ALIGN8_XQ_SEG", "BSA_ALIGN8_XQ_SPIN_CAP", "BSA_ALIGN8_X_LANES", "BSA_ALIGN8_X_N8", "BSA_ALIGN8_X2_LANES", "BSA_ALIGN8_NO_STATIC",
         "BSA_ALIGN8_ABS", "BSA_ALIGN8_ABS_R", "BSA_ALIGN8_DO2")
# each knob unset and set, alone and together with BSA_ALIGN8_XQ=1 (which takes the batch size out of the choice between row segments and whole pairs)
_ONE = [{}, {"BSA_ALIGN8_XQ": "0"}, {"BSA_ALIGN8_XQ_SEG": "64"}, {"BSA_ALIGN8_XQ_SEG": "1001"}, {"BSA_ALIGN8_XQ_SPIN_CAP": "5"}, {"BSA_ALIGN8_X_LANES": "4"},
        {"BSA_ALIGN8_X_LANES": "8"}, {"BSA_ALIGN8_X_N8": "16"}, {"BSA_ALIGN8_X_N8": "0"}, {"BSA_ALIGN8_X2_LANES": "8"}, {"BSA_ALIGN8_NO_STATIC": "1"},
        {"BSA_ALIGN8_ABS": "0"}, {"BSA_ALIGN8_ABS_R": "8"}, {"BSA_ALIGN8_DO2": "0"}]
ENVS = _ONE + [dict(e, BSA_ALIGN8_XQ="1") for e in _ONE if "BSA_ALIGN8_XQ" not in e]

# Chunks that ask for row segments (BSA_ALIGN8_XQ=1), have a buffer of exactly bsa_align8_xq_bytes and a row-segment form, and still do not get one: (env, case) --
# expected to be empty.  (At bandwidth 128 with two-piece gaps the launcher's first try, <16, 4>, does not fit that size for 1..8, 17..24 and 33..40 pairs; it then
# takes the <8, 8> segments the size is made for, so those chunks are not entries.)
NO_SEGMENTS_DESPITE_ROOM = []


def counts(cus):
    return (1, 31, 32, 33, 48, 64, 65, 16 * cus * 4, 16 * cus * 4 + 1, 100000)


def xs_words(W, pw):
    """dwords a lane of a wave's state block (k_align8_fwd_xq: the two row planes -- three with two-piece gaps --, and eleven more)"""
    return (3 if pw == 2 else 2) * W + 11


def has_segment_form(env, bw, pw, score, fmt):
    """the row-segment kernels that exist: none for two-piece gaps at 256, none for eight lanes per pair at 64, none beside the mix's lane-count knobs"""
    lanes = env.get("BSA_ALIGN8_X_LANES")
    if pw == 2 and bw == 256:
        return False
    if not score and bw == 64 and pw <= 1 and lanes == "8":
        return False
    if not score and fmt == 0 and bw == 128 and pw == 1 and (lanes is not None or "BSA_ALIGN8_X_N8" in env):
        return False
    return True


def check(env, d, abs_form, bw, sc, static, score, fmt, count, tlen, cus, xq_bytes):
    pw = PW[sc]
    assert d["gap_model"] == pw
    supported = not (fmt == 1 and not (pw == 1 and bw == 128)) and not (score and (pw == 2 or fmt == 1))
    assert d["launch"] == supported
    if not supported:
        assert d["form"] == B.X_NONE
        return
    form, W, L = d["form"], d["W"], d["L"]
    assert form in (B.X_STATIC, B.X_SEG, B.X_WHOLE, B.X_MIX)
    assert 2 * W * L == bw and d["pw"] == pw
    assert d["score"] == int(score) and d["do2"] == int(fmt == 1)
    assert not (d["score"] and (d["abs"] or d["do2"]))
    # every pair has its lanes
    if form in (B.X_STATIC, B.X_WHOLE):
        assert d["grid"] * 256 // L >= count
    elif form == B.X_SEG:
        assert d["groups"] * 64 // L >= count and d["grid"] == d["groups"] * d["nseg"]
    else:
        n8, n4 = d["n8"], count - d["n8"]
        assert 0 < n8 < count and L == 4 and d["nb8"] * 32 >= n8 and (d["grid"] - d["nb8"]) * 64 >= n4
        assert bw == 128 and pw == 1 and fmt == 0 and not score
    # band in place exactly where the batch allows it and a kernel exists
    in_place = static and "BSA_ALIGN8_NO_STATIC" not in env and not (pw == 2 and bw != 128)
    assert (form == B.X_STATIC) == in_place
    # row segments: every row, the kernel's state layout, inside the caller's buffer
    if form == B.X_SEG:
        assert env.get("BSA_ALIGN8_XQ") != "0" and xq_bytes > 0
        assert d["nseg"] >= 1 and d["nseg"] * d["seg_rows"] >= tlen and d["seg_rows"] % 8 == 0 and d["seg_rows"] >= 64
        assert d["ctl_bytes"] >= (16 + d["groups"]) * 4 and d["state_bytes"] == d["groups"] * xs_words(W, pw) * 64 * 4
        assert d["ctl_bytes"] + d["state_bytes"] <= xq_bytes
        assert d["wps"] in (2, 3) and d["spin_cap"] == (5 if "BSA_ALIGN8_XQ_SPIN_CAP" in env else 1 << 22)
        assert d["rmask"] == (d["rebase_rows"] - 1 if d["abs"] else 0)
        assert has_segment_form(env, bw, pw, score, fmt)
        if env.get("BSA_ALIGN8_XQ") != "1":
            assert d["groups"] > cus * 4 * d["wps"]          # one generation of resident waves runs whole pairs
    elif env.get("BSA_ALIGN8_XQ") == "1" and not in_place and xq_bytes >= d["xq_need"] > 0 and has_segment_form(env, bw, pw, score, fmt):
        assert (env, (bw, sc, static, score, fmt, count, tlen, cus)) in NO_SEGMENTS_DESPITE_ROOM
    if W == 4:
        assert env.get("BSA_ALIGN8_X_LANES") == "8" and form == B.X_WHOLE
    # the absolute-score form where bsa_align8_abs_rows allows it, with its maxima and period
    if d["abs"]:
        assert abs_form[0] in (1, 2) and d["m3"] == int(abs_form[0] == 2) and d["rebase_rows"] == abs_form[1]
        assert bw in (128, 256) and pw <= 1 and W == 16 and form != B.X_STATIC
    else:
        assert not d["m3"] and not d["rebase_rows"]
        if abs_form[0] in (1, 2) and not score and form != B.X_STATIC:
            assert bw == 128 and pw == 1 and L == 8          # the eight-lane whole-pair kernel keeps the difference form
    # the name says what ran
    name = d["name"]
    if name:
        assert name.startswith({B.X_STATIC: "k_align8_fwd_x_static", B.X_SEG: "k_align8_fwd_xq", B.X_WHOLE: "k_align8_fwd_x", B.X_MIX: "k_align8_fwd_x_mix"}[form])
        assert ("score-only" in name) == bool(score) and ("two-bit D/Od" in name) == (fmt == 1)
        m = re.search(r"\[rebase every (\d+) rows\] \[(three-operand maxima, biased frame|integer maxima)\]$", name)
        assert bool(m) == bool(d["abs"])
        if m:
            assert int(m.group(1)) == d["rebase_rows"] and (m.group(2) == "integer maxima") == (not d["m3"])
    else:
        assert not score and fmt == 0 and not d["abs"]          # (these show bsa_align_run's default for the path)


def chooser():
    """B.align8_x_choice without its per-call costs (B.lib() compares the environment at every call): one look at the knobs, one pair of buffers"""
    fn = B.lib().bsa_align8_x_choice_internal
    out, name = (C.c_uint64 * len(B.X_CHOICE_FIELDS))(), C.create_string_buffer(400)

    def choose(par, count, tlen, static, fmt, score, xq_bytes, cus):
        rc = fn(par, count, tlen, int(static), fmt, int(score), xq_bytes, cus, out, name, 400)
        assert rc >= 0
        d = dict(zip(B.X_CHOICE_FIELDS, out))
        d.update(name=name.value.decode(), launch=rc == 1)
        return d
    return choose


@pytest.mark.parametrize("env", ENVS, ids=["+".join("%s=%s" % (k[11:], v) for k, v in e.items()) or "defaults" for e in ENVS])
def test_the_choice_keeps_the_launchers_contract(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    choose = chooser()
    seen = set()
    for bw in (64, 128, 256):
        for sc in SC:
            par = B.make_params(B.MODE_GLOBAL, bw, *SC[sc])
            abs_form = B.align8_abs_form(par)
            for static in (False, True):
                for score in (False, True):
                    for fmt in (0, 1):
                        for cus in CUS:
                            for count in counts(cus):
                                for tlen in TLENS:
                                    need = 0
                                    for claim in (0, 1, 2):          # no buffer, half of what bsa_align_run would allocate, all of it
                                        xq_bytes = need * claim // 2
                                        d = choose(par, count, tlen, static, fmt, score, xq_bytes, cus)
                                        check(env, d, abs_form, bw, sc, static, score, fmt, count, tlen, cus, xq_bytes)
                                        need = d["xq_need"]
                                        seen.add(d["form"])
    assert {B.X_NONE, B.X_WHOLE} <= seen
    if not env:
        assert seen == {B.X_NONE, B.X_STATIC, B.X_SEG, B.X_WHOLE, B.X_MIX}


def test_widths_without_kernels_and_bad_arguments():
    par = B.make_params(B.MODE_GLOBAL, 80, *SC["affine"])
    assert not B.align8_x_choice(par, 48, 400)["launch"]
    with pytest.raises(ValueError):
        B.align8_x_choice(B.make_params(B.MODE_GLOBAL, 128, *SC["affine"]), 0, 400)


def test_buffer_size_is_the_recorded_formula():
    """bsa_align_run sizes the row-segment buffer by bsa_align8_xq_bytes: 64 control dwords and one a group, a spare 256 bytes, the groups' state blocks at the shape
    of the bandwidth and gap model (two-piece gaps at 256 have a size though no row-segment kernel)"""
    shape = {(64, 0): (8, 4), (64, 1): (8, 4), (64, 2): (8, 4), (128, 0): (16, 4), (128, 1): (16, 4), (128, 2): (8, 8), (256, 0): (16, 8), (256, 1): (16, 8), (256, 2): (16, 8)}
    for (bw, pw), (W, L) in shape.items():
        par = B.make_params(B.MODE_GLOBAL, bw, *SC[("linear", "affine", "twopiece")[pw]])
        for count in counts(256):
            groups = (count * L + 63) // 64
            assert B.align8_x_choice(par, count, 400)["xq_need"] == (16 + groups) * 4 + 256 + groups * xs_words(W, pw) * 256
