"""GPU: bench.py keeps its output contract -- ONE JSON line on stdout with the keys the driver reads; with --full also the roofline and
cpu_baseline objects and a parity spot check -- on a small instance of every workload.  A plain run is lean: the headline line alone,
and what it dumps is what a --full run dumps."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import support as S

pytestmark = pytest.mark.gpu

KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


@pytest.mark.parametrize("args", [
    ["--pairs", "2048", "--length", "2000", "--cpu-pairs", "20"],
    ["--workload", "edit", "--pairs", "1024", "--length", "5000", "--cpu-pairs", "10"],
    ["--workload", "edit", "--mode", "extend", "--bw", "-1", "--pairs", "512", "--length", "3000", "--cpu-pairs", "10"],
    ["--workload", "poa", "--pairs", "256", "--length", "800", "--cpu-pairs", "-1"],
    ["--workload", "poa", "--poa-source", "fixture", "--pairs", "64", "--cpu-pairs", "-1"],
], ids=["align8", "edit", "edit-extend-full", "poa", "poa-fixture"])
def test_one_json_line_with_the_contract_keys(args):
    r = subprocess.run([sys.executable, os.path.join(S.ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1"] + args,
                       capture_output=True, text=True, timeout=900, cwd=S.ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    for k in KEYS:
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["higher_is_better"] is True and j["scaling"] == "weak"
    assert j["value"] > 0 and j["ms_per_step"] > 0 and j["vs_baseline"] is None and "workload" in j["config"]
    rf = j["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    if "checks" in j and "oracle_identical_first8" in j["checks"]:
        assert j["checks"]["oracle_identical_first8"] is True and j["checks"]["pairs_flagged"] == 0
    if "fixture" in args:          # the committed programs: runs with oracle/_ref absent, every best end cell the reference's
        assert j["checks"]["best_end_cell_identical_all_programs"] is True and j["checks"]["programs"] == 64 * 6 and j["cpu_baseline"]["value"] is None
    if "--workload" not in args:
        # the pairwise line says what sits outside the timed region and validates the shard exchange on its own batch
        cfg, ex = j["config"], j["exchange"]
        assert cfg["plan_ms"] > 0 and cfg["pcie_inclusive_ms"] > j["ms_per_step"] and cfg["per_rank_gcups"] == [j["value"]] and cfg["ranks_counted"] == 1
        assert ex["pairs"] == 2048 and ex["ranks"] == 1 and ex["gathered_identical_to_rank0_whole_batch"] is True and ex["host_pointer_call_identical"] is True
        assert ex["round_trip_ms"] > 0 and ex["backend"] == "nccl"
    if args[-1] != "-1":
        cb = j["cpu_baseline"]
        # one pinned process per physical core the container may use, the one-core figure beside it (poa: one core)
        assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("reference", "port") and cb["sample"]
        assert cb["cores"] == 1 or (cb["one_core_alone"] > 0 and cb["per_core"] > 0)


def test_full_run_carries_the_three_workloads():
    """`python bench.py --full` (here with fewer steps): the headline line with "secondary" = the edit (C3) and POA lines measured in the
    same run, each with its own roofline and cpu_baseline; plan cost and the PCIe-inclusive time in config"""
    r = subprocess.run([sys.executable, os.path.join(S.ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1"], capture_output=True, text=True, timeout=1500, cwd=S.ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert j["config"]["pairs_per_gpu"] == 100000 and j["config"]["plan_ms"] > 0 and j["config"]["pcie_inclusive_ms"] > j["ms_per_step"]
    assert j["exchange"]["gathered_identical_to_rank0_whole_batch"] is True and j["exchange"]["pairs"] == 100000
    sec = j["secondary"]
    assert len(sec) == 3 and all("error" not in d for d in sec), sec
    ed, po, wq = sec
    # round 6: whole-query bands with scores outside the static guard on the checked systolic kernel, beside its own CPU baseline (>= 300 GCUPS, >= 5 x)
    assert "bandwidth 0" in wq["config"]["workload"] and "CHK" in wq["roofline"]["kernel"] and wq["checks"]["oracle_identical_first8"] is True
    assert wq["value"] >= 300 and wq["value"] >= 5 * wq["cpu_baseline"]["value"] and wq["checks"]["pairs_flagged"] <= 20
    assert ed["metric"].startswith("GCUPS") and "edit" in ed["config"]["workload"] and ed["value"] > 0 and ed["roofline"]["frac"] > 0 and ed["cpu_baseline"]["value"] > 0
    assert ed["checks"]["oracle_identical_first8"] is True and ed["config"]["plan_ms"] > 0
    assert "poa" in po["config"]["workload"] and po["value"] > 0 and po["roofline"]["frac"] > 0 and po["checks"]["best_end_cell_identical_all_programs"] is True
    print("\n[bench.py --full] align8 %.0f GCUPS (%.1f ms/step, plan %.0f ms, PCIe-inclusive %.0f ms), edit %.0f GCUPS, poa %.1f GCUPS, whole query out of guard %.0f GCUPS; secondaries took %.0f + %.0f + %.0f s"
          % (j["value"], j["ms_per_step"], j["config"]["plan_ms"], j["config"]["pcie_inclusive_ms"], ed["value"], po["value"], wq["value"], ed["wall_s"], po["wall_s"], wq["wall_s"]))


FULL_ONLY = ("cpu_baseline", "exchange", "exchange_ok", "secondary", "lockstep_end_to_end")


def _bench(argv, timeout=900):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(S.ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=timeout, cwd=S.ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), wall


@pytest.mark.parametrize("args", [
    ["--pairs", "2048", "--length", "2000"],
    ["--workload", "edit", "--pairs", "1024", "--length", "5000"],
    ["--workload", "poa", "--poa-source", "fixture", "--pairs", "64"],
], ids=["align8", "edit", "poa-fixture"])
def test_plain_run_is_the_headline_alone_and_dumps_what_full_dumps(args, tmp_path):
    """without --full: the contract keys, none of the checks, baselines or exchange that --full adds, and --dump-outputs writes the same arrays as
    a --full run of the same command"""
    plain, _ = _bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain")] + args)
    full, _ = _bench(["--full", "--cpu-pairs", "-1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "full")] + args)
    for k in KEYS:
        assert k in plain, k
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["higher_is_better"] is True
    for k in ("metric", "unit", "dtype", "n_gpus", "scaling", "vs_baseline", "data"):
        assert plain[k] == full[k], k
    assert not any(k in plain for k in FULL_ONLY), sorted(plain)
    assert not any(k.startswith("oracle_identical") for k in plain.get("checks", {})), plain.get("checks")
    if "--workload" not in args:
        assert plain["config"]["pcie_inclusive_ms"] is None and plain["checks"]["pairs_flagged"] == 0
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    assert plain["outputs_dumped"]["arrays"] == full["outputs_dumped"]["arrays"]
    for nm in names:
        assert np.array_equal(np.load(tmp_path / "plain" / nm), np.load(tmp_path / "full" / nm)), nm


def test_plain_default_run_spends_little_outside_its_steps():
    """`python bench.py --steps N --warmup W`: the C2 headline line without the secondary workloads, and (wall time of the whole process) - (N + W) x
    ms_per_step well inside 30 s"""
    j, wall = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert j["config"]["pairs_per_gpu"] == 100000 and j["value"] > 0
    assert not any(k in j for k in FULL_ONLY), sorted(j)
    outside = wall - (3 + 1) * j["ms_per_step"] / 1e3
    print("\n[bench.py plain] %.0f GCUPS, %.1f ms/step; %.1f s of %.1f s outside the steps" % (j["value"], j["ms_per_step"], outside, wall))
    assert outside < 30.0
