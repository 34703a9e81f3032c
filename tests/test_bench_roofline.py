"""bench.py's roofline object (host logic only): fractions cannot exceed 1 by construction, and a PMC traffic entry is
attached only to the machine code it was measured on ("Make the roofline object true")."""
import argparse
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

N32, NNZ32 = 601080390, 9927521280


def _roof(model="heisenberg_chain_32", dtype="f64", kernel="direct-pull+staged", ms=8.3, w=8, symm=False, row_bytes=8):
    args = argparse.Namespace(model=model, dtype=dtype)
    return bench.roofline_object(args, kernel, ms, 1, N32, N32, NNZ32, w, 1, ms * 1e-3, symm, row_bytes=row_bytes)


def test_kernel_isa_file_belongs_to_the_tree():
    path = os.path.join(ROOT, "distributed-matvec_amd", "kernel_isa.json")
    assert os.path.exists(path), "run __graft_entry__.build() (csrc/Makefile writes kernel_isa.json)"
    with open(path) as f:
        isa = json.load(f)
    assert isa["source_sha"] == bench.source_sha(), "kernel_isa.json is stale: rebuild"
    for fam in ("k_chain_t", "k_tile_pull", "k_tile", "k_direct", "k_scatter", "k_diag"):
        assert len(isa["families"][fam]["isa_sha"]) == 16
    assert bench.kernel_isa_sha("k_chain_t") == isa["families"]["k_chain_t"]["isa_sha"]
    assert bench.kernel_isa_sha("no_such_kernel") is None


def test_pull_fractions_cannot_exceed_one_at_the_copy_rate():
    # a pull kernel that moved only its compulsory bytes at the HBM peak would sit at frac == 1; at any real time below
    r = _roof(ms=8.3)
    assert r["formulation"].startswith("pull")
    # the staged f64 kernel streams ONE fused 8-byte sigma|partner record per row next to x and y: 24 B per row (VERDICT r2:
    # charging 28 flattered the fraction by 17 %); the row bytes are the plan's (ls_amd_plan_row_bytes), not a guess
    assert r["algorithmic_bytes_per_launch"] == N32 * 24
    assert _roof(dtype="c128", w=16, row_bytes=8)["algorithmic_bytes_per_launch"] == N32 * (4 + 4 + 32)
    assert _roof(kernel="tile-pull", row_bytes=16)["algorithmic_bytes_per_launch"] == N32 * (16 + 16)
    assert 0 < r["frac"] < 1 and r["frac"] == r["frac_compulsory"]
    t_peak_ms = r["algorithmic_bytes_per_launch"] / (bench.HBM_PEAK_GBPS * 1e9) * 1e3
    assert abs(_roof(ms=t_peak_ms)["frac"] - 1.0) < 1e-12
    # the push formula is only a cross-reference for pull kernels
    assert r["survey_formula"]["B_alg_push_bytes_per_matvec"] == N32 * 24 + NNZ32 * 16
    p = _roof(kernel="direct-push", ms=74.0)
    assert p["formulation"].startswith("push") and p["algorithmic_bytes_per_launch"] == N32 * 16 + NNZ32 * 16
    assert 0 < p["frac"] < 1
    # the staged push kernel (round 6) executes the same formulation: the same bytes, its own PMC entry on its own machine code
    ps = _roof(kernel="direct-push+staged", ms=41.9)
    assert ps["formulation"].startswith("push") and "staged" in ps["formulation"] and ps["algorithmic_bytes_per_launch"] == p["algorithmic_bytes_per_launch"]
    assert 0.49 < ps["frac"] < 0.51
    with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
        ent = json.load(f)["heisenberg_chain_32/f64/direct-push+staged"]
    assert ent["device_kernel"] == "k_push_t" and ent["instance"].startswith("k_push_t<")
    if bench.kernel_instance_sha(ent["instance"]) == ent["instance_isa_sha"]:  # (attached while the kernel is what was measured)
        assert ps["traffic"] == ent["traffic_bytes"] and ps["wasted_traffic"] < 1.0  # atomics combine: fewer bytes than the formula charges


def test_traffic_is_attached_only_to_the_code_it_measured(monkeypatch):
    with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
        ent = json.load(f)["heisenberg_chain_32/f64/direct-pull+staged"]
    assert ent["device_kernel"] == "k_chain_t" and ent.get("isa_sha")
    # same machine code -> attached, with fractions <= 1 and the waste factor >= 1
    monkeypatch.setattr(bench, "kernel_isa_sha", lambda fam: ent["isa_sha"] if fam == "k_chain_t" else None)
    r = _roof(ms=8.3)
    assert r["traffic"] == ent["traffic_bytes"]
    # ... or the measured instantiation alone is unchanged while a sibling of the family was edited / removed
    monkeypatch.setattr(bench, "kernel_isa_sha", lambda fam: "0" * 16)
    monkeypatch.setattr(bench, "kernel_instance_sha", lambda inst: ent["instance_isa_sha"] if inst == ent["instance"] else None)
    assert _roof(ms=8.3)["traffic"] == ent["traffic_bytes"]
    assert 0 < r["frac_traffic"] <= 1.0 and r["wasted_traffic"] >= 1.0
    # different machine code and different source -> refused, and the note says why
    monkeypatch.setattr(bench, "kernel_isa_sha", lambda fam: "0" * 16)
    monkeypatch.setattr(bench, "kernel_instance_sha", lambda inst: "1" * 16)
    monkeypatch.setattr(bench, "source_sha", lambda: "f" * 16)
    r = _roof(ms=8.3)
    assert r["traffic"] is None and r["frac_traffic"] is None and "stale" in r["traffic_note"]
    # a fingerprint file that does not belong to the tree's source is ignored altogether
    monkeypatch.undo()
    monkeypatch.setattr(bench, "source_sha", lambda: "f" * 16)
    assert bench.kernel_isa_sha("k_chain_t") is None


@pytest.mark.parametrize("key", ["heisenberg_chain_32/f64/direct-pull+staged", "heisenberg_chain_32/c128/direct-pull+staged"])
def test_headline_entries_describe_this_build(key):
    """The driver's bench line carries `traffic` only if the committed PMC passes belong to the shipped k_chain_t.  This
    test does not fail on a kernel edit -- it reports: a stale entry means re-running scripts/gpu_pmc_traffic.sh."""
    with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
        ent = json.load(f)[key]
    if bench.kernel_isa_sha("k_chain_t") != ent.get("isa_sha") and bench.kernel_instance_sha(ent.get("instance", "")) != ent.get("instance_isa_sha"):
        pytest.skip("k_chain_t changed since the committed PMC passes: traffic will be null until re-measured")
    model, dtype, kernel = key.split("/")
    r = _roof(model=model, dtype=dtype, kernel=kernel, ms=8.3 if dtype == "f64" else 14.7, w=8 if dtype == "f64" else 16)
    assert r["traffic"] == ent["traffic_bytes"] and r["frac_traffic"] <= 1.0


@pytest.mark.parametrize("model", ["heisenberg_chain_32", "heisenberg_chain_36_symm", "heisenberg_chain_40_symm"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 8])
def test_scaling_model_of_the_multi_gpu_line_is_total_and_serialisable(model, P):
    """`bench.py --gpus N` attaches scaling_model(...) to its JSON line at every N the driver's SCALE run uses: pure arithmetic that
    has never executed with N > 1 on hardware -- it must not raise, must serialise, and must order its bounds"""
    import json

    m = bench.scaling_model(model, P, fused_ms=7.7 if not model.endswith("_symm") else 280.0)
    if P < 2:
        assert m is None
        return
    json.dumps(m)
    lo, hi = m["predicted_ms_per_matvec"]
    assert 0 < lo <= hi
    s_lo, s_hi = m["predicted_speedup_over_one_gpu"]
    assert 0 < s_lo <= s_hi
    assert m["x_bytes_in_per_rank"] <= bench.MODEL_STATES[model] * 8 * (P - 1) / P
    if model.endswith("_symm"):
        c_lo, c_hi = m["predicted_ms_per_matvec_slot_cache"]
        assert 0 < c_lo <= c_hi <= hi
    assert bench.scaling_model(model, P, fused_ms=None) is None and bench.scaling_model("no_such_model", P, fused_ms=1.0) is None


def test_default_cpu_sample_and_model_config_need_no_reference_tree():
    """what the default run decides before it touches the GPU: the CPU-baseline sample size and the model input (from
    tests/golden/models.json -- /root/reference does not exist on the GPU box)"""
    assert bench.default_cpu_sample(20) == 20 and bench.default_cpu_sample(32) in (28, 32)
    for name in ("heisenberg_chain_32", "heisenberg_chain_36_symm", "heisenberg_chain_40_symm", "heisenberg_chain_28"):
        cfg, src = bench.model_config(name)
        L, symm = bench.parse_model(name)
        assert cfg["basis"]["number_spins"] == L and bool(cfg["basis"].get("symmetries")) == symm
        assert "/root/reference" not in src


def test_cpu_baseline_legs_on_small_samples():
    """the `cpu_baseline` objects of the --full run (the oracle timed on the host cores; the only place outside tests/ and smoke()
    that may call oracle/): both legs on samples that take a second -- they must produce a positive rate, say what the sample was,
    and label a scaled figure as scaled"""
    from oracle import c_oracle as CO
    from oracle import model as M

    s = bench.cpu_baseline(18, repeats=2)
    assert s["seconds_per_matvec"] > 0 and s["n"] == 48620 and s["nnz"] == bench.chain_nnz(18, 48620) and s["timed_matvecs"] == 2
    name = "heisenberg_chain_24_symm"
    o = CO.COracle(M.model_from_config(bench.model_config(name)[0]))
    reps = o.enumerate()
    nnz = bench.chain_nnz(24, len(reps))
    measured = bench.cpu_baseline_projected(name, reps, nnz, budget_s=60.0)
    assert measured["value"] > 0 and measured["scaled"] is False and "itself" in measured["sample"] and measured["kind"] == "port"
    scaled = bench.cpu_baseline_projected(name, None, nnz, probe=measured["probe"])
    assert scaled["scaled"] is True and scaled["sample"].startswith("SCALED") and scaled["value"] > 0
    for obj in (measured, scaled):
        obj.pop("probe", None)
        json.dumps(obj)


def test_dump_outputs_is_a_fixed_float64_sample(tmp_path):
    """--dump-outputs: float64 files only, the same positions in every run, the values at those positions, < 64 MB in all"""
    import numpy as np
    import torch

    n = 3 * bench.DUMP_SAMPLE
    y = torch.from_numpy(np.random.RandomState(1).rand(n))
    bench.dump_outputs(str(tmp_path / "a"), "y", y)
    bench.dump_outputs(str(tmp_path / "b"), "y", y)
    idx, val = (np.load(str(tmp_path / "a" / f)) for f in ("y_index.npy", "y.npy"))
    assert idx.dtype == val.dtype == np.float64 and len(idx) == len(val) <= bench.DUMP_SAMPLE
    assert np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(val, y.numpy()[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(str(tmp_path / "b" / "y_index.npy")))
    yc = torch.complex(y, -y)  # c128: real and imaginary part, the largest dump there is
    bench.dump_outputs(str(tmp_path / "c"), "y", yc)
    files = sorted(os.listdir(str(tmp_path / "c")))
    assert files == ["y_imag.npy", "y_index.npy", "y_real.npy"]
    assert np.array_equal(np.load(str(tmp_path / "c" / "y_imag.npy")), -np.load(str(tmp_path / "c" / "y_real.npy")))
    assert sum(os.path.getsize(str(tmp_path / "c" / f)) for f in files) < 64e6
    small = torch.arange(10, dtype=torch.float64)  # short vectors: whole
    bench.dump_outputs(str(tmp_path / "d"), "y", small)
    assert sorted(os.listdir(str(tmp_path / "d"))) == ["y.npy"]
    assert np.array_equal(np.load(str(tmp_path / "d" / "y.npy")), small.numpy())


def test_inject_fault_needs_full():
    """the fault-injection hook tests the parity checks, which only --full runs: without it the benchmark refuses at once"""
    import subprocess

    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--inject-fault"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--full" in p.stderr
