#!/usr/bin/env python3
"""What the block form of the PROJECTING cross-sector product buys: CrossSectorPlan.apply_block(method="kernel") on a
groups="project" plan (k_cross_project_blk, k_cross_project_blk_fermi: the target's element loop, the term sums, the projection of
every packet and its look-up once per chunk of 8 columns) against method="columns" (the loop of k_cross_project over the columns,
which repeats all of that for every column), on the two projecting plans that scripts/cross_groups_bench.py times:
  spin      S^z_q on heisenberg_chain_32, (k = 0, reflection 0, inversion +1) -> translations-only k = q (default 5)
  fermion   n_q on the 28-mode t-V ring at half filling, (k = 0, reflection 0) -> translations-only k = q
for K = 8 interleaved, K = 8 column-major and K = 64 interleaved blocks.  c128, device events, 1 warm-up and 3 timed runs of each,
alternating in one process; min-max.  Every record also holds one single apply of the plan, next to which the time per column of
either path reads.  --thermal adds evolve.thermal_correlation runs on the spin pair (K = 8 random vectors, four output times,
groups="project", bounds [-3 L, L] by the norm of the bonds, so that no Lanczos run is timed), one per path, with the share of the
time spent in apply_block.  One JSON line per record, appended to --out.
usage: cross_project_block_bench.py [--which spin|fermion|both] [--sites 32] [--modes 28] [--q 5] [--steps 3] [--warmup 1] [--thermal]
                                    [--out profiles/cross_project_block_bench.jsonl]"""
import argparse
import cmath
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config, evolve  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--which", default="both", choices=["spin", "fermion", "both"])
ap.add_argument("--sites", type=int, default=32)
ap.add_argument("--modes", type=int, default=28)
ap.add_argument("--q", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--thermal", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dtype = torch.complex128
torch.cuda.set_device(0)
SHAPES = [(8, "interleaved"), (8, "column-major"), (64, "interleaved")]


def phase(L, q, j):
    z = cmath.exp(-2j * math.pi * q * j / L)
    return "(" + repr(z.real) + ("+" if z.imag >= 0 else "-") + repr(abs(z.imag)) + "j)"


def symmetries(L, k, reflection=None):
    sym = [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]
    if reflection is not None:
        sym.append({"permutation": [L - 1 - i for i in range(L)], "sector": reflection})
    return sym


def spin_basis(L, k, full=False):
    b = {"number_spins": L, "hamming_weight": L // 2, "symmetries": symmetries(L, k, 0 if full else None)}
    if full:
        b["spin_inversion"] = 1
    return {"basis": b}


def fermi_basis(L, k, full=False):
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": L // 2, "symmetries": symmetries(L, k, 0 if full else None)}}


def momentum_op(L, q, one):
    return {"terms": [{"expression": phase(L, q, j) + one, "sites": [[j]]} for j in range(L)]}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def kernel_against_columns(head, src_cfg, dst_cfg, op_cfg):
    t0 = time.perf_counter()
    sbasis = D.loadConfigFromDict(src_cfg)
    tbasis = D.loadConfigFromDict(dst_cfg)
    A = D.Operator.fromSpec(sbasis, config.parse_operator(op_cfg, sbasis.spec))
    sreps, _ = D.enumerateStates(sbasis, 1)
    treps, _ = D.enumerateStates(tbasis, 1)
    cross = D.CrossSectorPlan(A, sreps[0], tbasis, treps[0], dtype, groups="project")
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    n1, n2 = int(sreps[0].numel()), int(treps[0].numel())
    x1 = D.fillRandom(sreps[0], 1, dtype)
    y1 = torch.zeros(n2, dtype=dtype, device="cuda")
    for K, layout in SHAPES:
        x = torch.stack([D.fillRandom(sreps[0], 1 + k, dtype) for k in range(K)], dim=1).contiguous()
        if layout == "interleaved":
            ys = {m: torch.zeros((n2, K), dtype=dtype, device="cuda") for m in ("kernel", "columns")}
        else:
            x = x.t().contiguous().t()
            ys = {m: torch.zeros((K, n2), dtype=dtype, device="cuda").t() for m in ("kernel", "columns")}
        runs = {m: (lambda m=m: cross.apply_block(x, ys[m], check=False, method=m)) for m in ys}
        runs["apply"] = lambda: cross.apply(x1, y1, check=False)
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        cross.check()
        diff, size = float((ys["kernel"] - ys["columns"]).abs().max()), float(ys["columns"].abs().max())
        ms = {m: [] for m in runs}
        for _ in range(args.steps):  # alternating
            for m, fn in runs.items():
                ms[m].append(timed(fn))
        cross.check()
        for v in ms.values():
            v.sort()
        tk, tc, ta = ms["kernel"], ms["columns"], ms["apply"]
        emit({**head, "dtype": "c128", "K": K, "layout": layout, "n_source": n1, "n_target": n2, "cross_nnz": cross.nnz,
              "kernel": cross.block_kernel(K, "kernel"), "column_kernel": cross.kernel, "steps": args.steps, "warmup": args.warmup,
              "kernel_ms_min": round(tk[0], 4), "kernel_ms_max": round(tk[-1], 4), "columns_ms_min": round(tc[0], 4), "columns_ms_max": round(tc[-1], 4),
              "apply_ms_min": round(ta[0], 4), "apply_ms_max": round(ta[-1], 4),
              "kernel_ms_per_column": round(tk[0] / K, 4), "columns_ms_per_column": round(tc[0] / K, 4),
              "kernel_over_columns_min": round(tk[0] / tc[-1], 4), "kernel_over_columns_max": round(tk[-1] / tc[0], 4),
              "kernel_is_faster": bool(tk[-1] < tc[0]),  # beyond the min-max spread of the timed runs
              "max_abs_difference": diff, "max_abs_y": size, "setup_seconds": round(setup_s, 2)})
    cross.destroy()


def thermal(L, q, method):
    """one thermal_correlation on the spin pair with every apply_block bracketed by device events"""
    events = []
    inner = D.CrossSectorPlan.apply_block

    def bracketed(self, x, y, check=True, method=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inner(self, x, y, check=check, method=method)
        e1.record()
        events.append((e0, e1))

    cfg = config.heisenberg_chain_config(L)
    cfg["basis"] = spin_basis(L, 0, full=True)["basis"]
    cfg["observables"] = [momentum_op(L, q, " σᶻ₀")]
    times = [0.0, 0.05, 0.1, 0.15]
    D.CrossSectorPlan.apply_block = bracketed
    try:
        torch.cuda.synchronize()
        res = evolve.thermal_correlation(cfg, 0, 0.1, times, num_vectors=8, seed=1, target=spin_basis(L, q)["basis"], groups="project",
                                         bounds=(-3.0 * L - 0.5, L + 0.5), block_method=method)
        torch.cuda.synchronize()
    finally:
        D.CrossSectorPlan.apply_block = inner
    apply_ms = sum(e0.elapsed_time(e1) for e0, e1 in events)
    emit({"record": "thermal_correlation", "model": f"heisenberg_chain_{L}", "source_symmetries": "translation+reflection+inversion",
          "target_symmetries": "translation", "operator": "S^z_q", "groups": "project", "block_method": method, "target_sector": q, "K": 8,
          "beta": 0.1, "times": times, "dimension": res.dimension, "bounds": list(res.bounds), "orders": [int(n) for n in res.orders],
          "matvec_columns": res.matvec_columns, "kernel": res.kernel, "apply_block_calls": len(events), "apply_block_ms": round(apply_ms, 3),
          "seconds": round(res.seconds, 3), "apply_block_share": round(apply_ms / (1e3 * res.seconds), 5),
          "correlation_real": [float(c.real) for c in res.correlation], "correlation_imag": [float(c.imag) for c in res.correlation]})


if args.which in ("spin", "both"):
    L, q = args.sites, args.q % args.sites
    kernel_against_columns({"record": "kernel_against_columns", "model": f"heisenberg_chain_{L}", "operator": "S^z_q",
                            "source_symmetries": "translation+reflection+inversion", "target_symmetries": "translation", "target_sector": q},
                           spin_basis(L, 0, full=True), spin_basis(L, q), momentum_op(L, q, " σᶻ₀"))
if args.which in ("fermion", "both"):
    L, q = args.modes, args.q % args.modes
    kernel_against_columns({"record": "kernel_against_columns", "model": f"tV_ring_{L}", "operator": "n_q",
                            "source_symmetries": "translation+reflection", "target_symmetries": "translation", "target_sector": q},
                           fermi_basis(L, 0, full=True), fermi_basis(L, q), momentum_op(L, q, " × n₀"))
if args.thermal:
    for method in ("columns", "kernel"):
        thermal(args.sites, args.q % args.sites, method)
