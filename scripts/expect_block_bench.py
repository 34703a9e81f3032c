#!/usr/bin/env python3
"""What ExpectationPlan.values_block (k_expect_blk / k_expect_blk_fermi) costs for a block of K = 8 states next to 8 calls of
ExpectationPlan.values (k_expect / k_expect_fermi, which the block form leaves untouched: the single-state kernel of the same build
stands in for the code before the block form).  Shapes, those of scripts/expectation_bench.py:
  dimer  dimer_correlations' operator batch -- the reference bond (0, 1) against all bonds -- on heisenberg_chain_32 with
         translations, sector k = 0 in float64 and k = 3 in complex128;
  pair   pair_correlations' batch, all L^2 entries, on the Hubbard ring of 14 sites (2 x 14 modes) at (7, 7), k = 0, float64.
Each shape: values_block with interleaved columns (strides (K, 1)) and with column-major ones (strides (1, n)), and K calls of values
on contiguous columns.  Device events around each variant, --warmup untimed runs and --steps timed ones, min-max reported.  Every call
ends synchronised (the values come back to the host), so an event pair spans the whole call.  With --thermal one
evolve.thermal_expectation run (K = 8, four betas) on the k = 0 sector of the chain, with the share of its wall time spent inside
values_block.  One JSON line per shape, appended to --out.
usage: expect_block_bench.py [--shapes dimer_k0,dimer_k3,pair] [--sites-dimer 32] [--sites-pair 14] [--columns 8] [--steps 3]
                             [--warmup 1] [--thermal] [--out profiles/expect_block_bench.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd.expectation import dimer_section, pair_section  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="dimer_k0,dimer_k3,pair")
ap.add_argument("--sites-dimer", type=int, default=32)
ap.add_argument("--sites-pair", type=int, default=14)
ap.add_argument("--columns", type=int, default=8)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--thermal", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)


def timed(fn):
    """[ms] of --steps runs between device events, after --warmup untimed ones"""
    for _ in range(args.warmup):
        fn()
    out = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"min": round(min(out), 3), "max": round(max(out), 3)}


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def shape(name):
    if name.startswith("dimer"):
        L, k = args.sites_dimer, int(name.split("_k")[1])
        basis_cfg = {"number_spins": L, "hamming_weight": L // 2, "symmetries": [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]}
        model = f"heisenberg_chain_{L}"
        operators = [dimer_section((0, 1), (b, (b + 1) % L)) for b in range(L)]
        dtype = torch.float64 if k in (0, L // 2) else torch.complex128
    else:
        L, k = args.sites_pair, 0
        basis_cfg = {"particle": "spinful-fermion", "number_sites": L, "number_particles": 2 * (L // 2), "number_up": L // 2,
                     "symmetries": [{"permutation": [(i + 1) % L for i in range(L)], "sector": 0}]}
        model = f"hubbard_ring_{L}"
        operators = [pair_section(i, j) for i in range(L) for j in range(L)]
        dtype = torch.float64
    return model, k, basis_cfg, operators, dtype


def run(name):
    model, k, basis_cfg, operators, dtype = shape(name)
    K = args.columns
    basis = D.loadConfigFromDict({"basis": basis_cfg})
    reps, _ = D.enumerateStates(basis, 1)
    n = int(reps[0].numel())
    inter = torch.stack([D.fillRandom(reps[0], 1 + c, dtype) for c in range(K)], dim=1).contiguous()
    inter /= torch.linalg.vector_norm(inter, dim=0)
    colmajor = inter.t().contiguous().t()
    cols = [colmajor[:, c] for c in range(K)]  # (contiguous: values takes them as they are)
    plan = D.ExpectationPlan(basis, reps[0], operators)
    single = timed(lambda: [plan.values(c) for c in cols])
    t_inter = timed(lambda: plan.values_block(inter))
    t_col = timed(lambda: plan.values_block(colmajor))
    want = np.stack([plan.values(c) for c in cols], axis=1)
    diff = max(float(np.abs(plan.values_block(inter) - want).max()), float(np.abs(plan.values_block(colmajor) - want).max()))
    rec = {"shape": name, "model": model, "symmetries": "translation", "sector": k, "dtype": "f64" if dtype == torch.float64 else "c128", "n": n,
           "columns": K, "operators": len(operators), "device_terms": plan.num_terms, "flip_groups": plan.num_groups,
           "kernel": plan.block_kernel(K), "single_kernel": plan.kernel(), "steps": args.steps, "warmup": args.warmup,
           "values_x_columns_ms": single, "values_block_interleaved_ms": t_inter, "values_block_column_major_ms": t_col,
           "interleaved_over_single": [round(t_inter["min"] / single["max"], 3), round(t_inter["max"] / single["min"], 3)],
           "column_major_over_single": [round(t_col["min"] / single["max"], 3), round(t_col["max"] / single["min"], 3)],
           "max_difference_from_values": diff}
    plan.destroy()
    emit(rec)


def thermal():
    from distributed_matvec_amd import evolve

    L = args.sites_dimer
    bonds = [[i, (i + 1) % L] for i in range(L)]
    cfg = {"basis": {"number_spins": L, "hamming_weight": L // 2, "symmetries": [{"permutation": [(i + 1) % L for i in range(L)], "sector": 0}]},
           "hamiltonian": {"name": "Heisenberg", "terms": [{"expression": e, "sites": bonds} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]}}
    operators = [dimer_section((0, 1), (b, (b + 1) % L)) for b in range(L)]
    betas = [0.0, 0.1, 0.2, 0.4]
    bounds = (-1.85 * L, 1.05 * L)  # encloses the spectrum of sum sigma.sigma on a ring: E0 > -1.7726 L, E_max = L
    res = evolve.thermal_expectation(cfg, operators, betas, num_vectors=args.columns, seed=1, bounds=bounds)
    emit({"shape": "thermal_expectation", "model": f"heisenberg_chain_{L}", "sector": 0, "dtype": "f64", "n": res.dimension, "columns": args.columns,
          "betas": betas, "operators": len(operators), "orders": res.orders.tolist(), "matvec_columns": res.matvec_columns, "kernel": res.kernel,
          "seconds": round(res.seconds, 3), "values_block_seconds": round(res.expectation_seconds, 3),
          "values_block_share": round(res.expectation_seconds / res.seconds, 3), "energy": [round(float(e), 6) for e in res.energy],
          "specific_heat": [round(float(c), 6) for c in res.specific_heat], "entropy": [round(float(s), 6) for s in res.entropy],
          "first_value": [round(float(v.real), 8) for v in res.values[:, 1]]})


for s in [x for x in args.shapes.split(",") if x]:
    run(s)
if args.thermal:
    thermal()
