#!/usr/bin/env python3
"""What ExpectationPlan.matrix_elements (k_expect_mat / k_expect_mat_fermi) costs for Ka = Kb = 8 interleaved columns -- 64 matrix
elements per operator in one pass -- next to
  (a) the polarisation route for the same 64 elements: 256 complex128 columns through ExpectationPlan.values_block (k_expect_blk,
      which the matrix kernel leaves untouched: the code before it), method="polarisation";
  (b) for information, one values_block call at K = 8: the 8 diagonal numbers of the 64.
Shapes, those of scripts/expect_block_bench.py:
  dimer  dimer_correlations' operator batch -- the reference bond (0, 1) against all bonds -- on heisenberg_chain_32 with
         translations, sector k = 0 in float64 and k = 3 in complex128;
  pair   pair_correlations' batch, all L^2 entries, on the Hubbard ring of 14 sites (2 x 14 modes) at (7, 7), k = 0, float64.
Device events around each variant, --warmup untimed runs and --steps timed ones, min-max reported.  Every call ends synchronised (the
values come back to the host), so an event pair spans the whole call.  The two routes are compared in the same run.  One JSON line per
shape, appended to --out.
usage: expect_matrix_bench.py [--shapes dimer_k0,dimer_k3,pair] [--sites-dimer 32] [--sites-pair 14] [--columns 8] [--steps 3]
                              [--warmup 1] [--out profiles/expect_matrix_bench.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config  # noqa: E402
from distributed_matvec_amd.expectation import dimer_section, pair_section  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="dimer_k0,dimer_k3,pair")
ap.add_argument("--sites-dimer", type=int, default=32)
ap.add_argument("--sites-pair", type=int, default=14)
ap.add_argument("--columns", type=int, default=8)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
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

    def block(seed):
        b = torch.stack([D.fillRandom(reps[0], seed + c, dtype) for c in range(K)], dim=1).contiguous()
        return b / torch.linalg.vector_norm(b, dim=0)

    bra, ket = block(1), block(101)
    specs = [config.parse_operator(sec, basis.spec) for sec in operators]
    # the tolerance of the tests per operator: 2e-11 max(1, sum |v|); 8 of them between the two routes
    atol = np.array([2e-11 * max(1.0, sum(abs(t[0]) for t in s.terms)) for s in specs])[:, None, None]
    plan = D.ExpectationPlan(basis, reps[0], specs)
    t_kernel = timed(lambda: plan.matrix_elements(bra, ket, method="kernel"))
    t_pol = timed(lambda: plan.matrix_elements(bra, ket, method="polarisation"))
    t_diag = timed(lambda: plan.values_block(ket))
    a, b = plan.matrix_elements(bra, ket, method="kernel"), plan.matrix_elements(bra, ket, method="polarisation")
    ratio = float((np.abs(a - b) / (8 * atol)).max())
    rec = {"shape": name, "model": model, "symmetries": "translation", "sector": k, "dtype": "f64" if dtype == torch.float64 else "c128", "n": n,
           "bra_columns": K, "ket_columns": K, "operators": len(operators), "device_terms": plan.num_terms, "flip_groups": plan.num_groups,
           "kernel": plan.matrix_kernel(K, K, method="kernel"), "block_kernel": plan.block_kernel(K), "auto": plan.matrix_kernel(K, K, method="auto"),
           "steps": args.steps, "warmup": args.warmup, "matrix_elements_kernel_ms": t_kernel, "polarisation_ms": t_pol,
           "polarisation_columns": 4 * K * K, "values_block_diagonal_ms": t_diag,
           "kernel_over_polarisation": [round(t_kernel["min"] / t_pol["max"], 3), round(t_kernel["max"] / t_pol["min"], 3)],
           "kernel_over_diagonal_block": [round(t_kernel["min"] / t_diag["max"], 3), round(t_kernel["max"] / t_diag["min"], 3)],
           "max_difference_between_routes": float(np.abs(a - b).max()), "max_difference_over_8_atol": ratio, "routes_agree": ratio <= 1.0}
    plan.destroy()
    emit(rec)
    if ratio > 1.0:
        raise SystemExit(f"{name}: the kernel and the polarisation route differ by {ratio:.3g} x (8 ATOL)")


for s in [x for x in args.shapes.split(",") if x]:
    run(s)
