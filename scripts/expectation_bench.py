#!/usr/bin/env python3
"""What the expectation values of multi-site operators on a sector state cost (ExpectationPlan: k_expect / k_expect_fermi) next to
the route without the plan: one hand-averaged Hermitian Operator per distance through MatvecPlan + vdot, with and without the creation
of its plan, timed on --orbits distances and extrapolated to all of them.  Two workloads:
  dimer  dimer_correlations on the Heisenberg ring of --sites sites (half filling, translations, sector 0): one reference bond (0, 1)
         against all bonds (b, b + 1).  The hand average of distance d is L^-1 sum_t (D_t D_{t+d} + D_{t+d} D_t) / 2, D_t = S_t.S_{t+1},
         whose expectation is Re <D_0 D_d>.
  pair   pair_correlations on the Hubbard ring of --sites sites (2 x sites modes, half filling, translations, sector 0): all L^2 entries.
         The hand average of distance d is L^-1 sum_t (Delta+_t Delta_{t+d} + h.c.), whose expectation is 2 Re P[0][d] (d = 0: 2 P[0][0]).
The state is a normalised random vector.  Every figure is the range over --steps timed runs after --warmup untimed ones, wall time
around a call that ends synchronised.  One JSON line per workload, appended to --out.
usage: expectation_bench.py [--workload dimer|pair|both] [--sites N] [--steps 3] [--warmup 1] [--orbits 3]
                            [--out profiles/expectation_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd.expectation import dimer_section, pair_section  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="both", choices=["dimer", "pair", "both"])
ap.add_argument("--sites", type=int, default=0, help="0: 32 for dimer, 14 for pair")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--orbits", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
dtype = torch.float64


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def series(fn):
    for _ in range(args.warmup):
        fn()
    t = sorted(wall(fn)[0] for _ in range(args.steps))
    return {"min": round(t[0], 3), "median": round(t[len(t) // 2], 3), "max": round(t[-1], 3)}


def run(workload):
    L = args.sites or (32 if workload == "dimer" else 14)
    symmetries = [{"permutation": [(i + 1) % L for i in range(L)], "sector": 0}]
    if workload == "dimer":
        basis_cfg = {"number_spins": L, "hamming_weight": L // 2, "symmetries": symmetries}
        name = f"heisenberg_chain_{L}"
        operators = [dimer_section((0, 1), (b, (b + 1) % L)) for b in range(L)]

        def averaged(d):  # Hermitian: both orders, half each
            terms = []
            for t in range(L):
                a, b = (t, (t + 1) % L), ((t + d) % L, (t + d + 1) % L)
                terms += dimer_section(a, b, 0.5 / L)["terms"] + dimer_section(b, a, 0.5 / L)["terms"]
            return terms

        def expected(vals, d):
            return vals[d].real
    else:
        basis_cfg = {"particle": "spinful-fermion", "number_sites": L, "number_particles": 2 * (L // 2), "number_up": L // 2, "symmetries": symmetries}
        name = f"hubbard_ring_{L}"
        operators = [pair_section(i, j) for i in range(L) for j in range(L)]

        def averaged(d):
            terms = []
            for t in range(L):
                terms += pair_section(t, (t + d) % L)["terms"] + pair_section((t + d) % L, t)["terms"]
            return [{"expression": repr(1.0 / L) + " × " + q["expression"], "sites": q["sites"]} for q in terms]

        def expected(vals, d):
            return 2.0 * vals[d].real  # (row i = 0 of the L x L matrix)
    t0 = time.perf_counter()
    basis = D.loadConfigFromDict({"basis": basis_cfg})
    reps, _ = D.enumerateStates(basis, 1)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    n = int(reps[0].numel())
    psi = D.fillRandom(reps[0], 1, dtype)
    psi = psi / torch.linalg.vector_norm(psi)
    y = torch.zeros_like(psi)
    create_ms, plan = wall(lambda: D.ExpectationPlan(basis, reps[0], operators))
    values = series(lambda: plan.values(psi))
    vals = plan.values(psi)
    n_dist = L
    distances = sorted({2, L // 2, 1, L // 4, 0})[: args.orbits] if args.orbits < 5 else list(range(args.orbits))
    orbit_create, orbit_apply, worst = [], [], 0.0
    for d in distances:
        def create():
            _, op = D.loadConfigFromDict({"basis": basis_cfg, "hamiltonian": {"terms": averaged(d)}}, hamiltonian=True)
            return op, D.MatvecPlan(op, reps, dtype)

        ms, (op, oplan) = wall(create)
        orbit_create.append(ms)

        def apply():
            y.zero_()
            oplan.matvec([psi], [y], check=False)
            return complex(torch.vdot(psi, y))

        for _ in range(args.warmup):
            apply()
        runs = sorted((wall(apply) for _ in range(args.steps)), key=lambda r: r[0])
        orbit_apply.append(runs[len(runs) // 2][0])
        worst = max(worst, abs(runs[0][1] - expected(vals, d)))
        del oplan, op
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    route = n_dist * mean(orbit_apply)
    route_create = n_dist * (mean(orbit_apply) + mean(orbit_create))
    rec = {"workload": workload, "model": name, "symmetries": "translation", "sector": 0, "dtype": "f64", "n": n, "operators": len(operators),
           "device_terms": plan.num_terms, "flip_groups": plan.num_groups, "kernel": plan.kernel(), "steps": args.steps, "warmup": args.warmup,
           "plan_create_ms": round(create_ms, 3), "values_ms": values,
           "orbit_distances": distances, "orbit_create_ms": [round(v, 3) for v in orbit_create],
           "orbit_matvec_dot_ms": [round(v, 3) for v in orbit_apply], "orbits": n_dist,
           "orbit_route_ms_extrapolated": round(route, 3), "orbit_route_with_creation_ms_extrapolated": round(route_create, 3),
           "plan_over_orbit_route": round(values["median"] / route, 3),
           "plan_with_creation_over_orbit_route_with_creation": round((values["median"] + create_ms) / route_create, 3),
           "orbit_route_max_difference": float(worst), "setup_seconds": round(setup_s, 2)}
    plan.destroy()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


for w in (("dimer", "pair") if args.workload == "both" else (args.workload,)):
    run(w)
