#!/usr/bin/env python3
"""What the correlation matrices of a sector state cost (CorrelationPlan: k_corr_diag, k_corr_hop / k_corr_hop_fermi) next to
  (b) one matvec of H in the same sector, by the kernel the library picks for that basis, and
  (c) the route without the plan: one group-averaged Operator per orbit of ordered pairs -- on a ring with translations the orbit of
      (i, j) is the distance d = j - i -- a matvec plan for each, one matvec and one dot.  The pull plans of a projected basis take
      Hermitian operators, so the operator of a distance is L^-1 sum_t (B+_t B_{t+d} + h.c.), whose expectation is 2 Re G[0][d]; the
      imaginary parts need the i (.. - h.c.) combinations, and d and L - d share both: L - 1 operators for the L - 1 distances.
      Timed with and without the creation of its plan on --orbits distances and extrapolated to L - 1.
--model heisenberg: the Heisenberg ring of --sites sites at half filling with translations, sector --sector; --model tv: the t-V ring
(spinless fermions, N = sites / 2).  The state is a normalised random vector.  Every figure is the range over --steps timed runs after
--warmup untimed ones, wall time around a call that ends synchronised (the plan's calls synchronise themselves; the matvec and the
orbit route are followed by a device synchronisation).  One JSON line, appended to --out.
usage: correlations_bench.py [--model heisenberg] [--sites 32] [--sector 0] [--dtype f64] [--steps 5] [--warmup 2] [--orbits 3]
                             [--out profiles/correlations_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="heisenberg", choices=["heisenberg", "tv"])
ap.add_argument("--sites", type=int, default=32)
ap.add_argument("--sector", type=int, default=0)
ap.add_argument("--V", type=float, default=1.0)
ap.add_argument("--dtype", default="f64", choices=["f64", "c128"])
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--orbits", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = args.sites
dtype = torch.complex128 if args.dtype == "c128" else torch.float64
torch.cuda.set_device(0)
ring = [[i, (i + 1) % L] for i in range(L)]
symmetries = [{"permutation": [(i + 1) % L for i in range(L)], "sector": args.sector}]
if args.model == "heisenberg":
    basis_cfg = {"number_spins": L, "hamming_weight": L // 2, "symmetries": symmetries}
    h_terms = [{"expression": e, "sites": ring} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]
    pair_expression = "σ⁻₀ σ⁺₁"  # B+_i B_j: sigma^- sets a bit
else:
    basis_cfg = {"particle": "spinless-fermion", "number_sites": L, "number_particles": L // 2, "symmetries": symmetries}
    h_terms = [{"expression": "-1.0 × c†₀ c₁", "sites": ring}, {"expression": "-1.0 × c†₁ c₀", "sites": ring},
               {"expression": repr(float(args.V)) + " × n₀ n₁", "sites": ring}]
    pair_expression = "c†₀ c₁"


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


t0 = time.perf_counter()
basis, h = D.loadConfigFromDict({"basis": basis_cfg, "hamiltonian": {"terms": h_terms}}, hamiltonian=True)
reps, _ = D.enumerateStates(basis, 1)
n = int(reps[0].numel())
plan = D.MatvecPlan(h, reps, dtype)
torch.cuda.synchronize()
setup_s = time.perf_counter() - t0
psi = D.fillRandom(reps[0], 1, dtype)
psi = psi / torch.linalg.vector_norm(psi)
y = torch.zeros_like(psi)

create_ms, corr = wall(lambda: D.CorrelationPlan(basis, reps[0]))
dens = series(lambda: corr.densities(psi))
hops = series(lambda: corr.hoppings(psi))
raw = series(lambda: corr.hoppings(psi, symmetrize=False))
def do_matvec():
    y.zero_()
    plan.matvec([psi], [y], check=False)


matvec = series(do_matvec)
plan.check()
G = corr.hoppings(psi)

# (c) the orbits of ordered pairs under the translations: the distances 1 .. L - 1
distances = sorted({1, L // 4, L // 2, 3, L - 1})[: args.orbits] if args.orbits < 5 else list(range(1, args.orbits + 1))
orbit_create, orbit_apply, worst = [], [], 0.0
for dist in distances:
    terms = [{"expression": repr(1.0 / L) + " × " + pair_expression, "sites": [[t, (t + dist) % L] for t in range(L)]},
             {"expression": repr(1.0 / L) + " × " + pair_expression, "sites": [[(t + dist) % L, t] for t in range(L)]}]

    def create():
        _, op = D.loadConfigFromDict({"basis": basis_cfg, "hamiltonian": {"terms": terms}}, hamiltonian=True)
        return op, D.MatvecPlan(op, reps, dtype)

    ms, (op, oplan) = wall(create)
    orbit_create.append(ms)

    def apply():
        y.zero_()  # (matrixVectorProduct adds to y)
        oplan.matvec([psi], [y], check=False)
        return complex(torch.vdot(psi, y))

    for _ in range(args.warmup):
        apply()
    runs = sorted((wall(apply) for _ in range(args.steps)), key=lambda r: r[0])
    orbit_apply.append(runs[len(runs) // 2][0])
    worst = max(worst, abs(runs[0][1] - 2.0 * G[0, dist % L].real))
    del oplan, op
n_orbits = L - 1
mean = lambda v: sum(v) / len(v)  # noqa: E731
rec = {"model": ("heisenberg_chain_" if args.model == "heisenberg" else "tV_ring_") + str(L), "symmetries": "translation", "sector": args.sector,
       "dtype": args.dtype, "n": n, "modes": corr.modes, "kernels": [corr.kernel(0), corr.kernel(1)], "matvec_kernel": plan.kernel,
       "steps": args.steps, "warmup": args.warmup,
       "plan_create_ms": round(create_ms, 3), "densities_ms": dens, "hoppings_ms": hops, "hoppings_raw_ms": raw, "matvec_ms": matvec,
       "hoppings_over_matvec": round(hops["median"] / matvec["median"], 3),
       "orbit_distances": distances, "orbit_create_ms": [round(v, 3) for v in orbit_create], "orbit_matvec_dot_ms": [round(v, 3) for v in orbit_apply],
       "orbits": n_orbits, "orbit_route_ms_extrapolated": round(n_orbits * mean(orbit_apply), 3),
       "orbit_route_with_creation_ms_extrapolated": round(n_orbits * (mean(orbit_apply) + mean(orbit_create)), 3),
       "orbit_route_max_difference": float(worst), "setup_seconds": round(setup_s, 2)}
line = json.dumps(rec)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
