#!/usr/bin/env python3
"""What one cross-sector product between projected FERMIONIC bases costs next to one matvec of H: c+_q = sum_j e^{-2 pi i q j / L} c+_j
on the t-V ring of --sites sites with translation symmetry, from the N = --particles, k = 0 sector into N + 1, k = q
(CrossSectorPlan, k_cross_pull_fermi), against one matvec of H = -t sum (c+_i c_{i+1} + h.c.) + V sum n_i n_{i+1} in the TARGET
sector by the kernel the library picks for that basis.  A photoemission spectrum runs the cross product once and M / 2 Chebyshev
steps, so the ratio is the figure that matters.  The same plan and the same timing as scripts/cross_sector_bench.py: the two
alternate inside one process after a warm-up; each is timed by device events (the matvec also by the plan's own event pairs);
medians over --steps.  One JSON line, appended to --out.
usage: fermion_cross_bench.py [--sites 28] [--particles L/2] [--q L/2] [--dtype c128] [--steps 10] [--warmup 2] [--out profiles/fermion_cross_bench.jsonl]"""
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
from distributed_matvec_amd import config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sites", type=int, default=28)
ap.add_argument("--particles", type=int, default=None, help="particles of the source sector (default: sites / 2)")
ap.add_argument("--V", type=float, default=1.0)
ap.add_argument("--q", type=int, default=None, help="target momentum sector (default: sites / 2)")
ap.add_argument("--dtype", default="c128", choices=["f64", "c128"])
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = args.sites
q = L // 2 if args.q is None else args.q % L
dtype = torch.complex128 if args.dtype == "c128" else torch.float64
torch.cuda.set_device(0)


N = L // 2 if args.particles is None else args.particles


def ring(n, k):
    """the t-V ring with n particles in momentum sector k"""
    terms = [{"expression": "-1.0 × c†₀ c₁", "sites": [[i, (i + 1) % L] for i in range(L)]},
             {"expression": "-1.0 × c†₁ c₀", "sites": [[i, (i + 1) % L] for i in range(L)]},
             {"expression": repr(float(args.V)) + " × n₀ n₁", "sites": [[i, (i + 1) % L] for i in range(L)]}]
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": n,
                      "symmetries": [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]},
            "hamiltonian": {"terms": terms}}


def phase(j):
    z = cmath.exp(-2j * math.pi * q * j / L)
    if 2 * q % L == 0:
        z = complex(round(z.real), 0.0)  # exp(-i pi j): exactly +-1, so that f64 is admissible
    return "(" + repr(z.real) + ("+" if z.imag >= 0 else "-") + repr(abs(z.imag)) + "j)"


t0 = time.perf_counter()
sbasis = D.loadConfigFromDict(ring(N, 0))
tbasis, h_t = D.loadConfigFromDict(ring(N + 1, q), hamiltonian=True)
A = D.Operator.fromSpec(sbasis, config.parse_operator({"terms": [{"expression": phase(j) + " × c†₀", "sites": [[j]]} for j in range(L)]}, sbasis.spec))
sreps, _ = D.enumerateStates(sbasis, 1)
treps, _ = D.enumerateStates(tbasis, 1)
cross = D.CrossSectorPlan(A, sreps[0], tbasis, treps[0], dtype)
plan = D.MatvecPlan(h_t, treps, dtype)
plan.enable_timing(args.steps + args.warmup + 4)
torch.cuda.synchronize()
setup_s = time.perf_counter() - t0
x = D.fillRandom(sreps[0], 1, dtype)
v = torch.zeros(treps[0].numel(), dtype=dtype, device="cuda")
w = torch.zeros_like(v)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def do_cross():
    cross.apply(x, v, check=False)


def do_matvec():
    plan.matvec([v], [w], check=False)


for _ in range(args.warmup):
    do_cross()
    do_matvec()
cross.check()
plan.check()
warm = len(plan.kernel_times_ms())
tc, tm = [], []
for _ in range(args.steps):  # alternating
    tc.append(timed(do_cross))
    tm.append(timed(do_matvec))
cross.check()
plan.check()
own = sorted(plan.kernel_times_ms()[warm:])
tc.sort()
tm.sort()
med = lambda t: t[len(t) // 2]  # noqa: E731
rec = {"model": f"tV_ring_{L}", "V": args.V, "symmetries": "translation", "operator": "c+_q", "source_particles": N, "target_particles": N + 1,
       "source_sector": 0, "target_sector": q,
       "dtype": args.dtype, "n_source": int(sreps[0].numel()), "n_target": int(treps[0].numel()), "cross_kernel": cross.kernel,
       "cross_nnz": cross.nnz, "matvec_kernel": plan.kernel, "matvec_nnz": plan.nnz, "steps": args.steps, "warmup": args.warmup,
       "cross_ms_median": round(med(tc), 4), "cross_ms_min": round(tc[0], 4), "cross_ms_max": round(tc[-1], 4),
       "matvec_ms_median": round(med(tm), 4), "matvec_ms_min": round(tm[0], 4), "matvec_ms_max": round(tm[-1], 4),
       "matvec_ms_median_plan_events": round(med(own), 4) if own else None,
       "cross_over_matvec": round(med(tc) / med(tm), 4), "setup_seconds": round(setup_s, 2)}
line = json.dumps(rec)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
