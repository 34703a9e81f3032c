#!/usr/bin/env python3
"""What a cross-sector product between bases with DIFFERENT symmetry groups costs (CrossSectorPlan(groups=...)): the operator
O_q = sum_j e^{-2 pi i q j / L} o_j (o = sigma^z on the Heisenberg ring at half filling, o = n on the t-V ring at half filling) into the
translations-only sector k = q,
  (a) groups="restrict" from the sector with every symmetry (k = 0, reflection 0, and spin inversion +1 on the spin ring),
  (b) today's same-generator plan from the translations-only k = 0 sector into the same target -- the comparison for (a): the same
      kernel on the same target rows, a source with 2-4 times as many rows,
  (c) groups="project" on the pair of (a): the sum over the |G2| = L elements of the target group around the same stages.
Each is timed by device events, one warm-up and --steps timed applies (default 3), reported as min - max; the three alternate
inside one process.  One JSON line per run, appended to --out.
usage: cross_groups_bench.py [--model heisenberg|tv] [--sites 32|28] [--q 5] [--steps 3] [--warmup 1] [--out profiles/cross_groups_bench.jsonl]"""
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
ap.add_argument("--model", default="heisenberg", choices=["heisenberg", "tv"])
ap.add_argument("--sites", type=int, default=None, help="default: 32 (heisenberg), 28 (tv)")
ap.add_argument("--q", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
spin = args.model == "heisenberg"
L = args.sites or (32 if spin else 28)
q = args.q % L
dtype = torch.complex128
torch.cuda.set_device(0)

T = [(i + 1) % L for i in range(L)]
R = [L - 1 - i for i in range(L)]


def basis(k, reflection=None, inversion=None):
    sym = [{"permutation": T, "sector": k}]
    if reflection is not None:
        sym.append({"permutation": R, "sector": reflection})
    if spin:
        b = {"number_spins": L, "hamming_weight": L // 2, "symmetries": sym}
        if inversion is not None:
            b["spin_inversion"] = inversion
    else:
        b = {"particle": "spinless-fermion", "number_sites": L, "number_particles": L // 2, "symmetries": sym}
    return {"basis": b}


def phase(j):
    z = cmath.exp(-2j * math.pi * q * j / L)
    return "(" + repr(z.real) + ("+" if z.imag >= 0 else "-") + repr(abs(z.imag)) + "j)"


def operator(on):
    one = " σᶻ₀" if spin else " × n₀"
    return D.Operator.fromSpec(on, config.parse_operator({"terms": [{"expression": phase(j) + one, "sites": [[j]]} for j in range(L)]}, on.spec))


t0 = time.perf_counter()
full = D.loadConfigFromDict(basis(0, 0, 1 if spin else None))  # every symmetry
trans = D.loadConfigFromDict(basis(0))
target = D.loadConfigFromDict(basis(q))
freps, treps, dreps = (D.enumerateStates(b, 1)[0][0] for b in (full, trans, target))
plans = {"restrict": D.CrossSectorPlan(operator(full), freps, target, dreps, dtype, groups="restrict"),
         "same": D.CrossSectorPlan(operator(trans), treps, target, dreps, dtype),
         "project": D.CrossSectorPlan(operator(full), freps, target, dreps, dtype, groups="project")}
xs = {"restrict": D.fillRandom(freps, 1, dtype), "same": D.fillRandom(treps, 1, dtype)}
xs["project"] = xs["restrict"]
y = torch.zeros(dreps.numel(), dtype=dtype, device="cuda")
torch.cuda.synchronize()
setup_s = time.perf_counter() - t0


def timed(name):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    plans[name].apply(xs[name], y, check=False)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


for _ in range(args.warmup):
    for name in plans:
        timed(name)
for p in plans.values():
    p.check()
ms = {name: [] for name in plans}
for _ in range(args.steps):  # alternating
    for name in plans:
        ms[name].append(timed(name))
for p in plans.values():
    p.check()
lo = {name: min(v) for name, v in ms.items()}
order = L  # |G2|: the translations of the target
rec = {"model": (f"heisenberg_chain_{L}" if spin else f"tV_ring_{L}"), "operator": "S^z_q" if spin else "n_q", "q": q, "dtype": "c128",
       "source_symmetries": "translation+reflection" + ("+inversion" if spin else ""), "target_symmetries": "translation", "target_group_order": order,
       "n_source_full": int(freps.numel()), "n_source_translation": int(treps.numel()), "n_target": int(dreps.numel()),
       "steps": args.steps, "warmup": args.warmup, "setup_seconds": round(setup_s, 2)}
for name, p in plans.items():
    rec[name] = {"kernel": p.kernel, "nnz": p.nnz, "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4)}
rec["restrict_over_same"] = round(lo["restrict"] / lo["same"], 4)
rec["project_over_restrict"] = round(lo["project"] / lo["restrict"], 4)
rec["project_over_restrict_per_element"] = round(lo["project"] / lo["restrict"] / order, 4)
line = json.dumps(rec)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
