#!/usr/bin/env python3
"""The CSR export of a sector matrix next to the products it replaces, and the dense full-spectrum solve.
For every export case (a translation sector of the Heisenberg ring, complex128): one JSON line with
  export_ms   CrossSectorPlan.to_csr: counting pass, scan, fill, merge, scan, write, and the copies into torch tensors
  apply_ms    one CrossSectorPlan.apply of the same plan (what one emitting pass costs at the least)
  matvec_ms   one MatvecPlan.matvec on the same sector (the production kernel family)
  packets, nnz, csr_bytes (the arrays of the result), bound_bytes (ls_amd_cross_csr_bytes: the peak of the export)
and for --spectrum one line with the seconds of diagonalize.full_spectrum (enumeration, export, dense matrix, eigvalsh).
Every time is a wall clock between two device synchronisations, after --warmup runs, repeated --repeats times: median, min, max.
Appends to profiles/sector_matrix_bench.jsonl (--out).
usage: sector_matrix_bench.py [--cases 24:12:5,32:16:5] [--spectrum 20:10:0] [--repeats 5] [--warmup 1] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd.diagonalize import full_spectrum  # noqa: E402


def ring(L, weight, k):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"basis": {"number_spins": L, "hamming_weight": weight,
                      "symmetries": [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]},
            "hamiltonian": {"name": "Heisenberg", "terms": [{"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds},
                                                            {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}}


ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="24:12:5,32:16:5", help="sites:weight:momentum of the export cases")
ap.add_argument("--spectrum", default="20:10:0", help="sites:weight:momentum of the full_spectrum case ('' to skip)")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector_matrix_bench.jsonl"))
args = ap.parse_args()
torch.cuda.set_device(0)
out = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(fn):
    """median, min, max milliseconds of fn between device synchronisations"""
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3), "repeats": len(ts)}


for case in [c for c in args.cases.split(",") if c]:
    L, w, k = (int(v) for v in case.split(":"))
    dtype = torch.complex128
    basis, h = D.loadConfigFromDict(ring(L, w, k), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    n = int(reps[0].numel())
    plan = D.CrossSectorPlan(h, reps[0], basis, reps[0], dtype)
    mv = D.MatvecPlan(h, reps, dtype)
    x = D.fillRandom(reps[0], 7, dtype)
    y = torch.zeros_like(x)
    bound = plan.csr_bytes
    csr = plan.to_csr(max_bytes=bound)
    nnz = csr.nnz
    csr_bytes = sum(t.numel() * t.element_size() for t in (csr.crow_indices, csr.col_indices, csr.values))
    # the export is the matrix of both products
    z = torch.zeros_like(x)
    z.index_add_(0, csr.row_indices(), csr.values * x[csr.col_indices])
    plan.apply(x, y)
    assert float((z - y).abs().max()) <= 1e-12 * 3 * L * float(x.abs().max())
    mv.matvec([x], [y])
    assert float((z - y).abs().max()) <= 1e-12 * 3 * L * float(x.abs().max())
    del csr, z

    def export():
        plan.to_csr(max_bytes=bound)

    rec = {"model": f"heisenberg_ring_{L}", "weight": w, "momentum": k, "rows": n, "dtype": "c128", "kernel": plan.kernel,
           "matvec_kernel": mv.kernel, "packets": plan.nnz, "nnz": nnz, "csr_bytes": csr_bytes, "bound_bytes": bound,
           "export_ms": timed(export), "apply_ms": timed(lambda: plan.apply(x, y, check=False)),
           "matvec_ms": timed(lambda: mv.matvec([x], [y], check=False))}
    emit(rec)
    plan.destroy()
    mv.destroy()
    del x, y, reps, plan, mv
    torch.cuda.empty_cache()

if args.spectrum:
    L, w, k = (int(v) for v in args.spectrum.split(":"))
    cfg = ring(L, w, k)
    res = None

    def solve():
        global res
        res = full_spectrum(cfg)

    t = timed(solve)
    emit({"model": f"heisenberg_ring_{L}", "weight": w, "momentum": k, "driver": "full_spectrum", "rows": res.dimension,
          "dtype": "f64" if k in (0, L // 2) else "c128", "eigenvalue_min": float(res.eigenvalues[0]), "eigenvalue_max": float(res.eigenvalues[-1]),
          "ms": t})
