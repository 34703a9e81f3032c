#!/usr/bin/env python3
"""diagonalize.interior_eigenpairs at mid-band: order of the filter, filter applications, columns x orders, polish rounds, wall time
and its split into filter / Lanczos orthogonalisation / Rayleigh-Ritz, per model, (num_evals, block_size), LS_AMD_BLOCK mode and cut.
Models: rf_chain_L (the Heisenberg ring of L sites at weight L / 2 with fields h_i sigma^z_i, h_i uniform in [-1, 1] from seed 5, no
symmetries, f64) and chain_24_k (the translation sector k = 3 of heisenberg_chain_24, c128).  --warmup (1) warm-up and --runs timed runs per
line (median, min, max of the wall time; every run synchronises the device before and after).  Bounds and the density of states at
sigma are computed once per model outside the timed region and handed to every run, so the runs of one line do the same work.
--full-spectrum adds, for models of at most 32768 states, the time of diagonalize.full_spectrum and the largest deviation of the
interior levels from it.
usage: interior_bench.py [--models rf_chain_16,...] [--settings 8:8,32:16] [--modes auto,kernel] [--cuts 0.17] [--runs 3] [--warmup 1]
                         [--eps 1e-9] [--full-spectrum] [--out profiles/interior_bench.jsonl]"""
import argparse
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config, kpm  # noqa: E402
from distributed_matvec_amd import diagonalize as dg  # noqa: E402


def model(name):
    m = re.fullmatch(r"rf_chain_(\d+)", name)
    if m:
        L = int(m.group(1))
        cfg = config.heisenberg_chain_config(L)
        h = np.random.RandomState(5).uniform(-1.0, 1.0, L)
        cfg["hamiltonian"]["terms"] += [{"expression": f"{float(h[i])!r} × σᶻ₀", "sites": [[i]]} for i in range(L)]
        return cfg, torch.float64
    m = re.fullmatch(r"chain_(\d+)_k", name)
    if m:
        L = int(m.group(1))
        cfg = config.heisenberg_chain_config(L)
        cfg["basis"]["symmetries"] = [{"permutation": [(i + 1) % L for i in range(L)], "sector": 3}]
        return cfg, torch.complex128
    raise SystemExit(f"unknown model {name}")


ap = argparse.ArgumentParser()
ap.add_argument("--models", default="rf_chain_16")
ap.add_argument("--settings", default="8:8,8:16,32:8,32:16", help="num_evals:block_size,...")
ap.add_argument("--modes", default="auto", help="LS_AMD_BLOCK values")
ap.add_argument("--cuts", default="0.17")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--eps", type=float, default=1e-9)
ap.add_argument("--full-spectrum", action="store_true")
ap.add_argument("--out", default=None, help="append the JSON lines here as well")
args = ap.parse_args()
torch.cuda.set_device(0)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


for name in [m for m in args.models.split(",") if m]:
    cfg, dtype = model(name)
    t0 = time.perf_counter()
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    op = dg.LocalOperator(h, reps, dtype)
    n = op.n_local
    bounds = kpm.spectral_bounds(op)
    sigma = 0.5 * (bounds[0] + bounds[1])
    dos = kpm._dos_at(op, sigma, bounds)
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    exact = None
    if args.full_spectrum and n <= 32768:
        fs = dg.full_spectrum(cfg, dtype=dtype)
        exact = np.asarray(fs.eigenvalues)
        emit({"model": name, "N": n, "driver": "full_spectrum", "seconds": round(fs.seconds, 3)})
    for mode in args.modes.split(","):
        os.environ["LS_AMD_BLOCK"] = mode
        for setting in args.settings.split(","):
            k, K = (int(v) for v in setting.split(":"))
            guard = max(K, k // 4)
            while guard > 0 and 2 * (k + guard) + 3 * K > 128:  # (the basis window of lanczos_block_smallest: 32:16 runs with guard 8)
                guard -= 1
            for cut in (float(c) for c in args.cuts.split(",")):
                order = kpm.filter_order(k + guard, n, dos, bounds, cut=cut, sigma=sigma)
                runs = []
                for it in range(args.runs + args.warmup):
                    torch.cuda.synchronize()
                    r = dg.interior_eigenpairs(op, sigma, num_evals=k, eps=args.eps, block_size=K, order=order, guard=guard, bounds=bounds)
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        runs.append(r)
                secs = [r.seconds for r in runs]
                r = runs[len(runs) // 2]
                rec = {"model": name, "N": n, "dtype": "c128" if dtype == torch.complex128 else "f64", "mode": mode, "kernel": r.kernel,
                       "num_evals": k, "block_size": K, "guard": guard, "cut": cut, "eps": args.eps, "sigma": sigma,
                       "bounds": list(bounds), "dos_at_sigma": dos, "order": r.order, "applications": r.applications,
                       "columns_x_orders": r.matvecs, "lanczos_restarts": r.lanczos_restarts, "polish_rounds": r.polish_rounds,
                       "converged": all(q.converged for q in runs), "max_residual_over_norm": max(r.residual_norms) / max(abs(bounds[0]), abs(bounds[1])),
                       "runs": len(runs), "seconds_median": round(statistics.median(secs), 3), "seconds_min": round(min(secs), 3),
                       "seconds_max": round(max(secs), 3), "filter_seconds": round(r.filter_seconds, 3),
                       "orth_seconds": round(r.orth_seconds, 3), "ritz_seconds": round(r.ritz_seconds, 3), "setup_seconds": round(setup, 3)}
                if exact is not None:
                    near = np.sort(exact[np.argsort(np.abs(exact - sigma))[:k]])
                    rec["max_level_deviation"] = float(np.abs(np.array(r.eigenvalues) - near).max())
                emit(rec)
    os.environ.pop("LS_AMD_BLOCK", None)
